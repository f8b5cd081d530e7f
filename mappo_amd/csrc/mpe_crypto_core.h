// mpe_crypto_core.h — the MPE `simple_crypto` environment as device functions: reset, one environment step and the observation
// write, one lane per environment, and the traits (MpeCrypto, at the end) through which the shared kernels reach them: the stepwise
// kernels (mpe_ragged_env.h) and the one-launch rollout episode (rollout_sep_img.h), so a step computes the same values whichever
// launch runs it.
//
// Reference: onpolicy/envs/mpe/environment.py:194-256 (action decoding: an agent that does not move and is not silent speaks its whole
// action vector), :49-50,142 (world.collaborative is not set: per-agent rewards), :179-185 (time-limit done);
// onpolicy/envs/mpe/core.py:280-287 (state.c = action.c, no noise); onpolicy/envs/mpe/scenarios/simple_crypto.py:21-44 (nobody moves
// or collides, dim_c 4), :47-75 (reset), :94-121 (reward), :124-171 (observation); and the reset-on-done of the vec-env wrappers
// (envs/env_wrappers.py:146-152).
//
// There is no arithmetic to round: every observation is a one-hot or zeros and every reward is -2, 0 or 2, so the outputs EQUAL the
// fp32 cast of the reference's (tests/golden/mpe_crypto.npz).  State is device resident; resets draw from the counter-based Philox
// stream keyed by (seed, episode, index) — index layout below.
//
// Fixed shape (num_agents = 3, num_landmarks L = 2, 3 or 4): agent 0 is the ADVERSARY "Eve" (a listener: observes what the speaker
// said, 4 features), agent 1 the good listener "Bob" (the key, then what the speaker said: 8 features), agent 2 the SPEAKER "Alice"
// (the goal, then the key: 8 features).  Nobody moves and nothing collides: every agent only speaks, Discrete(4) = dim_c, and the
// whole state of an environment is five small integers — goal and key (landmark indices; landmark k's colour is the one-hot e_k of
// R^4) and the symbol each agent last said (-1: nothing yet, the reference's zero vector).  The positions the reference also draws
// enter neither an observation nor a reward and are not kept.  The world is NOT collaborative: each agent receives its own reward.
//
// Reset draws: Philox stream (seed, episode), 32-bit word MPE_CRYPTO_DRAWS * n + k of environment n —
//   k = 0                     goal landmark: (word * L) >> 32 in 64-bit arithmetic, so 0 .. L - 1
//   k = 1                     key landmark, the same map of its own word: independent of the goal
// so no two draws of one (seed, episode) share an index.
#pragma once
#include "mpe_core.h"

#define MPE_CRYPTO_M 3
#define MPE_CRYPTO_C 4                                              // dim_c: every agent's action width, and a colour's
#define MPE_CRYPTO_MIN_L 2
#define MPE_CRYPTO_MAX_L 4                                          // landmark k's colour is e_k of R^4
#define MPE_CRYPTO_OBS_E 4                                          // Eve: the speaker's c
#define MPE_CRYPTO_OBS_B 8                                          // Bob: key | the speaker's c
#define MPE_CRYPTO_OBS_A 8                                          // Alice: goal | key
#define MPE_CRYPTO_SHARE (MPE_CRYPTO_OBS_E + MPE_CRYPTO_OBS_B + MPE_CRYPTO_OBS_A)    // the three side by side, Eve first: 20
#define MPE_CRYPTO_DRAWS 2
#define MPE_CRYPTO_SPEAKER 2

struct MpeCryptoArgs {
  int32_t *goal, *key;             // [N] landmark index of every agent's goal_a | of the speaker's key
  int32_t *comm;                   // [N][3] the symbol each agent last said, -1: nothing said (state.c all zeros)
  int32_t *tstep;                  // [N] steps since the last reset
  int64_t *episode;                // [N] resets so far (Philox counter)
  const float *act;                // mode 0: one-hots / probabilities [N][3][4] | mode 1: indices [N][3]
  float *obs[MPE_CRYPTO_M];        // [N][4], [N][8], [N][8]
  float *rewards;                  // [N][3]: one per agent
  uint8_t *dones;                  // [N][3] bool bytes
  int N, T, mode, L;
  uint64_t seed;
};

// the state one lane holds
struct MpeCryptoState {
  int g, k, c[MPE_CRYPTO_M];
  int32_t tstep;
  int64_t episode;
};

__device__ __forceinline__ int mpe_crypto_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a 32-bit word -> 0 .. L - 1
__device__ __forceinline__ int mpe_crypto_draw(uint64_t seed, uint64_t ep, uint64_t idx, int L) {
  return (int)(((uint64_t)philox_u32(seed, ep, idx) * (uint64_t)L) >> 32);
}

// scenario.reset_world (simple_crypto.py:47-75): goal and key each np.random.choice over the landmarks, every c the zero vector
__device__ __forceinline__ void mpe_crypto_reset_env(const MpeCryptoArgs &a, int n, MpeCryptoState &s, int64_t ep) {
  const uint64_t base = (uint64_t)n * MPE_CRYPTO_DRAWS;
  s.g = mpe_crypto_draw(a.seed, (uint64_t)ep, base, a.L);
  s.k = mpe_crypto_draw(a.seed, (uint64_t)ep, base + 1, a.L);
#pragma unroll
  for (int m = 0; m < MPE_CRYPTO_M; ++m) s.c[m] = -1;
}

// four floats: the one-hot of k, all zeros for k = -1
__device__ __forceinline__ void mpe_crypto_onehot(float *o, int k) {
#pragma unroll
  for (int d = 0; d < MPE_CRYPTO_C; ++d) o[d] = d == k ? 1.f : 0.f;
}

// scenario.observation (simple_crypto.py:124-171): Eve [speaker's c], Bob [key | speaker's c], Alice [goal | key]
__device__ __forceinline__ void mpe_crypto_write_obs(float *o0, float *o1, float *o2, const MpeCryptoState &s) {
  mpe_crypto_onehot(o0, s.c[MPE_CRYPTO_SPEAKER]);
  mpe_crypto_onehot(o1, s.k);
  mpe_crypto_onehot(o1 + MPE_CRYPTO_C, s.c[MPE_CRYPTO_SPEAKER]);
  mpe_crypto_onehot(o2, s.g);
  mpe_crypto_onehot(o2 + MPE_CRYPTO_C, s.k);
}

__device__ __forceinline__ void mpe_crypto_load(const MpeCryptoArgs &a, int n, MpeCryptoState &s) {
  s.g = mpe_crypto_clamp(a.goal[n], 0, a.L - 1);
  s.k = mpe_crypto_clamp(a.key[n], 0, a.L - 1);
#pragma unroll
  for (int m = 0; m < MPE_CRYPTO_M; ++m) s.c[m] = mpe_crypto_clamp(a.comm[(size_t)n * MPE_CRYPTO_M + m], -1, MPE_CRYPTO_C - 1);
  s.tstep = a.tstep[n];
  s.episode = a.episode[n];
}

// draws: also the goal, the key and the episode counter (they change only at a reset)
__device__ __forceinline__ void mpe_crypto_store(const MpeCryptoArgs &a, int n, const MpeCryptoState &s, bool draws) {
#pragma unroll
  for (int m = 0; m < MPE_CRYPTO_M; ++m) a.comm[(size_t)n * MPE_CRYPTO_M + m] = s.c[m];
  a.tstep[n] = s.tstep;
  if (draws) {
    a.goal[n] = s.g;
    a.key[n] = s.k;
    a.episode[n] = s.episode;
  }
}

// scenario.reward (simple_crypto.py:94-121) on the state as it stands.  d(a) = |c_a - e_goal|^2: 0 where agent a said the goal's
// symbol, 2 for any other one-hot; an agent whose c is all zeros (-1 here) is skipped.  Eve -d(Eve); Bob and Alice d(Eve) - d(Bob).
__device__ __forceinline__ void mpe_crypto_reward(const MpeCryptoState &s, float (&reward)[MPE_CRYPTO_M]) {
  const float d_eve = s.c[0] < 0 ? 0.f : (s.c[0] == s.g ? 0.f : 2.f);
  const float d_bob = s.c[1] < 0 ? 0.f : (s.c[1] == s.g ? 0.f : 2.f);
  reward[0] = 0.f - d_eve;
  reward[1] = d_eve - d_bob;
  reward[2] = d_eve - d_bob;
}

// One step of environment n on the state the lane holds: the three actions -> the symbols said, per-agent rewards, time-limit done,
// reset-on-done, observations.  act: the environment's own actions (a.mode 0: [3][4] floats, the symbol is the index of the row's
// first maximum | 1: [3] indices, clamped to 0 .. 3; stride act_stride floats between the agents); o0 / o1 / o2: its three
// observation rows (4, 8 and 8 floats).  reward[m]: what agent m receives.  Returns done (the state is then the reset state: new
// goal and key, nothing said).
__device__ __forceinline__ bool mpe_crypto_step_env(const MpeCryptoArgs &a, int n, const float *act, int act_stride, MpeCryptoState &s,
                                                    float *o0, float *o1, float *o2, float (&reward)[MPE_CRYPTO_M]) {
  // ---- action -> state.c (environment.py:245-251: action.c is the action vector; core.py:280-287: state.c = action.c, no noise) ----
#pragma unroll
  for (int m = 0; m < MPE_CRYPTO_M; ++m) {
    const float *am = act + m * act_stride;
    int k;
    if (a.mode == 0) {
      k = 0;
#pragma unroll
      for (int d = 1; d < MPE_CRYPTO_C; ++d)
        if (am[d] > am[k]) k = d;
    } else {
      k = mpe_crypto_clamp((int)am[0], 0, MPE_CRYPTO_C - 1);          // out of range -> the nearest
    }
    s.c[m] = k;
  }
  // ---- rewards: world.collaborative is not set, each agent keeps its own (environment.py:49-50,142) ----
  mpe_crypto_reward(s, reward);
  const int t = s.tstep + 1;
  const bool done = t >= a.T;                                       // environment.py:179-185
  if (done) {                                                       // vec-env wrappers: the returned obs are the reset obs
    s.episode += 1;
    mpe_crypto_reset_env(a, n, s, s.episode);
    s.tstep = 0;
  } else {
    s.tstep = t;
  }
  mpe_crypto_write_obs(o0, o1, o2, s);
  return done;
}

// What the shared kernels need of the scenario, in the one form they take it in.  obs_off / obs_dim: where agent m's observation
// starts in the share row, and its width.  store's flag is `draws` here: the same role as the other scenarios' `landmarks`.
struct MpeCrypto {
  typedef MpeCryptoArgs Args;
  typedef MpeCryptoState State;
  static constexpr int M = MPE_CRYPTO_M, U = MPE_CRYPTO_C, SHARE = MPE_CRYPTO_SHARE;
  __host__ __device__ static constexpr int obs_dim(int m) { return m == 0 ? MPE_CRYPTO_OBS_E : MPE_CRYPTO_OBS_B; }
  __host__ __device__ static constexpr int obs_off(int m) { return m == 0 ? 0 : MPE_CRYPTO_OBS_E + (m - 1) * MPE_CRYPTO_OBS_B; }
  static __device__ __forceinline__ void load(const Args &a, int n, State &s) { mpe_crypto_load(a, n, s); }
  static __device__ __forceinline__ void store(const Args &a, int n, const State &s, bool draws) { mpe_crypto_store(a, n, s, draws); }
  static __device__ __forceinline__ void reset_env(const Args &a, int n, State &s, int64_t ep) { mpe_crypto_reset_env(a, n, s, ep); }
  static __device__ __forceinline__ void write_obs(float *const (&o)[M], const State &s) { mpe_crypto_write_obs(o[0], o[1], o[2], s); }
  static __device__ __forceinline__ bool step_env(const Args &a, int n, const float *act, int act_stride, State &s, float *const (&o)[M],
                                                  float (&reward)[M]) {
    return mpe_crypto_step_env(a, n, act, act_stride, s, o[0], o[1], o[2], reward);
  }
};
