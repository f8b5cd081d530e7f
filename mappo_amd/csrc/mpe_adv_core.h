// mpe_adv_core.h — the MPE `simple_adversary` ("physical deception") environment as device functions: reset, one environment step
// and the observation write, one lane per environment, and the traits (MpeAdv, at the end) through which the shared kernels reach
// them: the stepwise kernels (mpe_ragged_env.h) and the one-launch rollout episode (rollout_sep_img.h), so a step computes the same
// float64 values whichever launch runs it.
//
// Reference: onpolicy/envs/mpe/environment.py:194-256 (action decoding), :49-50,142 (world.collaborative is not set: per-agent
// rewards), :179-185 (time-limit done); onpolicy/envs/mpe/core.py:207-287 (World.step: action force, damping + integration; nothing
// collides); onpolicy/envs/mpe/scenarios/simple_adversary.py:36-53 (reset), :74-116 (reward), :119-137 (observation); and the
// reset-on-done of the vec-env wrappers (envs/env_wrappers.py:146-152).
//
// Float64 as in the reference's NumPy code; the only function beyond add and multiply is a correctly rounded sqrt, and with
// contraction off the outputs EQUAL the fp32 cast of the reference's (tests/golden/mpe_adversary.npz).  State is device resident;
// resets draw from the counter-based Philox stream keyed by (seed, episode, index) — index layout below.
//
// Fixed shape (num_agents = 3: one adversary, num_agents - 1 good agents and as many landmarks): agent 0 is the ADVERSARY (observes
// the two landmarks and the two others relative to itself: 8 features; it is not told which landmark is the goal), agents 1 and 2
// are the GOOD agents (the goal landmark relative to themselves, then the same 8: 10 features).  Every agent moves, Discrete(5);
// nobody speaks and nothing collides.  The world is NOT collaborative: each agent receives its own reward.
//
// Reset draws: Philox stream (seed, episode), mpe_uniform index MPE_ADV_DRAWS * n + k for environment n —
//   k = 2 a, 2 a + 1          position of agent a, U(-1,1)
//   k = 6 + 2 l, 7 + 2 l      position of landmark l, U(-1,1)
//   k = 10                    goal landmark: min(1, floor(2 u)), u = (draw + 1) / 2 in [0, 1)
//   k = 11 .. 15              unused
// so no two draws of one (seed, episode) share an index.
#pragma once
#include "mpe_core.h"

#define MPE_ADV_M 3
#define MPE_ADV_L 2
#define MPE_ADV_U 5                                                 // every agent's action width (mode 0)
#define MPE_ADV_OBS_A 8                                             // adversary: 2 L + 2 (M - 1)
#define MPE_ADV_OBS_G 10                                            // good agent: 2 + 2 L + 2 (M - 1)
#define MPE_ADV_SHARE (MPE_ADV_OBS_A + 2 * MPE_ADV_OBS_G)           // the three observations side by side, adversary first
#define MPE_ADV_DRAWS 16

struct MpeAdvArgs {
  double *apos, *avel, *lpos;      // agents [N][3][2], [N][3][2]; landmarks [N][2][2]
  int32_t *goal;                   // [N] landmark index of every agent's goal_a
  int32_t *tstep;                  // [N] steps since the last reset
  int64_t *episode;                // [N] resets so far (Philox counter)
  const float *act;                // mode 0: one-hots / probabilities [N][3][5] | mode 1: indices [N][3]
  float *obs[MPE_ADV_M];           // [N][8], [N][10], [N][10]
  float *rewards;                  // [N][3]: one per agent
  uint8_t *dones;                  // [N][3] bool bytes
  int N, T, mode;
  uint64_t seed;
};

// the state one lane holds
struct MpeAdvState {
  double p[MPE_ADV_M][2], v[MPE_ADV_M][2], lp[MPE_ADV_L][2];
  int g;
  int32_t tstep;
  int64_t episode;
};

// scenario.reset_world (simple_adversary.py:36-53): the goal uniform over the landmarks, agents and landmarks U(-1,1)^2, at rest
__device__ __forceinline__ void mpe_adv_reset_env(const MpeAdvArgs &a, int n, MpeAdvState &s, int64_t ep) {
#pragma clang fp contract(off)   // as in mpe_adv_step_env, which inlines this
  const uint64_t base = (uint64_t)n * MPE_ADV_DRAWS;
#pragma unroll
  for (int m = 0; m < MPE_ADV_M; ++m) {
    s.p[m][0] = mpe_uniform(a.seed, (uint64_t)ep, base + 2 * m);
    s.p[m][1] = mpe_uniform(a.seed, (uint64_t)ep, base + 2 * m + 1);
    s.v[m][0] = s.v[m][1] = 0.0;
  }
#pragma unroll
  for (int l = 0; l < MPE_ADV_L; ++l) {
    s.lp[l][0] = mpe_uniform(a.seed, (uint64_t)ep, base + 6 + 2 * l);
    s.lp[l][1] = mpe_uniform(a.seed, (uint64_t)ep, base + 7 + 2 * l);
  }
  const double u = (mpe_uniform(a.seed, (uint64_t)ep, base + 10) + 1.0) * 0.5;
  const int k = (int)floor(2.0 * u);
  s.g = k < 0 ? 0 : (k > 1 ? 1 : k);
}

// scenario.observation (simple_adversary.py:119-137) of agent m into o: [goal - self (good agents only), landmarks - self, the
// others - self in world-agent order]
__device__ __forceinline__ void mpe_adv_write_obs_agent(float *o, const MpeAdvState &s, int m) {
#pragma clang fp contract(off)
  int k = 0;
  if (m != 0) {
    o[k++] = (float)((s.g == 0 ? s.lp[0][0] : s.lp[1][0]) - s.p[m][0]);
    o[k++] = (float)((s.g == 0 ? s.lp[0][1] : s.lp[1][1]) - s.p[m][1]);
  }
#pragma unroll
  for (int l = 0; l < MPE_ADV_L; ++l) { o[k++] = (float)(s.lp[l][0] - s.p[m][0]); o[k++] = (float)(s.lp[l][1] - s.p[m][1]); }
#pragma unroll
  for (int i = 0; i < MPE_ADV_M; ++i)
    if (i != m) { o[k++] = (float)(s.p[i][0] - s.p[m][0]); o[k++] = (float)(s.p[i][1] - s.p[m][1]); }
}

__device__ __forceinline__ void mpe_adv_write_obs(float *o0, float *o1, float *o2, const MpeAdvState &s) {
  mpe_adv_write_obs_agent(o0, s, 0);
  mpe_adv_write_obs_agent(o1, s, 1);
  mpe_adv_write_obs_agent(o2, s, 2);
}

__device__ __forceinline__ void mpe_adv_load(const MpeAdvArgs &a, int n, MpeAdvState &s) {
#pragma unroll
  for (int m = 0; m < MPE_ADV_M; ++m)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      s.p[m][d] = a.apos[((size_t)n * MPE_ADV_M + m) * 2 + d];
      s.v[m][d] = a.avel[((size_t)n * MPE_ADV_M + m) * 2 + d];
    }
#pragma unroll
  for (int l = 0; l < MPE_ADV_L; ++l) { s.lp[l][0] = a.lpos[((size_t)n * MPE_ADV_L + l) * 2]; s.lp[l][1] = a.lpos[((size_t)n * MPE_ADV_L + l) * 2 + 1]; }
  const int k = a.goal[n];
  s.g = k < 0 ? 0 : (k > 1 ? 1 : k);
  s.tstep = a.tstep[n];
  s.episode = a.episode[n];
}

// landmarks: also the landmark positions, the goal and the episode counter (they change only at a reset)
__device__ __forceinline__ void mpe_adv_store(const MpeAdvArgs &a, int n, const MpeAdvState &s, bool landmarks) {
#pragma unroll
  for (int m = 0; m < MPE_ADV_M; ++m)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      a.apos[((size_t)n * MPE_ADV_M + m) * 2 + d] = s.p[m][d];
      a.avel[((size_t)n * MPE_ADV_M + m) * 2 + d] = s.v[m][d];
    }
  a.tstep[n] = s.tstep;
  if (landmarks) {
#pragma unroll
    for (int l = 0; l < MPE_ADV_L; ++l) { a.lpos[((size_t)n * MPE_ADV_L + l) * 2] = s.lp[l][0]; a.lpos[((size_t)n * MPE_ADV_L + l) * 2 + 1] = s.lp[l][1]; }
    a.goal[n] = s.g;
    a.episode[n] = s.episode;
  }
}

// One step of environment n on the state the lane holds: the three actions -> forces, integration, per-agent rewards, time-limit
// done, reset-on-done, observations.  act: the environment's own actions (a.mode 0: [3][5] floats | 1: [3] indices, stride
// act_stride floats between the agents); o0 / o1 / o2: its three observation rows (8, 10 and 10 floats).  reward[m]: what agent m
// receives.  Returns done (the state is then the reset state: new positions, landmarks and goal).
__device__ __forceinline__ bool mpe_adv_step_env(const MpeAdvArgs &a, int n, const float *act, int act_stride, MpeAdvState &s, float *o0,
                                                 float *o1, float *o2, float (&reward)[MPE_ADV_M]) {
  // contraction pinned off for the reason given in mpe_step_env: the body is inlined into two kernels that must agree to the bit,
  // and here every value is also held EQUAL to the reference's float64 (sqrt is correctly rounded; nothing else is transcendental)
#pragma clang fp contract(off)
  // ---- action -> force (environment.py:194-256: u = [a1 - a2, a3 - a4] * sensitivity 5, accel is None; core.py:229-238: mass 1, no
  // noise; nothing collides) and integrate (core.py:265-278: damping 0.25, dt 0.1, no max_speed) ----
#pragma unroll
  for (int m = 0; m < MPE_ADV_M; ++m) {
    const float *am = act + m * act_stride;
    double u0, u1;
    if (a.mode == 0) {
      u0 = (double)am[1] - (double)am[2]; u1 = (double)am[3] - (double)am[4];
    } else {
      int k = (int)am[0];
      k = k < 0 ? 0 : (k > 4 ? 4 : k);                              // out of range -> the nearest
      u0 = k == 1 ? 1.0 : (k == 2 ? -1.0 : 0.0);                    // the one-hot of index k through the line above
      u1 = k == 3 ? 1.0 : (k == 4 ? -1.0 : 0.0);
    }
    const double f0 = 5.0 * u0, f1 = 5.0 * u1;
    s.v[m][0] = s.v[m][0] * (1.0 - 0.25); s.v[m][1] = s.v[m][1] * (1.0 - 0.25);
    s.v[m][0] += f0 * 0.1; s.v[m][1] += f1 * 0.1;
    s.p[m][0] += s.v[m][0] * 0.1; s.p[m][1] += s.v[m][1] * 0.1;
  }
  // ---- rewards (simple_adversary.py:74-116, shaped): adversary -|p - goal|^2; a good agent -min over the good agents of |p - goal|
  // + |adversary - goal|.  world.collaborative is not set: each agent keeps its own (environment.py:49-50,142) ----
  const double gx = s.g == 0 ? s.lp[0][0] : s.lp[1][0], gy = s.g == 0 ? s.lp[0][1] : s.lp[1][1];
  double sq[MPE_ADV_M];
#pragma unroll
  for (int m = 0; m < MPE_ADV_M; ++m) { const double dx = s.p[m][0] - gx, dy = s.p[m][1] - gy; sq[m] = dx * dx + dy * dy; }
  const double d_adv = sqrt(sq[0]), d1 = sqrt(sq[1]), d2 = sqrt(sq[2]);
  const double good = -(d2 < d1 ? d2 : d1) + (0.0 + d_adv);          // pos_rew + adv_rew, adv_rew = sum([d_adv])
  reward[0] = (float)(-sq[0]);
  reward[1] = (float)good;
  reward[2] = (float)good;
  const int t = s.tstep + 1;
  const bool done = t >= a.T;                                       // environment.py:179-185
  if (done) {                                                       // vec-env wrappers: the returned obs are the reset obs
    s.episode += 1;
    mpe_adv_reset_env(a, n, s, s.episode);
    s.tstep = 0;
  } else {
    s.tstep = t;
  }
  mpe_adv_write_obs(o0, o1, o2, s);
  return done;
}

// What the shared kernels need of the scenario, in the one form they take it in.  obs_off / obs_dim: where agent m's observation
// starts in the share row, and its width.
struct MpeAdv {
  typedef MpeAdvArgs Args;
  typedef MpeAdvState State;
  static constexpr int M = MPE_ADV_M, U = MPE_ADV_U, SHARE = MPE_ADV_SHARE;
  __host__ __device__ static constexpr int obs_dim(int m) { return m == 0 ? MPE_ADV_OBS_A : MPE_ADV_OBS_G; }
  __host__ __device__ static constexpr int obs_off(int m) { return m == 0 ? 0 : MPE_ADV_OBS_A + (m - 1) * MPE_ADV_OBS_G; }
  static __device__ __forceinline__ void load(const Args &a, int n, State &s) { mpe_adv_load(a, n, s); }
  static __device__ __forceinline__ void store(const Args &a, int n, const State &s, bool landmarks) { mpe_adv_store(a, n, s, landmarks); }
  static __device__ __forceinline__ void reset_env(const Args &a, int n, State &s, int64_t ep) { mpe_adv_reset_env(a, n, s, ep); }
  static __device__ __forceinline__ void write_obs(float *const (&o)[M], const State &s) { mpe_adv_write_obs(o[0], o[1], o[2], s); }
  static __device__ __forceinline__ bool step_env(const Args &a, int n, const float *act, int act_stride, State &s, float *const (&o)[M],
                                                  float (&reward)[M]) {
    return mpe_adv_step_env(a, n, act, act_stride, s, o[0], o[1], o[2], reward);
  }
};
