// mpe_push_core.h — the MPE `simple_push` ("keep-away") environment as device functions: reset, one environment step and the
// observation write, one lane per environment, and the traits (MpePush, at the end) through which the shared kernels reach them: the
// stepwise kernels (mpe_ragged_env.h) and the one-launch rollout episode (rollout_push.h), so a step computes the same float64 values
// whichever launch runs it.
//
// Reference: onpolicy/envs/mpe/environment.py:194-256 (action decoding), :49-50,142 (world.collaborative is not set: per-agent
// rewards), :179-185 (time-limit done); onpolicy/envs/mpe/core.py:207-322 (World.step: action force, the soft-collision force
// between the two agents, damping, integration; no max_speed); onpolicy/envs/mpe/scenarios/simple_push.py:12-40 (both agents collide,
// the landmarks do not), :42-65 (reset), :67-84 (reward), :86-107 (observation); and the reset-on-done of the vec-env wrappers
// (envs/env_wrappers.py:146-152).
//
// Float64 as in the reference's NumPy code, contraction off.  Beside adds, multiplies and correctly rounded square roots the
// contact force goes through exp and log1p, and the device's are not NumPy's, so outputs match the fp32 cast of the reference's
// (tests/golden/mpe_push.npz) to 1e-6, not by construction to the bit.  State is device resident; resets draw from the
// counter-based Philox stream keyed by (seed, episode, index) — index layout below.
//
// Fixed shape (num_agents = 2, num_landmarks = 2): agent 0 is the ADVERSARY (own velocity, the two landmarks and the other agent
// relative to itself: 8 features; it is not told which landmark is the goal), agent 1 is the GOOD agent (own velocity, the goal
// relative to itself, its own colour — which names the goal —, the two landmarks relative to itself, the landmarks' colours and
// the other agent relative to itself: 19 features).  Both move, Discrete(5); nobody speaks.  The two agents collide with each
// other (size 0.05 each) and with nothing else: the landmarks neither move nor collide.  accel and max_speed are not set, so the
// action force is the sensitivity 5 per unit of u and there is no speed clamp.  The world is NOT collaborative: each agent receives
// its own reward.
//
// Reset draws: Philox stream (seed, episode), mpe_uniform index MPE_PUSH_DRAWS * n + k for environment n —
//   k = 2 a, 2 a + 1          position of agent a, U(-1,1)                          (k = 0 .. 3)
//   k = 4 + 2 l, 5 + 2 l      position of landmark l, 0.8 U(-1,1)                   (k = 4 .. 7)
//   k = 8                     goal landmark: min(1, floor(2 u)), u = (draw + 1) / 2 in [0, 1)
//   k = 9 .. 15               unused
// so no two draws of one (seed, episode) share an index.
#pragma once
#include "mpe_tag_core.h"                                            // mpe_tag_contact: the soft-collision force of core.py:289-322

#define MPE_PUSH_M 2
#define MPE_PUSH_L 2
#define MPE_PUSH_GOOD 1                                             // the good agent's index; 0 is the adversary
#define MPE_PUSH_U 5                                                // every agent's action width (mode 0)
#define MPE_PUSH_OBS_A 8                                            // adversary: 2 + 2 L + 2 (M - 1)
#define MPE_PUSH_OBS_G 19                                           // good agent: 2 + 2 + 3 + 2 L + 3 L + 2 (M - 1)
#define MPE_PUSH_SHARE (MPE_PUSH_OBS_A + MPE_PUSH_OBS_G)            // the two observations side by side, adversary first: 27
#define MPE_PUSH_DRAWS 16
#define MPE_PUSH_SIZE 0.05                                          // both agents (core.py: the default entity size)

struct MpePushArgs {
  double *apos, *avel, *lpos;      // agents [N][2][2], [N][2][2]; landmarks [N][2][2]
  int32_t *goal;                   // [N] landmark index of both agents' goal_a
  int32_t *tstep;                  // [N] steps since the last reset
  int64_t *episode;                // [N] resets so far (Philox counter)
  const float *act;                // mode 0: one-hots / probabilities [N][2][5] | mode 1: indices [N][2]
  float *obs[MPE_PUSH_M];          // [N][8], [N][19]
  float *rewards;                  // [N][2]: one per agent
  uint8_t *dones;                  // [N][2] bool bytes
  int N, T, mode;
  uint64_t seed;
};

// the state one lane holds
struct MpePushState {
  double p[MPE_PUSH_M][2], v[MPE_PUSH_M][2], lp[MPE_PUSH_L][2];
  int g;
  int32_t tstep;
  int64_t episode;
};

// scenario.reset_world (simple_push.py:42-65): the goal uniform over the landmarks, agents U(-1,1)^2 at rest, landmarks
// 0.8 U(-1,1)^2
__device__ __forceinline__ void mpe_push_reset_env(const MpePushArgs &a, int n, MpePushState &s, int64_t ep) {
#pragma clang fp contract(off)   // as in mpe_push_step_env, which inlines this
  const uint64_t base = (uint64_t)n * MPE_PUSH_DRAWS;
#pragma unroll
  for (int m = 0; m < MPE_PUSH_M; ++m) {
    s.p[m][0] = mpe_uniform(a.seed, (uint64_t)ep, base + 2 * m);
    s.p[m][1] = mpe_uniform(a.seed, (uint64_t)ep, base + 2 * m + 1);
    s.v[m][0] = s.v[m][1] = 0.0;
  }
#pragma unroll
  for (int l = 0; l < MPE_PUSH_L; ++l) {
    s.lp[l][0] = 0.8 * mpe_uniform(a.seed, (uint64_t)ep, base + 2 * MPE_PUSH_M + 2 * l);
    s.lp[l][1] = 0.8 * mpe_uniform(a.seed, (uint64_t)ep, base + 2 * MPE_PUSH_M + 2 * l + 1);
  }
  const double u = (mpe_uniform(a.seed, (uint64_t)ep, base + 8) + 1.0) * 0.5;
  const int k = (int)floor(2.0 * u);
  s.g = k < 0 ? 0 : (k > 1 ? 1 : k);
}

// scenario.observation (simple_push.py:86-107).  oa, the adversary: [vel, landmarks - self, other - self].  og, the good agent:
// [vel, goal - self, own colour, landmarks - self, landmark colours, other - self].  The colours are the reference's float64 sums
// (landmark k: 0.1 everywhere, [k + 1] += 0.8; good agent: 0.25 everywhere, [goal + 1] += 0.5), cast to fp32 afterwards.
__device__ __forceinline__ void mpe_push_write_obs(float *oa, float *og, const MpePushState &s) {
#pragma clang fp contract(off)
  constexpr double lc_base = 0.1, lc_on = 0.1 + 0.8, gc_base = 0.25, gc_on = 0.25 + 0.5;
  const double gx = s.g == 0 ? s.lp[0][0] : s.lp[1][0], gy = s.g == 0 ? s.lp[0][1] : s.lp[1][1];
  int k = 0;
  oa[k++] = (float)s.v[0][0]; oa[k++] = (float)s.v[0][1];
#pragma unroll
  for (int l = 0; l < MPE_PUSH_L; ++l) { oa[k++] = (float)(s.lp[l][0] - s.p[0][0]); oa[k++] = (float)(s.lp[l][1] - s.p[0][1]); }
  oa[k++] = (float)(s.p[1][0] - s.p[0][0]); oa[k++] = (float)(s.p[1][1] - s.p[0][1]);
  k = 0;
  og[k++] = (float)s.v[1][0]; og[k++] = (float)s.v[1][1];
  og[k++] = (float)(gx - s.p[1][0]); og[k++] = (float)(gy - s.p[1][1]);
  og[k++] = (float)gc_base; og[k++] = (float)(s.g == 0 ? gc_on : gc_base); og[k++] = (float)(s.g == 1 ? gc_on : gc_base);
#pragma unroll
  for (int l = 0; l < MPE_PUSH_L; ++l) { og[k++] = (float)(s.lp[l][0] - s.p[1][0]); og[k++] = (float)(s.lp[l][1] - s.p[1][1]); }
#pragma unroll
  for (int l = 0; l < MPE_PUSH_L; ++l) {
    og[k++] = (float)lc_base; og[k++] = (float)(l == 0 ? lc_on : lc_base); og[k++] = (float)(l == 1 ? lc_on : lc_base);
  }
  og[k++] = (float)(s.p[0][0] - s.p[1][0]); og[k++] = (float)(s.p[0][1] - s.p[1][1]);
}

__device__ __forceinline__ void mpe_push_load(const MpePushArgs &a, int n, MpePushState &s) {
#pragma unroll
  for (int m = 0; m < MPE_PUSH_M; ++m)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      s.p[m][d] = a.apos[((size_t)n * MPE_PUSH_M + m) * 2 + d];
      s.v[m][d] = a.avel[((size_t)n * MPE_PUSH_M + m) * 2 + d];
    }
#pragma unroll
  for (int l = 0; l < MPE_PUSH_L; ++l) { s.lp[l][0] = a.lpos[((size_t)n * MPE_PUSH_L + l) * 2]; s.lp[l][1] = a.lpos[((size_t)n * MPE_PUSH_L + l) * 2 + 1]; }
  const int k = a.goal[n];
  s.g = k < 0 ? 0 : (k > 1 ? 1 : k);
  s.tstep = a.tstep[n];
  s.episode = a.episode[n];
}

// landmarks: also the landmark positions, the goal and the episode counter (they change only at a reset)
__device__ __forceinline__ void mpe_push_store(const MpePushArgs &a, int n, const MpePushState &s, bool landmarks) {
#pragma unroll
  for (int m = 0; m < MPE_PUSH_M; ++m)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      a.apos[((size_t)n * MPE_PUSH_M + m) * 2 + d] = s.p[m][d];
      a.avel[((size_t)n * MPE_PUSH_M + m) * 2 + d] = s.v[m][d];
    }
  a.tstep[n] = s.tstep;
  if (landmarks) {
#pragma unroll
    for (int l = 0; l < MPE_PUSH_L; ++l) { a.lpos[((size_t)n * MPE_PUSH_L + l) * 2] = s.lp[l][0]; a.lpos[((size_t)n * MPE_PUSH_L + l) * 2 + 1] = s.lp[l][1]; }
    a.goal[n] = s.g;
    a.episode[n] = s.episode;
  }
}

// scenario.reward (simple_push.py:67-84): the good agent -|p_good - goal|; the adversary |p_good - goal| (the min over the one good
// agent) - |goal - p_adv|.  world.collaborative is not set: each agent keeps its own (environment.py:49-50,142)
__device__ __forceinline__ void mpe_push_reward(const MpePushState &s, float (&reward)[MPE_PUSH_M]) {
#pragma clang fp contract(off)
  const double gx = s.g == 0 ? s.lp[0][0] : s.lp[1][0], gy = s.g == 0 ? s.lp[0][1] : s.lp[1][1];
  const double dgx = s.p[1][0] - gx, dgy = s.p[1][1] - gy, dax = gx - s.p[0][0], day = gy - s.p[0][1];
  const double d_good = sqrt(dgx * dgx + dgy * dgy), d_adv = sqrt(dax * dax + day * day);
  reward[0] = (float)(d_good - d_adv);
  reward[MPE_PUSH_GOOD] = (float)(-d_good);
}

// One step of environment n on the state the lane holds: the two actions -> forces, the contact force between the two agents,
// integration, per-agent rewards, time-limit done, reset-on-done, observations.  act: the environment's own actions (a.mode 0:
// [2][5] floats | 1: [2] indices, stride act_stride floats between the agents); oa / og: its two observation rows (8 and 19
// floats).  reward[m]: what agent m receives.  Returns done (the state is then the reset state: new positions, landmarks and goal).
__device__ __forceinline__ bool mpe_push_step_env(const MpePushArgs &a, int n, const float *act, int act_stride, MpePushState &s, float *oa,
                                                  float *og, float (&reward)[MPE_PUSH_M]) {
  // contraction pinned off for the reason given in mpe_step_env: the body is inlined into more than one kernel, and they must agree
  // to the bit
#pragma clang fp contract(off)
  double f[MPE_PUSH_M][2];
  // ---- action -> force (environment.py:194-256: u = [a1 - a2, a3 - a4] * sensitivity 5, accel is None; core.py:229-238: mass 1, no
  // noise) ----
#pragma unroll
  for (int m = 0; m < MPE_PUSH_M; ++m) {
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
    f[m][0] = 5.0 * u0; f[m][1] = 5.0 * u1;
  }
  // ---- soft-collision force (core.py:241-263,289-322): the one pair with two colliders, entity a = agent 0, entity b = agent 1; f_a
  // = force is added to the force on agent 0, f_b = -force to the force on agent 1 (both masses are 1) ----
  {
    double fx, fy;
    mpe_tag_contact(s.p[0][0] - s.p[1][0], s.p[0][1] - s.p[1][1], MPE_PUSH_SIZE + MPE_PUSH_SIZE, fx, fy);
    f[0][0] = fx + f[0][0]; f[0][1] = fy + f[0][1];
    f[1][0] = -fx + f[1][0]; f[1][1] = -fy + f[1][1];
  }
  // ---- integrate (core.py:265-278: damping 0.25, dt 0.1, no max_speed) ----
#pragma unroll
  for (int m = 0; m < MPE_PUSH_M; ++m) {
    s.v[m][0] = s.v[m][0] * (1.0 - 0.25); s.v[m][1] = s.v[m][1] * (1.0 - 0.25);
    s.v[m][0] += f[m][0] * 0.1; s.v[m][1] += f[m][1] * 0.1;
    s.p[m][0] += s.v[m][0] * 0.1; s.p[m][1] += s.v[m][1] * 0.1;
  }
  mpe_push_reward(s, reward);
  const int t = s.tstep + 1;
  const bool done = t >= a.T;                                       // environment.py:179-185
  if (done) {                                                       // vec-env wrappers: the returned obs are the reset obs
    s.episode += 1;
    mpe_push_reset_env(a, n, s, s.episode);
    s.tstep = 0;
  } else {
    s.tstep = t;
  }
  mpe_push_write_obs(oa, og, s);
  return done;
}

// What the shared kernels need of the scenario, in the one form they take it in.  obs_off / obs_dim: where agent m's observation
// starts in the share row, and its width.
struct MpePush {
  typedef MpePushArgs Args;
  typedef MpePushState State;
  static constexpr int M = MPE_PUSH_M, U = MPE_PUSH_U, SHARE = MPE_PUSH_SHARE;
  __host__ __device__ static constexpr int obs_dim(int m) { return m == 0 ? MPE_PUSH_OBS_A : MPE_PUSH_OBS_G; }
  __host__ __device__ static constexpr int obs_off(int m) { return m == 0 ? 0 : MPE_PUSH_OBS_A; }
  static __device__ __forceinline__ void load(const Args &a, int n, State &s) { mpe_push_load(a, n, s); }
  static __device__ __forceinline__ void store(const Args &a, int n, const State &s, bool landmarks) { mpe_push_store(a, n, s, landmarks); }
  static __device__ __forceinline__ void reset_env(const Args &a, int n, State &s, int64_t ep) { mpe_push_reset_env(a, n, s, ep); }
  static __device__ __forceinline__ void write_obs(float *const (&o)[M], const State &s) { mpe_push_write_obs(o[0], o[1], s); }
  static __device__ __forceinline__ bool step_env(const Args &a, int n, const float *act, int act_stride, State &s, float *const (&o)[M],
                                                  float (&reward)[M]) {
    return mpe_push_step_env(a, n, act, act_stride, s, o[0], o[1], reward);
  }
};
