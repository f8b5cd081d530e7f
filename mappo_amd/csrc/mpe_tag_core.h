// mpe_tag_core.h — the MPE `simple_tag` (predator-prey) environment as device functions: reset, one environment step and the
// observation write, one lane per environment, and the traits (MpeTag, at the end) through which the shared kernels reach them: the
// stepwise kernels (mpe_ragged_env.h) and the one-launch rollout episode (rollout_tag.h), so a step computes the same float64 values
// whichever launch runs it.
//
// Reference: onpolicy/envs/mpe/environment.py:194-256 (action decoding, accel in place of the sensitivity), :49-50,142
// (world.collaborative is not set: per-agent rewards), :179-185 (time-limit done); onpolicy/envs/mpe/core.py:207-322 (World.step:
// action force, soft-collision forces between every pair with a movable member, damping, the max_speed clamp, integration);
// onpolicy/envs/mpe/scenarios/simple_tag.py:20-31 (sizes, accel, max_speed), :37-51 (reset), :81-126 (reward), :128-144 (observation);
// and the reset-on-done of the vec-env wrappers (envs/env_wrappers.py:146-152).
//
// Float64 as in the reference's NumPy code, contraction off.  Unlike simple_adversary this step is not only adds, multiplies and
// square roots: the contact force goes through exp and log1p and the boundary penalty through exp, and the device's are not NumPy's,
// so outputs match the fp32 cast of the reference's (tests/golden/mpe_tag.npz) to 1e-6, not to the bit.  State is device resident;
// resets draw from the counter-based Philox stream keyed by (seed, episode, index) — index layout below.
//
// Fixed shape (num_adversaries = 3, num_good_agents = 1, num_landmarks = 2): agents 0..2 are the ADVERSARIES (size 0.075, accel 3,
// max_speed 1), agent 3 is the GOOD agent (size 0.05, accel 4, max_speed 1.3); the landmarks (size 0.2) collide and do not move.
// Every agent moves, Discrete(5); nobody speaks.  Observation of agent m: own velocity, own position, the two landmarks relative to
// it, the three other agents relative to it in world order, and — adversaries only — the good agent's velocity: 16 | 16 | 16 | 14
// features.  The world is NOT collaborative: each agent receives its own reward.
//
// The action force is accel * (accel * u), u = (a1 - a2, a3 - a4): the reference scales u by accel where other scenarios use the
// sensitivity 5 (environment.py:235-238) and multiplies by accel once more when it turns u into a force (core.py:236-237), so an
// adversary is pushed with 9 and the good agent with 16 per unit of u.
//
// Reset draws: Philox stream (seed, episode), mpe_uniform index MPE_TAG_DRAWS * n + k for environment n —
//   k = 2 a, 2 a + 1          position of agent a, U(-1,1)                          (k = 0 .. 7)
//   k = 8 + 2 l, 9 + 2 l      position of landmark l, 0.8 U(-1,1)                   (k = 8 .. 11)
//   k = 12 .. 15              unused
// so no two draws of one (seed, episode) share an index.
#pragma once
#include "mpe_core.h"

#define MPE_TAG_M 4
#define MPE_TAG_L 2
#define MPE_TAG_GOOD 3                                              // the good agent's index; 0 .. 2 are adversaries
#define MPE_TAG_U 5                                                 // every agent's action width (mode 0)
#define MPE_TAG_OBS_A 16                                            // adversary: 4 + 2 L + 2 (M - 1) + 2
#define MPE_TAG_OBS_G 14                                            // good agent: 4 + 2 L + 2 (M - 1)
#define MPE_TAG_SHARE (3 * MPE_TAG_OBS_A + MPE_TAG_OBS_G)           // the four observations side by side, adversaries first: 62
#define MPE_TAG_DRAWS 16

// per-agent physics (simple_tag.py:20-24) and the landmarks' size (:31)
__host__ __device__ constexpr double mpe_tag_size(int m) { return m == MPE_TAG_GOOD ? 0.05 : 0.075; }
__host__ __device__ constexpr double mpe_tag_accel(int m) { return m == MPE_TAG_GOOD ? 4.0 : 3.0; }
__host__ __device__ constexpr double mpe_tag_max_speed(int m) { return m == MPE_TAG_GOOD ? 1.3 : 1.0; }
#define MPE_TAG_LSIZE 0.2

struct MpeTagArgs {
  double *apos, *avel, *lpos;      // agents [N][4][2], [N][4][2]; landmarks [N][2][2]
  int32_t *tstep;                  // [N] steps since the last reset
  int64_t *episode;                // [N] resets so far (Philox counter)
  const float *act;                // mode 0: one-hots / probabilities [N][4][5] | mode 1: indices [N][4]
  float *obs[MPE_TAG_M];           // [N][16] x 3, [N][14]
  float *rewards;                  // [N][4]: one per agent
  uint8_t *dones;                  // [N][4] bool bytes
  int N, T, mode;
  uint64_t seed;
};

// the state one lane holds
struct MpeTagState {
  double p[MPE_TAG_M][2], v[MPE_TAG_M][2], lp[MPE_TAG_L][2];
  int32_t tstep;
  int64_t episode;
};

// scenario.reset_world (simple_tag.py:37-51): agents U(-1,1)^2 at rest, landmarks 0.8 U(-1,1)^2
__device__ __forceinline__ void mpe_tag_reset_env(const MpeTagArgs &a, int n, MpeTagState &s, int64_t ep) {
#pragma clang fp contract(off)   // as in mpe_tag_step_env, which inlines this
  const uint64_t base = (uint64_t)n * MPE_TAG_DRAWS;
#pragma unroll
  for (int m = 0; m < MPE_TAG_M; ++m) {
    s.p[m][0] = mpe_uniform(a.seed, (uint64_t)ep, base + 2 * m);
    s.p[m][1] = mpe_uniform(a.seed, (uint64_t)ep, base + 2 * m + 1);
    s.v[m][0] = s.v[m][1] = 0.0;
  }
#pragma unroll
  for (int l = 0; l < MPE_TAG_L; ++l) {
    s.lp[l][0] = 0.8 * mpe_uniform(a.seed, (uint64_t)ep, base + 2 * MPE_TAG_M + 2 * l);
    s.lp[l][1] = 0.8 * mpe_uniform(a.seed, (uint64_t)ep, base + 2 * MPE_TAG_M + 2 * l + 1);
  }
}

// scenario.observation (simple_tag.py:128-144) of agent m into o: [vel, pos, landmarks - self, the others - self in world-agent
// order, (adversaries:) the good agent's velocity]
__device__ __forceinline__ void mpe_tag_write_obs_agent(float *o, const MpeTagState &s, int m) {
#pragma clang fp contract(off)
  int k = 0;
  o[k++] = (float)s.v[m][0]; o[k++] = (float)s.v[m][1];
  o[k++] = (float)s.p[m][0]; o[k++] = (float)s.p[m][1];
#pragma unroll
  for (int l = 0; l < MPE_TAG_L; ++l) { o[k++] = (float)(s.lp[l][0] - s.p[m][0]); o[k++] = (float)(s.lp[l][1] - s.p[m][1]); }
#pragma unroll
  for (int i = 0; i < MPE_TAG_M; ++i)
    if (i != m) { o[k++] = (float)(s.p[i][0] - s.p[m][0]); o[k++] = (float)(s.p[i][1] - s.p[m][1]); }
  if (m != MPE_TAG_GOOD) { o[k++] = (float)s.v[MPE_TAG_GOOD][0]; o[k++] = (float)s.v[MPE_TAG_GOOD][1]; }
}

__device__ __forceinline__ void mpe_tag_write_obs(float *o0, float *o1, float *o2, float *o3, const MpeTagState &s) {
  mpe_tag_write_obs_agent(o0, s, 0);
  mpe_tag_write_obs_agent(o1, s, 1);
  mpe_tag_write_obs_agent(o2, s, 2);
  mpe_tag_write_obs_agent(o3, s, 3);
}

__device__ __forceinline__ void mpe_tag_load(const MpeTagArgs &a, int n, MpeTagState &s) {
#pragma unroll
  for (int m = 0; m < MPE_TAG_M; ++m)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      s.p[m][d] = a.apos[((size_t)n * MPE_TAG_M + m) * 2 + d];
      s.v[m][d] = a.avel[((size_t)n * MPE_TAG_M + m) * 2 + d];
    }
#pragma unroll
  for (int l = 0; l < MPE_TAG_L; ++l) { s.lp[l][0] = a.lpos[((size_t)n * MPE_TAG_L + l) * 2]; s.lp[l][1] = a.lpos[((size_t)n * MPE_TAG_L + l) * 2 + 1]; }
  s.tstep = a.tstep[n];
  s.episode = a.episode[n];
}

// landmarks: also the landmark positions and the episode counter (they change only at a reset)
__device__ __forceinline__ void mpe_tag_store(const MpeTagArgs &a, int n, const MpeTagState &s, bool landmarks) {
#pragma unroll
  for (int m = 0; m < MPE_TAG_M; ++m)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      a.apos[((size_t)n * MPE_TAG_M + m) * 2 + d] = s.p[m][d];
      a.avel[((size_t)n * MPE_TAG_M + m) * 2 + d] = s.v[m][d];
    }
  a.tstep[n] = s.tstep;
  if (landmarks) {
#pragma unroll
    for (int l = 0; l < MPE_TAG_L; ++l) { a.lpos[((size_t)n * MPE_TAG_L + l) * 2] = s.lp[l][0]; a.lpos[((size_t)n * MPE_TAG_L + l) * 2 + 1] = s.lp[l][1]; }
    a.episode[n] = s.episode;
  }
}

// core.py:289-322 for one pair: the soft-collision force on the first entity (the second receives its negative: both masses are 1)
// from delta = p_first - p_second and dist_min = the two sizes added.  contact_margin 1e-3, contact_force 1e2.
__device__ __forceinline__ void mpe_tag_contact(double dx, double dy, double dist_min, double &fx, double &fy) {
#pragma clang fp contract(off)
  const double dist = sqrt(dx * dx + dy * dy);
  const double k = 1e-3, x = -(dist - dist_min) / k;
  const double pen = (x > 0.0 ? x + log1p(exp(-x)) : log1p(exp(x))) * k;   // np.logaddexp(0, x) * k
  fx = 1e2 * dx / dist * pen; fy = 1e2 * dy / dist * pen;
}

// simple_tag.py:100-105: what leaving the arena costs the good agent, per coordinate, x = |coordinate|
__device__ __forceinline__ double mpe_tag_bound(double x) {
#pragma clang fp contract(off)
  if (x < 0.9) return 0.0;
  if (x < 1.0) return (x - 0.9) * 10.0;
  const double e = exp(2.0 * x - 2.0);
  return e < 10.0 ? e : 10.0;
}

// One step of environment n on the state the lane holds: the four actions -> forces, collision forces, integration with the speed
// clamp, per-agent rewards, time-limit done, reset-on-done, observations.  act: the environment's own actions (a.mode 0: [4][5] floats
// | 1: [4] indices, stride act_stride floats between the agents); o0 .. o3: its four observation rows (16, 16, 16 and 14 floats).
// reward[m]: what agent m receives.  Returns done (the state is then the reset state: new positions and landmarks).
__device__ __forceinline__ bool mpe_tag_step_env(const MpeTagArgs &a, int n, const float *act, int act_stride, MpeTagState &s, float *o0,
                                                 float *o1, float *o2, float *o3, float (&reward)[MPE_TAG_M]) {
  // contraction pinned off for the reason given in mpe_step_env: the body is inlined into more than one kernel, and they must agree
  // to the bit
#pragma clang fp contract(off)
  double f[MPE_TAG_M][2];
  // ---- action -> force (environment.py:194-256: u = [a1 - a2, a3 - a4] * accel; core.py:229-238: force = (mass * accel) * u, mass 1,
  // no noise) ----
#pragma unroll
  for (int m = 0; m < MPE_TAG_M; ++m) {
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
    const double acc = mpe_tag_accel(m);
    f[m][0] = acc * (u0 * acc); f[m][1] = acc * (u1 * acc);
  }
  // ---- soft-collision forces (core.py:241-263,289-322): entity pairs a < b in world order, agents 0 .. 3 then landmarks 4, 5; f_a is
  // added to the force on a, then f_b to the force on b; two landmarks do not act on each other (neither moves).  The 14 pairs are
  // walked by a ROLLED loop over the uniform (a, b), entities and forces picked by selects: unrolled, the pairs' float64 exp / log1p
  // are scheduled side by side and the step holds 212 registers, more than a rollout wave has beside its networks.  Same operations
  // in the same order either way ----
  {
    int pa = 0, pb = 1;
#pragma nounroll
    for (int pair = 0; pair < 14; ++pair) {
      double ax = s.p[0][0], ay = s.p[0][1], bx = s.lp[1][0], by = s.lp[1][1];
#pragma unroll
      for (int m = 1; m < MPE_TAG_M; ++m) { ax = pa == m ? s.p[m][0] : ax; ay = pa == m ? s.p[m][1] : ay; }
#pragma unroll
      for (int m = 1; m < MPE_TAG_M; ++m) { bx = pb == m ? s.p[m][0] : bx; by = pb == m ? s.p[m][1] : by; }
      bx = pb == MPE_TAG_M ? s.lp[0][0] : bx; by = pb == MPE_TAG_M ? s.lp[0][1] : by;
      const double sa = pa == MPE_TAG_GOOD ? mpe_tag_size(MPE_TAG_GOOD) : mpe_tag_size(0);
      const double sb = pb < MPE_TAG_GOOD ? mpe_tag_size(0) : (pb == MPE_TAG_GOOD ? mpe_tag_size(MPE_TAG_GOOD) : MPE_TAG_LSIZE);
      double fx, fy;
      mpe_tag_contact(ax - bx, ay - by, sa + sb, fx, fy);
#pragma unroll
      for (int m = 0; m < MPE_TAG_M; ++m) {
        const double gx = pa == m ? fx : -fx, gy = pa == m ? fy : -fy;     // f_a = force, f_b = -force
        const bool hit = pa == m || pb == m;
        f[m][0] = hit ? gx + f[m][0] : f[m][0]; f[m][1] = hit ? gy + f[m][1] : f[m][1];
      }
      if (++pb == MPE_TAG_M + MPE_TAG_L) { ++pa; pb = pa + 1; }
    }
  }
  // ---- integrate (core.py:265-278: damping 0.25, the max_speed clamp, dt 0.1) ----
#pragma unroll
  for (int m = 0; m < MPE_TAG_M; ++m) {
    double vx = s.v[m][0] * (1.0 - 0.25), vy = s.v[m][1] * (1.0 - 0.25);
    vx += f[m][0] * 0.1; vy += f[m][1] * 0.1;
    const double speed = sqrt(vx * vx + vy * vy);
    if (speed > mpe_tag_max_speed(m)) { vx = vx / speed * mpe_tag_max_speed(m); vy = vy / speed * mpe_tag_max_speed(m); }
    s.v[m][0] = vx; s.v[m][1] = vy;
    s.p[m][0] += vx * 0.1; s.p[m][1] += vy * 0.1;
  }
  // ---- rewards (simple_tag.py:81-126, unshaped): every adversary +10 per adversary in contact with the good agent; the good agent
  // -10 per such contact, minus the boundary penalty of |x| and of |y|.  world.collaborative is not set: each agent keeps its own
  // (environment.py:49-50,142) ----
  double caught = 0.0;
#pragma unroll
  for (int m = 0; m < MPE_TAG_GOOD; ++m) {
    const double dx = s.p[MPE_TAG_GOOD][0] - s.p[m][0], dy = s.p[MPE_TAG_GOOD][1] - s.p[m][1];
    if (sqrt(dx * dx + dy * dy) < mpe_tag_size(MPE_TAG_GOOD) + mpe_tag_size(m)) caught += 10.0;
  }
  double good = 0.0 - caught;
  good -= mpe_tag_bound(fabs(s.p[MPE_TAG_GOOD][0]));
  good -= mpe_tag_bound(fabs(s.p[MPE_TAG_GOOD][1]));
  reward[0] = reward[1] = reward[2] = (float)caught;
  reward[MPE_TAG_GOOD] = (float)good;
  const int t = s.tstep + 1;
  const bool done = t >= a.T;                                       // environment.py:179-185
  if (done) {                                                       // vec-env wrappers: the returned obs are the reset obs
    s.episode += 1;
    mpe_tag_reset_env(a, n, s, s.episode);
    s.tstep = 0;
  } else {
    s.tstep = t;
  }
  mpe_tag_write_obs(o0, o1, o2, o3, s);
  return done;
}

// What the shared kernels need of the scenario, in the one form they take it in.  obs_off / obs_dim: where agent m's observation
// starts in the share row, and its width.
struct MpeTag {
  typedef MpeTagArgs Args;
  typedef MpeTagState State;
  static constexpr int M = MPE_TAG_M, U = MPE_TAG_U, SHARE = MPE_TAG_SHARE;
  __host__ __device__ static constexpr int obs_dim(int m) { return m == MPE_TAG_GOOD ? MPE_TAG_OBS_G : MPE_TAG_OBS_A; }
  __host__ __device__ static constexpr int obs_off(int m) { return m * MPE_TAG_OBS_A; }
  static __device__ __forceinline__ void load(const Args &a, int n, State &s) { mpe_tag_load(a, n, s); }
  static __device__ __forceinline__ void store(const Args &a, int n, const State &s, bool landmarks) { mpe_tag_store(a, n, s, landmarks); }
  static __device__ __forceinline__ void reset_env(const Args &a, int n, State &s, int64_t ep) { mpe_tag_reset_env(a, n, s, ep); }
  static __device__ __forceinline__ void write_obs(float *const (&o)[M], const State &s) { mpe_tag_write_obs(o[0], o[1], o[2], o[3], s); }
  static __device__ __forceinline__ bool step_env(const Args &a, int n, const float *act, int act_stride, State &s, float *const (&o)[M],
                                                  float (&reward)[M]) {
    return mpe_tag_step_env(a, n, act, act_stride, s, o[0], o[1], o[2], o[3], reward);
  }
};
