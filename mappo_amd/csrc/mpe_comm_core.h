// mpe_comm_core.h — the MPE `simple_speaker_listener` environment as device functions: reset, one environment step and the
// observation write, one lane per environment.  Shared by the stepwise kernels (mpe_comm_env.hip) and the one-launch rollout
// episode (rollout_comm.h), so a step computes the same float64 values whichever launch runs it.  Reference sites: see
// mpe_comm_env.hip.
//
// Fixed shape (the scenario asserts 2 agents and colours exactly 3 landmarks): agent 0 is the SPEAKER (does not move, observes the
// colour of the goal landmark: 3 features, says one of dim_c = 3 symbols: Discrete(3)), agent 1 the LISTENER (silent, observes its
// velocity, the three landmarks relative to itself and the speaker's symbol: 2 + 6 + 3 = 11 features, moves: Discrete(5)).  The
// speaker's own position and velocity are neither observed nor rewarded, so they are not part of the state.  The channel symbol
// is kept as state (-1: none, after a reset) for whoever inspects the environment; the step that sets it writes it into the
// listener's observation itself.
//
// Reset draws: Philox stream (seed, episode), mpe_uniform index MPE_COMM_DRAWS * n + k for environment n —
//   k = 0, 1      listener position x, y
//   k = 2 .. 7    landmark l position x, y at 2 + 2 l, 3 + 2 l (U(-1,1): this scenario does not shrink the landmarks' range)
//   k = 8         goal landmark: min(2, floor(3 u)), u = (draw + 1) / 2 in [0, 1)
//   k = 9 .. 15   unused
// so no two draws of one (seed, episode) share an index.
#pragma once
#include "mpe_core.h"

#define MPE_COMM_M 2
#define MPE_COMM_L 3
#define MPE_COMM_C 3                                                // dim_c: the speaker's action width (mode 0)
#define MPE_COMM_U 5                                                // the listener's action width (mode 0)
#define MPE_COMM_OBS_S 3                                            // speaker: colour of the goal landmark
#define MPE_COMM_OBS_L 11                                           // listener: 2 + 2 L + dim_c
#define MPE_COMM_SHARE (MPE_COMM_OBS_S + MPE_COMM_OBS_L)            // both observations side by side, speaker first
#define MPE_COMM_DRAWS 16

struct MpeCommArgs {
  double *pos, *vel, *lpos;        // listener [N][2], [N][2]; landmarks [N][3][2]
  int32_t *goal;                   // [N] landmark index of the speaker's goal_b
  int32_t *symbol;                 // [N] the symbol in the channel, -1: none (after a reset)
  int32_t *tstep;                  // [N] steps since the last reset
  int64_t *episode;                // [N] resets so far (Philox counter)
  const float *act_s, *act_l;      // mode 0: one-hots / probabilities [N][3], [N][5] | mode 1: act_s = indices [N][2] (symbol, move), act_l unused
  float *obs_s, *obs_l, *rewards;  // [N][3], [N][11], [N][2]
  uint8_t *dones;                  // [N][2] bool bytes
  int N, T, mode;
  uint64_t seed;
};

// the state one lane holds
struct MpeCommState {
  double p[2], v[2], lp[MPE_COMM_L][2];
  int g, sym;
  int32_t tstep;
  int64_t episode;
};

// scenario.reset_world (simple_speaker_listener.py:38-63): the goal uniform over the landmarks, listener and landmarks U(-1,1)^2,
// at rest, c = 0
__device__ __forceinline__ void mpe_comm_reset_env(const MpeCommArgs &a, int n, MpeCommState &s, int64_t ep) {
#pragma clang fp contract(off)   // as in mpe_comm_step_env, which inlines this
  const uint64_t base = (uint64_t)n * MPE_COMM_DRAWS;
  s.p[0] = mpe_uniform(a.seed, (uint64_t)ep, base);
  s.p[1] = mpe_uniform(a.seed, (uint64_t)ep, base + 1);
  s.v[0] = s.v[1] = 0.0;
#pragma unroll
  for (int l = 0; l < MPE_COMM_L; ++l) {
    s.lp[l][0] = mpe_uniform(a.seed, (uint64_t)ep, base + 2 + 2 * l);
    s.lp[l][1] = mpe_uniform(a.seed, (uint64_t)ep, base + 3 + 2 * l);
  }
  const double u = (mpe_uniform(a.seed, (uint64_t)ep, base + 8) + 1.0) * 0.5;
  const int k = (int)floor(3.0 * u);
  s.g = k < 0 ? 0 : (k > 2 ? 2 : k);
  s.sym = -1;
}

// scenario.observation (simple_speaker_listener.py:75-98).  speaker: the goal landmark's colour ((.65,.15,.15), (.15,.65,.15),
// (.15,.15,.65)); listener: [vel, landmarks - pos, the speaker's c].  as: the speaker's action that set c in this step (mode as in
// MpeCommArgs: 0 = 3 floats taken verbatim, 1 = one index), or null: c = 0 (after a reset)
__device__ __forceinline__ void mpe_comm_write_obs(float *os, float *ol, const MpeCommState &s, const float *as, int mode) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < 3; ++c) os[c] = s.g == c ? 0.65f : 0.15f;
  ol[0] = (float)s.v[0]; ol[1] = (float)s.v[1];
#pragma unroll
  for (int l = 0; l < MPE_COMM_L; ++l) { ol[2 + 2 * l] = (float)(s.lp[l][0] - s.p[0]); ol[3 + 2 * l] = (float)(s.lp[l][1] - s.p[1]); }
  int ci = (as && mode == 1) ? (int)as[0] : -1;
  if (as && mode == 1) ci = ci < 0 ? 0 : (ci > 2 ? 2 : ci);        // the symbol mpe_comm_step_env keeps as state: out of range -> the nearest
#pragma unroll
  for (int c = 0; c < MPE_COMM_C; ++c) ol[8 + c] = !as ? 0.f : (mode == 0 ? as[c] : (ci == c ? 1.f : 0.f));
}

__device__ __forceinline__ void mpe_comm_load(const MpeCommArgs &a, int n, MpeCommState &s) {
  s.p[0] = a.pos[(size_t)n * 2]; s.p[1] = a.pos[(size_t)n * 2 + 1];
  s.v[0] = a.vel[(size_t)n * 2]; s.v[1] = a.vel[(size_t)n * 2 + 1];
#pragma unroll
  for (int l = 0; l < MPE_COMM_L; ++l) { s.lp[l][0] = a.lpos[((size_t)n * MPE_COMM_L + l) * 2]; s.lp[l][1] = a.lpos[((size_t)n * MPE_COMM_L + l) * 2 + 1]; }
  const int k = a.goal[n];
  s.g = k < 0 ? 0 : (k > 2 ? 2 : k);
  s.sym = a.symbol[n];
  s.tstep = a.tstep[n];
  s.episode = a.episode[n];
}

// landmarks: also the landmark positions, the goal and the episode counter (they change only at a reset)
__device__ __forceinline__ void mpe_comm_store(const MpeCommArgs &a, int n, const MpeCommState &s, bool landmarks) {
  a.pos[(size_t)n * 2] = s.p[0]; a.pos[(size_t)n * 2 + 1] = s.p[1];
  a.vel[(size_t)n * 2] = s.v[0]; a.vel[(size_t)n * 2 + 1] = s.v[1];
  a.symbol[n] = s.sym;
  a.tstep[n] = s.tstep;
  if (landmarks) {
#pragma unroll
    for (int l = 0; l < MPE_COMM_L; ++l) { a.lpos[((size_t)n * MPE_COMM_L + l) * 2] = s.lp[l][0]; a.lpos[((size_t)n * MPE_COMM_L + l) * 2 + 1] = s.lp[l][1]; }
    a.goal[n] = s.g;
    a.episode[n] = s.episode;
  }
}

// One step of environment n on the state the lane holds: the listener's action -> force, integration, the speaker's symbol -> the
// channel, shared reward, time-limit done, reset-on-done, observations.  as / al: the environment's own actions (a.mode 0: 3 and 5
// floats | 1: one index each); os / ol: its two observation rows (3 and 11 floats).  reward: what BOTH agents receive.  Returns
// done (the state is then the reset state: new landmarks and goal, c = 0).
__device__ __forceinline__ bool mpe_comm_step_env(const MpeCommArgs &a, int n, const float *as, const float *al, MpeCommState &s, float *os,
                                                  float *ol, float &reward) {
  // contraction pinned off for the reason given in mpe_step_env: the body is inlined into two kernels that must agree to the bit,
  // and here every value is also held EQUAL to the reference's float64 (no transcendental in this scenario)
#pragma clang fp contract(off)
  // ---- the listener's action -> force (environment.py:194-256: u = [a1 - a2, a3 - a4] * sensitivity 5; core.py:227-236: mass 1,
  // no noise, no collisions) and integrate (core.py:264-275); the speaker is not movable ----
  double u0, u1;
  if (a.mode == 0) {
    u0 = (double)al[1] - (double)al[2]; u1 = (double)al[3] - (double)al[4];
  } else {
    const int m = (int)al[0];
    u0 = m == 1 ? 1.0 : (m == 2 ? -1.0 : 0.0);                      // the one-hot of index m through the line above
    u1 = m == 3 ? 1.0 : (m == 4 ? -1.0 : 0.0);
  }
  const double f0 = 5.0 * u0, f1 = 5.0 * u1;
  s.v[0] = s.v[0] * (1.0 - 0.25); s.v[1] = s.v[1] * (1.0 - 0.25);
  s.v[0] += f0 * 0.1; s.v[1] += f1 * 0.1;
  s.p[0] += s.v[0] * 0.1; s.p[1] += s.v[1] * 0.1;
  // ---- the speaker's symbol -> the channel (core.py:277-287: state.c = action.c) ----
  if (a.mode == 0) s.sym = as[0] >= as[1] ? (as[0] >= as[2] ? 0 : 2) : (as[1] >= as[2] ? 1 : 2);
  else { const int c = (int)as[0]; s.sym = c < 0 ? 0 : (c > 2 ? 2 : c); }
  // ---- reward (simple_speaker_listener.py:69-73: -|listener - goal landmark|^2 for either agent; collaborative: both receive the
  // sum over the agents, environment.py:139-143) ----
  const double lx = s.g == 0 ? s.lp[0][0] : (s.g == 1 ? s.lp[1][0] : s.lp[2][0]);
  const double ly = s.g == 0 ? s.lp[0][1] : (s.g == 1 ? s.lp[1][1] : s.lp[2][1]);
  const double dx = s.p[0] - lx, dy = s.p[1] - ly;
  const double r = -(dx * dx + dy * dy);
  reward = (float)(r + r);
  const int t = s.tstep + 1;
  const bool done = t >= a.T;                                       // environment.py:179-185
  if (done) {                                                       // vec-env wrappers: the returned obs are the reset obs
    s.episode += 1;
    mpe_comm_reset_env(a, n, s, s.episode);
    s.tstep = 0;
  } else {
    s.tstep = t;
  }
  mpe_comm_write_obs(os, ol, s, done ? nullptr : as, a.mode);       // the listener hears the symbol said in this same step
  return done;
}
