// mpe_ref_core.h — the MPE `simple_reference` environment as device functions: reset, one environment step and the observation
// write, one lane per environment.  Shared by the stepwise kernels (mpe_ref_env.hip) and the one-launch rollout episode
// (rollout_reference.h), so a step computes the same float64 values whichever launch runs it.  Reference sites: see mpe_ref_env.hip.
//
// Fixed shape (the scenario asserts 2 agents and colours exactly 3 landmarks): M = 2 agents, L = 3 landmarks, dim_c = 10, action
// space MultiDiscrete([[0, 4], [0, 9]]) = a move head of 5 and a communication head of 10, 21 observation features.  The
// communication state needs no storage: the step that sets it writes it into the observations, and a reset clears it.
//
// Reset draws: Philox stream (seed, episode), mpe_uniform index MPE_REF_DRAWS * n + k for environment n —
//   k = 0 .. 3    agent i position x, y at 2 i, 2 i + 1
//   k = 4 .. 9    landmark l position x, y at 4 + 2 l, 4 + 2 l + 1 (scaled by 0.8)
//   k = 10, 11    goal of agent i at 10 + i: min(2, floor(3 u)), u = (draw + 1) / 2 in [0, 1)
//   k = 12 .. 15  unused
// so no two draws of one (seed, episode) share an index.
#pragma once
#include "mpe_core.h"

#define MPE_REF_M 2
#define MPE_REF_L 3
#define MPE_REF_C 10
#define MPE_REF_A 15                                                // 5 + dim_c: the env's one-hot action width (mode 0)
#define MPE_REF_K 2                                                 // action heads: the buffer's action columns (mode 1)
#define MPE_REF_OBS 21                                              // 2 + 2 L + 3 + dim_c
#define MPE_REF_DRAWS 16

struct MpeRefArgs {
  double *apos, *avel, *lpos;      // [N][2][2], [N][2][2], [N][3][2]
  int32_t *goal;                   // [N][2] landmark index of each agent's goal_b
  int32_t *tstep;                  // [N] steps since the last reset
  int64_t *episode;                // [N] resets so far (Philox counter)
  const float *actions;            // mode 0: the heads' one-hots / probabilities side by side [N][2][15] | mode 1: head indices [N][2][2]
  float *obs, *rewards;            // [N][2][21], [N][2]
  uint8_t *dones;                  // [N][2] bool bytes
  int N, T, mode;
  uint64_t seed;
};

// scenario.reset_world (simple_reference.py:34-60): goals uniform over the landmarks, agents U(-1,1)^2 at rest with c = 0,
// landmarks 0.8 U(-1,1)^2
__device__ __forceinline__ void mpe_ref_reset_env(const MpeRefArgs &p, int n, double (&ap)[MPE_REF_M][2], double (&av)[MPE_REF_M][2],
                                                  double (&lp)[MPE_REF_L][2], int (&g)[MPE_REF_M], int64_t ep) {
#pragma clang fp contract(off)   // as in mpe_ref_step_env, which inlines this
  const uint64_t base = (uint64_t)n * MPE_REF_DRAWS;
#pragma unroll
  for (int i = 0; i < MPE_REF_M; ++i) {
    ap[i][0] = mpe_uniform(p.seed, (uint64_t)ep, base + 2 * i);
    ap[i][1] = mpe_uniform(p.seed, (uint64_t)ep, base + 2 * i + 1);
    av[i][0] = av[i][1] = 0.0;
    const double u = (mpe_uniform(p.seed, (uint64_t)ep, base + 10 + i) + 1.0) * 0.5;
    const int k = (int)floor(3.0 * u);
    g[i] = k < 0 ? 0 : (k > 2 ? 2 : k);
  }
#pragma unroll
  for (int l = 0; l < MPE_REF_L; ++l) {
    lp[l][0] = 0.8 * mpe_uniform(p.seed, (uint64_t)ep, base + 4 + 2 * l);
    lp[l][1] = 0.8 * mpe_uniform(p.seed, (uint64_t)ep, base + 4 + 2 * l + 1);
  }
}

// scenario.observation (simple_reference.py:69-97): [vel, landmarks - pos, colour of the own goal landmark, the other agent's c];
// obs: the environment's 2 rows of 21 floats.  act: the actions that set c in this step (mode as in MpeRefArgs), or null: c = 0
// (after a reset)
__device__ __forceinline__ void mpe_ref_write_obs(float *obs, const double (&ap)[MPE_REF_M][2], const double (&av)[MPE_REF_M][2],
                                                  const double (&lp)[MPE_REF_L][2], const int (&g)[MPE_REF_M], const float *act, int mode) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < MPE_REF_M; ++i) {
    float *o = obs + i * MPE_REF_OBS;
    o[0] = (float)av[i][0]; o[1] = (float)av[i][1];
    int k = 2;
#pragma unroll
    for (int l = 0; l < MPE_REF_L; ++l) { o[k++] = (float)(lp[l][0] - ap[i][0]); o[k++] = (float)(lp[l][1] - ap[i][1]); }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[k++] = g[i] == c ? 0.75f : 0.25f;         // landmark colours (.75,.25,.25), (.25,.75,.25), (.25,.25,.75)
    const int other = 1 - i;
    const int ci = (act && mode == 1) ? (int)act[other * MPE_REF_K + 1] : -1;
    for (int c = 0; c < MPE_REF_C; ++c)
      o[k++] = !act ? 0.f : (mode == 0 ? act[other * MPE_REF_A + 5 + c] : (ci == c ? 1.f : 0.f));
  }
}

__device__ __forceinline__ void mpe_ref_load(const MpeRefArgs &p, int n, double (&ap)[MPE_REF_M][2], double (&av)[MPE_REF_M][2],
                                             double (&lp)[MPE_REF_L][2], int (&g)[MPE_REF_M]) {
#pragma unroll
  for (int i = 0; i < MPE_REF_M; ++i) {
    ap[i][0] = p.apos[((size_t)n * MPE_REF_M + i) * 2]; ap[i][1] = p.apos[((size_t)n * MPE_REF_M + i) * 2 + 1];
    av[i][0] = p.avel[((size_t)n * MPE_REF_M + i) * 2]; av[i][1] = p.avel[((size_t)n * MPE_REF_M + i) * 2 + 1];
    const int k = p.goal[(size_t)n * MPE_REF_M + i];
    g[i] = k < 0 ? 0 : (k > 2 ? 2 : k);
  }
#pragma unroll
  for (int l = 0; l < MPE_REF_L; ++l) { lp[l][0] = p.lpos[((size_t)n * MPE_REF_L + l) * 2]; lp[l][1] = p.lpos[((size_t)n * MPE_REF_L + l) * 2 + 1]; }
}

// landmarks: also the landmark positions and the goals (they change only at a reset)
__device__ __forceinline__ void mpe_ref_store(const MpeRefArgs &p, int n, const double (&ap)[MPE_REF_M][2], const double (&av)[MPE_REF_M][2],
                                              const double (&lp)[MPE_REF_L][2], const int (&g)[MPE_REF_M], bool landmarks) {
#pragma unroll
  for (int i = 0; i < MPE_REF_M; ++i) {
    p.apos[((size_t)n * MPE_REF_M + i) * 2] = ap[i][0]; p.apos[((size_t)n * MPE_REF_M + i) * 2 + 1] = ap[i][1];
    p.avel[((size_t)n * MPE_REF_M + i) * 2] = av[i][0]; p.avel[((size_t)n * MPE_REF_M + i) * 2 + 1] = av[i][1];
  }
  if (landmarks) {
#pragma unroll
    for (int l = 0; l < MPE_REF_L; ++l) { p.lpos[((size_t)n * MPE_REF_L + l) * 2] = lp[l][0]; p.lpos[((size_t)n * MPE_REF_L + l) * 2 + 1] = lp[l][1]; }
#pragma unroll
    for (int i = 0; i < MPE_REF_M; ++i) p.goal[(size_t)n * MPE_REF_M + i] = g[i];
  }
}

// One step of environment n on the state the lane holds (ap, av, lp, g, tstep, episode): action -> force and communication,
// integration, shared reward, time-limit done, reset-on-done, observations.  Everything the step reads and writes besides that
// state is the environment's own slice: act (p.mode 0: 2 x 15 | 1: 2 x 2 head indices), obs (2 rows), rewards [2], and dones [2]
// (bool bytes) and / or masks [2] (1 - done as fp32, the rollout buffer's form) — either may be null.  Returns done (the state
// is then the reset state: new landmarks and goals, c = 0).
__device__ __forceinline__ bool mpe_ref_step_env(const MpeRefArgs &p, int n, const float *act, double (&ap)[MPE_REF_M][2],
                                                 double (&av)[MPE_REF_M][2], double (&lp)[MPE_REF_L][2], int (&g)[MPE_REF_M], int32_t &tstep,
                                                 int64_t &episode, float *obs, float *rewards, uint8_t *dones, float *masks) {
  // contraction pinned off for the reason given in mpe_step_env: the body is inlined into two kernels that must agree to the bit,
  // and here every value is also held EQUAL to the reference's float64 (no transcendental in this scenario)
#pragma clang fp contract(off)
  // ---- action -> force (environment.py:194-256, MultiDiscrete split :198-205: u = [a1 - a2, a3 - a4] * sensitivity 5; core.py:
  // 227-236: mass 1, no noise; agents do not collide, so this is the whole force) and integrate (core.py:264-275) ----
#pragma unroll
  for (int i = 0; i < MPE_REF_M; ++i) {
    double u0, u1;
    if (p.mode == 0) {
      const float *a = act + i * MPE_REF_A;
      u0 = (double)a[1] - (double)a[2]; u1 = (double)a[3] - (double)a[4];
    } else {
      const int a = (int)act[i * MPE_REF_K];
      u0 = a == 1 ? 1.0 : (a == 2 ? -1.0 : 0.0);                    // the one-hot of index a through the line above
      u1 = a == 3 ? 1.0 : (a == 4 ? -1.0 : 0.0);
    }
    const double f0 = 5.0 * u0, f1 = 5.0 * u1;
    av[i][0] = av[i][0] * (1.0 - 0.25); av[i][1] = av[i][1] * (1.0 - 0.25);
    av[i][0] += f0 * 0.1; av[i][1] += f1 * 0.1;
    ap[i][0] += av[i][0] * 0.1; ap[i][1] += av[i][1] * 0.1;
  }
  // ---- reward (simple_reference.py:62-67: -|pos(goal_a = the other agent) - landmark goal_b|^2; shared: environment.py:139-143) ----
  double total = 0.0;
#pragma unroll
  for (int i = 0; i < MPE_REF_M; ++i) {
    const double lx = g[i] == 0 ? lp[0][0] : (g[i] == 1 ? lp[1][0] : lp[2][0]);
    const double ly = g[i] == 0 ? lp[0][1] : (g[i] == 1 ? lp[1][1] : lp[2][1]);
    const double dx = ap[1 - i][0] - lx, dy = ap[1 - i][1] - ly;
    const double r = -(dx * dx + dy * dy);
    total = i == 0 ? r : total + r;
  }
  const int t = tstep + 1;
  const bool done = t >= p.T;                                       // environment.py:179-185
#pragma unroll
  for (int i = 0; i < MPE_REF_M; ++i) {
    rewards[i] = (float)total;
    if (dones) dones[i] = done ? 1 : 0;
    if (masks) masks[i] = done ? 0.f : 1.f;
  }
  if (done) {                                                       // vec-env wrappers: the returned obs are the reset obs
    episode += 1;
    mpe_ref_reset_env(p, n, ap, av, lp, g, episode);
    tstep = 0;
  } else {
    tstep = t;
  }
  mpe_ref_write_obs(obs, ap, av, lp, g, done ? nullptr : act, p.mode);          // state.c = action.c (core.py:277-287)
  return done;
}
