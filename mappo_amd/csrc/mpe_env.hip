// mpe_env.hip — GPU-vectorised MPE `simple_spread`: N environments x M agents x L landmarks stepped by ONE
// kernel launch, one lane per environment.  Reference: onpolicy/envs/mpe/core.py:207-322 (World.step: action forces,
// pairwise soft-collision force, damping + integration), onpolicy/envs/mpe/scenarios/simple_spread.py:32-103 (reset, reward,
// observation), onpolicy/envs/mpe/environment.py:117-256 (action decoding, shared reward, time-limit done) and the reset-on-
// done of the vec-env wrappers (envs/env_wrappers.py:146-152,676-682).
//
// The reference computes in float64 NumPy; so does this kernel (an environment is ~200 flops per step: the launch is bound
// by its 20 + 72 M bytes of state / output per environment, not by the fp64 rate), so trajectories agree with the oracle to
// rounding of the transcendental functions and the fp32 cast of the outputs.  State (positions, velocities, landmarks, step
// and episode counters) is device resident; resets draw from a counter-based Philox stream keyed by (seed, episode, env), so
// the step is a pure device op and an episode of rollout steps + env steps can be captured into one hipGraph.
#include "mpe_core.h"

__global__ __launch_bounds__(256) void mpe_spread_reset_kernel(MpeArgs p) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= p.N) return;
  double ap[MPE_MAX_M][2], av[MPE_MAX_M][2], lp[MPE_MAX_L][2];
  const int64_t ep = p.episode[n] + 1;
  mpe_reset_env(p, n, ap, av, lp, ep);
  p.episode[n] = ep;
  p.tstep[n] = 0;
  mpe_store(p, n, ap, av, lp, true);
  mpe_write_obs(p, p.obs + (size_t)n * p.M * (4 + 2 * p.L + 4 * (p.M - 1)), ap, av, lp);
}

__global__ __launch_bounds__(256) void mpe_spread_step_kernel(MpeArgs p) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= p.N) return;
  const int M = p.M;
  double ap[MPE_MAX_M][2], av[MPE_MAX_M][2], lp[MPE_MAX_L][2];
  mpe_load(p, n, ap, av, lp);
  int32_t tstep = p.tstep[n];
  int64_t episode = p.episode[n];
  const bool done = mpe_step_env(p, n, p.actions + (size_t)n * M * (p.mode == 0 ? 5 : 1), ap, av, lp, tstep, episode,
                                 p.obs + (size_t)n * M * (4 + 2 * p.L + 4 * (M - 1)), p.rewards + (size_t)n * M, p.dones + (size_t)n * M, nullptr);
  p.tstep[n] = tstep;
  if (done) p.episode[n] = episode;
  mpe_store(p, n, ap, av, lp, done);
}

static int mpe_check(int N, int M, int L, const char *who) {
  MAPPO_REQUIRE(N > 0 && M >= 1 && M <= MPE_MAX_M && L >= 1 && L <= MPE_MAX_L, "%s: N=%d M=%d L=%d unsupported (M, L <= %d)", who, N, M, L,
                MPE_MAX_M);
  return MAPPO_OK;
}

extern "C" int mappo_mpe_spread_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                                      float *obs, int32_t N, int32_t M, int32_t L, uint64_t seed, mappo_stream_t stream) {
  if (int rc = mpe_check(N, M, L, "mpe_spread_reset")) return rc;
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && tstep && episode && obs, "mpe_spread_reset: null pointer");
  MpeArgs p = {};
  p.apos = agent_pos; p.avel = agent_vel; p.lpos = landmark_pos; p.tstep = tstep; p.episode = episode; p.obs = obs;
  p.N = N; p.M = M; p.L = L; p.seed = seed;
  hipLaunchKernelGGL(mpe_spread_reset_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), p);
  MAPPO_CHECK_LAUNCH("mpe_spread_reset");
  return MAPPO_OK;
}

extern "C" int mappo_mpe_spread_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                                     const float *actions, int32_t action_mode, float *obs, float *rewards, uint8_t *dones, int32_t N,
                                     int32_t M, int32_t L, int32_t episode_length, uint64_t seed, mappo_stream_t stream) {
  if (int rc = mpe_check(N, M, L, "mpe_spread_step")) return rc;
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && tstep && episode && actions && obs && rewards && dones,
                "mpe_spread_step: null pointer");
  MAPPO_REQUIRE(action_mode == 0 || action_mode == 1, "mpe_spread_step: action_mode %d", action_mode);
  MpeArgs p = {};
  p.apos = agent_pos; p.avel = agent_vel; p.lpos = landmark_pos; p.tstep = tstep; p.episode = episode; p.actions = actions;
  p.obs = obs; p.rewards = rewards; p.dones = dones; p.N = N; p.M = M; p.L = L; p.T = episode_length; p.mode = action_mode; p.seed = seed;
  hipLaunchKernelGGL(mpe_spread_step_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), p);
  MAPPO_CHECK_LAUNCH("mpe_spread_step");
  return MAPPO_OK;
}
