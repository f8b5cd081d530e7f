// mpe_ref_env.hip — GPU-vectorised MPE `simple_reference`: N environments x 2 agents x 3 landmarks stepped by ONE
// kernel launch, one lane per environment.  Reference: onpolicy/envs/mpe/environment.py:194-256 (action decoding, the
// MultiDiscrete split at :198-205), :139-143 (shared reward), :179-185 (time-limit done); onpolicy/envs/mpe/core.py:207-287
// (World.step: action force, damping + integration, state.c = action.c; the agents do not collide);
// onpolicy/envs/mpe/scenarios/simple_reference.py:34-60 (reset), :62-67 (reward), :69-97 (observation); and the reset-on-done of
// the vec-env wrappers (envs/env_wrappers.py:146-152,676-682).
//
// Float64 as in the reference's NumPy code, and with no transcendental in this scenario and contraction off the outputs EQUAL the
// fp32 cast of the reference's (tests/golden/mpe_envs.npz).  State is device resident; resets draw from the counter-based Philox
// stream keyed by (seed, episode, index) — index layout in mpe_ref_core.h.
#include "mpe_ref_core.h"

__global__ __launch_bounds__(256) void mpe_reference_reset_kernel(MpeRefArgs p) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= p.N) return;
  double ap[MPE_REF_M][2], av[MPE_REF_M][2], lp[MPE_REF_L][2];
  int g[MPE_REF_M];
  const int64_t ep = p.episode[n] + 1;
  mpe_ref_reset_env(p, n, ap, av, lp, g, ep);
  p.episode[n] = ep;
  p.tstep[n] = 0;
  mpe_ref_store(p, n, ap, av, lp, g, true);
  mpe_ref_write_obs(p.obs + (size_t)n * MPE_REF_M * MPE_REF_OBS, ap, av, lp, g, nullptr, 0);
}

__global__ __launch_bounds__(256) void mpe_reference_step_kernel(MpeRefArgs p) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= p.N) return;
  double ap[MPE_REF_M][2], av[MPE_REF_M][2], lp[MPE_REF_L][2];
  int g[MPE_REF_M];
  mpe_ref_load(p, n, ap, av, lp, g);
  int32_t tstep = p.tstep[n];
  int64_t episode = p.episode[n];
  const bool done = mpe_ref_step_env(p, n, p.actions + (size_t)n * MPE_REF_M * (p.mode == 0 ? MPE_REF_A : MPE_REF_K), ap, av, lp, g, tstep,
                                     episode, p.obs + (size_t)n * MPE_REF_M * MPE_REF_OBS, p.rewards + (size_t)n * MPE_REF_M,
                                     p.dones + (size_t)n * MPE_REF_M, nullptr);
  p.tstep[n] = tstep;
  if (done) p.episode[n] = episode;
  mpe_ref_store(p, n, ap, av, lp, g, done);
}

extern "C" int mappo_mpe_reference_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                                         int64_t *episode, float *obs, int32_t N, uint64_t seed, mappo_stream_t stream) {
  MAPPO_REQUIRE(N >= 1, "mpe_reference_reset: N=%d, needs at least one environment (N >= 1)", N);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode && obs, "mpe_reference_reset: null pointer");
  MpeRefArgs p = {};
  p.apos = agent_pos; p.avel = agent_vel; p.lpos = landmark_pos; p.goal = goal; p.tstep = tstep; p.episode = episode; p.obs = obs;
  p.N = N; p.seed = seed;
  hipLaunchKernelGGL(mpe_reference_reset_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), p);
  MAPPO_CHECK_LAUNCH("mpe_reference_reset");
  return MAPPO_OK;
}

extern "C" int mappo_mpe_reference_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                                        int64_t *episode, const float *actions, int32_t action_mode, float *obs, float *rewards,
                                        uint8_t *dones, int32_t N, int32_t episode_length, uint64_t seed, mappo_stream_t stream) {
  MAPPO_REQUIRE(N >= 1, "mpe_reference_step: N=%d, needs at least one environment (N >= 1)", N);
  MAPPO_REQUIRE(action_mode == 0 || action_mode == 1, "mpe_reference_step: action_mode %d (0: one-hot [N][2][15], 1: head indices [N][2][2])",
                action_mode);
  MAPPO_REQUIRE(episode_length >= 1, "mpe_reference_step: episode length %d, needs >= 1", episode_length);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode && actions && obs && rewards && dones,
                "mpe_reference_step: null pointer");
  MpeRefArgs p = {};
  p.apos = agent_pos; p.avel = agent_vel; p.lpos = landmark_pos; p.goal = goal; p.tstep = tstep; p.episode = episode; p.actions = actions;
  p.obs = obs; p.rewards = rewards; p.dones = dones; p.N = N; p.T = episode_length; p.mode = action_mode; p.seed = seed;
  hipLaunchKernelGGL(mpe_reference_step_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), p);
  MAPPO_CHECK_LAUNCH("mpe_reference_step");
  return MAPPO_OK;
}
