// mpe_adv_env.hip — GPU-vectorised MPE `simple_adversary`: N environments x (adversary, two good agents) x 2 landmarks stepped by ONE
// kernel launch, one lane per environment.  Reference: onpolicy/envs/mpe/environment.py:194-256 (action decoding), :49-50,142
// (world.collaborative is not set: per-agent rewards), :179-185 (time-limit done); onpolicy/envs/mpe/core.py:207-287 (World.step:
// action force, damping + integration; nothing collides); onpolicy/envs/mpe/scenarios/simple_adversary.py:36-53 (reset), :74-116
// (reward), :119-137 (observation); and the reset-on-done of the vec-env wrappers (envs/env_wrappers.py:146-152).
//
// Float64 as in the reference's NumPy code; the only function beyond add and multiply is a correctly rounded sqrt, and with
// contraction off the outputs EQUAL the fp32 cast of the reference's (tests/golden/mpe_adversary.npz).  State is device resident;
// resets draw from the counter-based Philox stream keyed by (seed, episode, index) — index layout in mpe_adv_core.h.
#include "mpe_adv_core.h"

__global__ __launch_bounds__(256) void mpe_adv_reset_kernel(MpeAdvArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpeAdvState s;
  s.episode = a.episode[n] + 1;
  s.tstep = 0;
  mpe_adv_reset_env(a, n, s, s.episode);
  mpe_adv_store(a, n, s, true);
  mpe_adv_write_obs(a.obs[0] + (size_t)n * MPE_ADV_OBS_A, a.obs[1] + (size_t)n * MPE_ADV_OBS_G, a.obs[2] + (size_t)n * MPE_ADV_OBS_G, s);
}

__global__ __launch_bounds__(256) void mpe_adv_step_kernel(MpeAdvArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpeAdvState s;
  mpe_adv_load(a, n, s);
  const int stride = a.mode == 0 ? MPE_ADV_U : 1;
  float reward[MPE_ADV_M];
  const bool done = mpe_adv_step_env(a, n, a.act + (size_t)n * MPE_ADV_M * stride, stride, s, a.obs[0] + (size_t)n * MPE_ADV_OBS_A,
                                     a.obs[1] + (size_t)n * MPE_ADV_OBS_G, a.obs[2] + (size_t)n * MPE_ADV_OBS_G, reward);
#pragma unroll
  for (int m = 0; m < MPE_ADV_M; ++m) {
    a.rewards[(size_t)n * MPE_ADV_M + m] = reward[m];
    a.dones[(size_t)n * MPE_ADV_M + m] = done ? 1 : 0;
  }
  mpe_adv_store(a, n, s, done);
}

extern "C" int mappo_mpe_adversary_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                                         int64_t *episode, float *obs_adversary, float *obs_good1, float *obs_good2, int32_t N,
                                         int32_t num_agents, uint64_t seed, mappo_stream_t stream) {
  MAPPO_REQUIRE(num_agents == MPE_ADV_M, "mpe_adversary_reset: num_agents=%d: simple_adversary is built for num_agents = 3 (1 adversary, 2 "
                "good agents, 2 landmarks)", num_agents);
  MAPPO_REQUIRE(N >= 1, "mpe_adversary_reset: N=%d, needs at least one environment (N >= 1)", N);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode && obs_adversary && obs_good1 && obs_good2,
                "mpe_adversary_reset: null pointer");
  MpeAdvArgs a = {};
  a.apos = agent_pos; a.avel = agent_vel; a.lpos = landmark_pos; a.goal = goal; a.tstep = tstep; a.episode = episode;
  a.obs[0] = obs_adversary; a.obs[1] = obs_good1; a.obs[2] = obs_good2; a.N = N; a.seed = seed;
  hipLaunchKernelGGL(mpe_adv_reset_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_adversary_reset");
  return MAPPO_OK;
}

extern "C" int mappo_mpe_adversary_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                                        int64_t *episode, const float *actions, int32_t action_mode, float *obs_adversary,
                                        float *obs_good1, float *obs_good2, float *rewards, uint8_t *dones, int32_t N, int32_t num_agents,
                                        int32_t episode_length, uint64_t seed, mappo_stream_t stream) {
  MAPPO_REQUIRE(num_agents == MPE_ADV_M, "mpe_adversary_step: num_agents=%d: simple_adversary is built for num_agents = 3 (1 adversary, 2 "
                "good agents, 2 landmarks)", num_agents);
  MAPPO_REQUIRE(N >= 1, "mpe_adversary_step: N=%d, needs at least one environment (N >= 1)", N);
  MAPPO_REQUIRE(action_mode == 0 || action_mode == 1, "mpe_adversary_step: action_mode %d (0: one-hots [N][3][5]; 1: indices [N][3])",
                action_mode);
  MAPPO_REQUIRE(episode_length >= 1, "mpe_adversary_step: episode length %d, needs >= 1", episode_length);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode && actions && obs_adversary && obs_good1 && obs_good2 &&
                rewards && dones, "mpe_adversary_step: null pointer");
  MpeAdvArgs a = {};
  a.apos = agent_pos; a.avel = agent_vel; a.lpos = landmark_pos; a.goal = goal; a.tstep = tstep; a.episode = episode;
  a.act = actions; a.obs[0] = obs_adversary; a.obs[1] = obs_good1; a.obs[2] = obs_good2; a.rewards = rewards; a.dones = dones;
  a.N = N; a.T = episode_length; a.mode = action_mode; a.seed = seed;
  hipLaunchKernelGGL(mpe_adv_step_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_adversary_step");
  return MAPPO_OK;
}
