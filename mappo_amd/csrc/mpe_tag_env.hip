// mpe_tag_env.hip — GPU-vectorised MPE `simple_tag` (predator-prey): N environments x (three adversaries, one good agent) x 2
// landmarks stepped by ONE kernel launch, one lane per environment.  Reference: onpolicy/envs/mpe/environment.py:194-256 (action
// decoding, accel in place of the sensitivity), :49-50,142 (world.collaborative is not set: per-agent rewards), :179-185 (time-limit
// done); onpolicy/envs/mpe/core.py:207-322 (World.step: action force, soft-collision forces between every pair with a movable
// member, damping, the max_speed clamp, integration); onpolicy/envs/mpe/scenarios/simple_tag.py:20-31 (sizes, accel, max_speed),
// :37-51 (reset), :81-126 (reward), :128-144 (observation); and the reset-on-done of the vec-env wrappers
// (envs/env_wrappers.py:146-152).
//
// Float64 as in the reference's NumPy code, contraction off.  Unlike simple_adversary this step is not only adds, multiplies and
// square roots: the contact force goes through exp and log1p and the boundary penalty through exp, and the device's are not NumPy's,
// so outputs match the fp32 cast of the reference's (tests/golden/mpe_tag.npz) to 1e-6, not to the bit.  State is device resident;
// resets draw from the counter-based Philox stream keyed by (seed, episode, index) — index layout in mpe_tag_core.h.
#include "mpe_tag_core.h"

__global__ __launch_bounds__(256) void mpe_tag_reset_kernel(MpeTagArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpeTagState s;
  s.episode = a.episode[n] + 1;
  s.tstep = 0;
  mpe_tag_reset_env(a, n, s, s.episode);
  mpe_tag_store(a, n, s, true);
  mpe_tag_write_obs(a.obs[0] + (size_t)n * MPE_TAG_OBS_A, a.obs[1] + (size_t)n * MPE_TAG_OBS_A, a.obs[2] + (size_t)n * MPE_TAG_OBS_A,
                    a.obs[3] + (size_t)n * MPE_TAG_OBS_G, s);
}

__global__ __launch_bounds__(256) void mpe_tag_step_kernel(MpeTagArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpeTagState s;
  mpe_tag_load(a, n, s);
  const int stride = a.mode == 0 ? MPE_TAG_U : 1;
  float reward[MPE_TAG_M];
  const bool done = mpe_tag_step_env(a, n, a.act + (size_t)n * MPE_TAG_M * stride, stride, s, a.obs[0] + (size_t)n * MPE_TAG_OBS_A,
                                     a.obs[1] + (size_t)n * MPE_TAG_OBS_A, a.obs[2] + (size_t)n * MPE_TAG_OBS_A,
                                     a.obs[3] + (size_t)n * MPE_TAG_OBS_G, reward);
#pragma unroll
  for (int m = 0; m < MPE_TAG_M; ++m) {
    a.rewards[(size_t)n * MPE_TAG_M + m] = reward[m];
    a.dones[(size_t)n * MPE_TAG_M + m] = done ? 1 : 0;
  }
  mpe_tag_store(a, n, s, done);
}

extern "C" int mappo_mpe_tag_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                                   float *obs_adv0, float *obs_adv1, float *obs_adv2, float *obs_good, int32_t N, int32_t num_agents,
                                   uint64_t seed, mappo_stream_t stream) {
  MAPPO_REQUIRE(num_agents == MPE_TAG_M, "mpe_tag_reset: num_agents=%d: simple_tag is built for num_agents = 4 (3 adversaries, 1 good "
                "agent, 2 landmarks)", num_agents);
  MAPPO_REQUIRE(N >= 1, "mpe_tag_reset: N=%d, needs at least one environment (N >= 1)", N);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && tstep && episode && obs_adv0 && obs_adv1 && obs_adv2 && obs_good,
                "mpe_tag_reset: null pointer");
  MpeTagArgs a = {};
  a.apos = agent_pos; a.avel = agent_vel; a.lpos = landmark_pos; a.tstep = tstep; a.episode = episode;
  a.obs[0] = obs_adv0; a.obs[1] = obs_adv1; a.obs[2] = obs_adv2; a.obs[3] = obs_good; a.N = N; a.seed = seed;
  hipLaunchKernelGGL(mpe_tag_reset_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_tag_reset");
  return MAPPO_OK;
}

extern "C" int mappo_mpe_tag_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                                  const float *actions, int32_t action_mode, float *obs_adv0, float *obs_adv1, float *obs_adv2,
                                  float *obs_good, float *rewards, uint8_t *dones, int32_t N, int32_t num_agents, int32_t episode_length,
                                  uint64_t seed, mappo_stream_t stream) {
  MAPPO_REQUIRE(num_agents == MPE_TAG_M, "mpe_tag_step: num_agents=%d: simple_tag is built for num_agents = 4 (3 adversaries, 1 good "
                "agent, 2 landmarks)", num_agents);
  MAPPO_REQUIRE(N >= 1, "mpe_tag_step: N=%d, needs at least one environment (N >= 1)", N);
  MAPPO_REQUIRE(action_mode == 0 || action_mode == 1, "mpe_tag_step: action_mode %d (0: one-hots [N][4][5]; 1: indices [N][4])", action_mode);
  MAPPO_REQUIRE(episode_length >= 1, "mpe_tag_step: episode length %d, needs >= 1", episode_length);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && tstep && episode && actions && obs_adv0 && obs_adv1 && obs_adv2 && obs_good &&
                rewards && dones, "mpe_tag_step: null pointer");
  MpeTagArgs a = {};
  a.apos = agent_pos; a.avel = agent_vel; a.lpos = landmark_pos; a.tstep = tstep; a.episode = episode;
  a.act = actions; a.obs[0] = obs_adv0; a.obs[1] = obs_adv1; a.obs[2] = obs_adv2; a.obs[3] = obs_good; a.rewards = rewards; a.dones = dones;
  a.N = N; a.T = episode_length; a.mode = action_mode; a.seed = seed;
  hipLaunchKernelGGL(mpe_tag_step_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_tag_step");
  return MAPPO_OK;
}
