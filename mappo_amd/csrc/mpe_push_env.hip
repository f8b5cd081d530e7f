// mpe_push_env.hip — GPU-vectorised MPE `simple_push` ("keep-away"): N environments x (adversary, good agent) x 2 landmarks stepped
// by ONE kernel launch, one lane per environment.  Reference: onpolicy/envs/mpe/environment.py:194-256 (action decoding), :49-50,142
// (world.collaborative is not set: per-agent rewards), :179-185 (time-limit done); onpolicy/envs/mpe/core.py:207-322 (World.step:
// action force, the soft-collision force between the two agents, damping, integration; no max_speed);
// onpolicy/envs/mpe/scenarios/simple_push.py:12-40 (both agents collide, the landmarks do not), :42-65 (reset), :67-84 (reward),
// :86-107 (observation); and the reset-on-done of the vec-env wrappers (envs/env_wrappers.py:146-152).
//
// Float64 as in the reference's NumPy code, contraction off.  Beside adds, multiplies and correctly rounded square roots the
// contact force goes through exp and log1p, and the device's are not NumPy's, so outputs match the fp32 cast of the reference's
// (tests/golden/mpe_push.npz) to 1e-6, not by construction to the bit.  State is device resident; resets draw from the
// counter-based Philox stream keyed by (seed, episode, index) — index layout in mpe_push_core.h.
#include "mpe_push_core.h"

__global__ __launch_bounds__(256) void mpe_push_reset_kernel(MpePushArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpePushState s;
  s.episode = a.episode[n] + 1;
  s.tstep = 0;
  mpe_push_reset_env(a, n, s, s.episode);
  mpe_push_store(a, n, s, true);
  mpe_push_write_obs(a.obs[0] + (size_t)n * MPE_PUSH_OBS_A, a.obs[1] + (size_t)n * MPE_PUSH_OBS_G, s);
}

__global__ __launch_bounds__(256) void mpe_push_step_kernel(MpePushArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpePushState s;
  mpe_push_load(a, n, s);
  const int stride = a.mode == 0 ? MPE_PUSH_U : 1;
  float reward[MPE_PUSH_M];
  const bool done = mpe_push_step_env(a, n, a.act + (size_t)n * MPE_PUSH_M * stride, stride, s, a.obs[0] + (size_t)n * MPE_PUSH_OBS_A,
                                      a.obs[1] + (size_t)n * MPE_PUSH_OBS_G, reward);
#pragma unroll
  for (int m = 0; m < MPE_PUSH_M; ++m) {
    a.rewards[(size_t)n * MPE_PUSH_M + m] = reward[m];
    a.dones[(size_t)n * MPE_PUSH_M + m] = done ? 1 : 0;
  }
  mpe_push_store(a, n, s, done);
}

extern "C" int mappo_mpe_push_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                                    int64_t *episode, float *obs_adversary, float *obs_good, int32_t N, int32_t num_agents, uint64_t seed,
                                    mappo_stream_t stream) {
  MAPPO_REQUIRE(num_agents == MPE_PUSH_M, "mpe_push_reset: num_agents=%d: simple_push is built for num_agents = 2 (1 adversary, 1 good "
                "agent, 2 landmarks)", num_agents);
  MAPPO_REQUIRE(N >= 1, "mpe_push_reset: N=%d, needs at least one environment (N >= 1)", N);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode && obs_adversary && obs_good, "mpe_push_reset: null pointer");
  MpePushArgs a = {};
  a.apos = agent_pos; a.avel = agent_vel; a.lpos = landmark_pos; a.goal = goal; a.tstep = tstep; a.episode = episode;
  a.obs[0] = obs_adversary; a.obs[1] = obs_good; a.N = N; a.seed = seed;
  hipLaunchKernelGGL(mpe_push_reset_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_push_reset");
  return MAPPO_OK;
}

extern "C" int mappo_mpe_push_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                                   int64_t *episode, const float *actions, int32_t action_mode, float *obs_adversary, float *obs_good,
                                   float *rewards, uint8_t *dones, int32_t N, int32_t num_agents, int32_t episode_length, uint64_t seed,
                                   mappo_stream_t stream) {
  MAPPO_REQUIRE(num_agents == MPE_PUSH_M, "mpe_push_step: num_agents=%d: simple_push is built for num_agents = 2 (1 adversary, 1 good "
                "agent, 2 landmarks)", num_agents);
  MAPPO_REQUIRE(N >= 1, "mpe_push_step: N=%d, needs at least one environment (N >= 1)", N);
  MAPPO_REQUIRE(action_mode == 0 || action_mode == 1, "mpe_push_step: action_mode %d (0: one-hots [N][2][5]; 1: indices [N][2])", action_mode);
  MAPPO_REQUIRE(episode_length >= 1, "mpe_push_step: episode length %d, needs >= 1", episode_length);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode && actions && obs_adversary && obs_good && rewards && dones,
                "mpe_push_step: null pointer");
  MpePushArgs a = {};
  a.apos = agent_pos; a.avel = agent_vel; a.lpos = landmark_pos; a.goal = goal; a.tstep = tstep; a.episode = episode;
  a.act = actions; a.obs[0] = obs_adversary; a.obs[1] = obs_good; a.rewards = rewards; a.dones = dones;
  a.N = N; a.T = episode_length; a.mode = action_mode; a.seed = seed;
  hipLaunchKernelGGL(mpe_push_step_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_push_step");
  return MAPPO_OK;
}
