// mpe_comm_env.hip — GPU-vectorised MPE `simple_speaker_listener`: N environments x (speaker, listener) x 3 landmarks stepped by ONE
// kernel launch, one lane per environment.  Reference: onpolicy/envs/mpe/environment.py:194-256 (action decoding), :139-143
// (collaborative reward: the sum over the agents), :179-185 (time-limit done); onpolicy/envs/mpe/core.py:207-287 (World.step: action
// force, damping + integration, state.c = action.c; nothing collides); onpolicy/envs/mpe/scenarios/simple_speaker_listener.py:38-63
// (reset), :69-73 (reward), :75-98 (observation); and the reset-on-done of the vec-env wrappers (envs/env_wrappers.py:146-152).
//
// Float64 as in the reference's NumPy code, and with no transcendental in this scenario and contraction off the outputs EQUAL the
// fp32 cast of the reference's (tests/golden/mpe_comm.npz).  State is device resident; resets draw from the counter-based Philox
// stream keyed by (seed, episode, index) — index layout in mpe_comm_core.h.
#include "mpe_comm_core.h"

__global__ __launch_bounds__(256) void mpe_comm_reset_kernel(MpeCommArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpeCommState s;
  s.episode = a.episode[n] + 1;
  s.tstep = 0;
  mpe_comm_reset_env(a, n, s, s.episode);
  mpe_comm_store(a, n, s, true);
  mpe_comm_write_obs(a.obs_s + (size_t)n * MPE_COMM_OBS_S, a.obs_l + (size_t)n * MPE_COMM_OBS_L, s, nullptr, 0);
}

__global__ __launch_bounds__(256) void mpe_comm_step_kernel(MpeCommArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpeCommState s;
  mpe_comm_load(a, n, s);
  const float *as = a.mode == 0 ? a.act_s + (size_t)n * MPE_COMM_C : a.act_s + (size_t)n * MPE_COMM_M;
  const float *al = a.mode == 0 ? a.act_l + (size_t)n * MPE_COMM_U : a.act_s + (size_t)n * MPE_COMM_M + 1;
  float reward;
  const bool done = mpe_comm_step_env(a, n, as, al, s, a.obs_s + (size_t)n * MPE_COMM_OBS_S, a.obs_l + (size_t)n * MPE_COMM_OBS_L, reward);
#pragma unroll
  for (int i = 0; i < MPE_COMM_M; ++i) {
    a.rewards[(size_t)n * MPE_COMM_M + i] = reward;
    a.dones[(size_t)n * MPE_COMM_M + i] = done ? 1 : 0;
  }
  mpe_comm_store(a, n, s, done);
}

extern "C" int mappo_mpe_comm_reset(double *listener_pos, double *listener_vel, double *landmark_pos, int32_t *goal, int32_t *symbol,
                                    int32_t *tstep, int64_t *episode, float *obs_speaker, float *obs_listener, int32_t N, uint64_t seed,
                                    mappo_stream_t stream) {
  MAPPO_REQUIRE(N >= 1, "mpe_comm_reset: N=%d, needs at least one environment (N >= 1)", N);
  MAPPO_REQUIRE(listener_pos && listener_vel && landmark_pos && goal && symbol && tstep && episode && obs_speaker && obs_listener,
                "mpe_comm_reset: null pointer");
  MpeCommArgs a = {};
  a.pos = listener_pos; a.vel = listener_vel; a.lpos = landmark_pos; a.goal = goal; a.symbol = symbol; a.tstep = tstep; a.episode = episode;
  a.obs_s = obs_speaker; a.obs_l = obs_listener; a.N = N; a.seed = seed;
  hipLaunchKernelGGL(mpe_comm_reset_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_comm_reset");
  return MAPPO_OK;
}

extern "C" int mappo_mpe_comm_step(double *listener_pos, double *listener_vel, double *landmark_pos, int32_t *goal, int32_t *symbol,
                                   int32_t *tstep, int64_t *episode, const float *actions_speaker, const float *actions_listener,
                                   int32_t action_mode, float *obs_speaker, float *obs_listener, float *rewards, uint8_t *dones, int32_t N,
                                   int32_t episode_length, uint64_t seed, mappo_stream_t stream) {
  MAPPO_REQUIRE(N >= 1, "mpe_comm_step: N=%d, needs at least one environment (N >= 1)", N);
  MAPPO_REQUIRE(action_mode == 0 || action_mode == 1, "mpe_comm_step: action_mode %d (0: one-hots, speaker [N][3] and listener [N][5]; "
                "1: indices [N][2])", action_mode);
  MAPPO_REQUIRE(episode_length >= 1, "mpe_comm_step: episode length %d, needs >= 1", episode_length);
  MAPPO_REQUIRE(listener_pos && listener_vel && landmark_pos && goal && symbol && tstep && episode && actions_speaker &&
                (action_mode == 1 || actions_listener) && obs_speaker && obs_listener && rewards && dones, "mpe_comm_step: null pointer");
  MpeCommArgs a = {};
  a.pos = listener_pos; a.vel = listener_vel; a.lpos = landmark_pos; a.goal = goal; a.symbol = symbol; a.tstep = tstep; a.episode = episode;
  a.act_s = actions_speaker; a.act_l = actions_listener; a.obs_s = obs_speaker; a.obs_l = obs_listener; a.rewards = rewards; a.dones = dones;
  a.N = N; a.T = episode_length; a.mode = action_mode; a.seed = seed;
  hipLaunchKernelGGL(mpe_comm_step_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_comm_step");
  return MAPPO_OK;
}
