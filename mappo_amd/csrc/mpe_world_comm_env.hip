// mpe_world_comm_env.hip — GPU-vectorised MPE `simple_world_comm`: N environments x (four adversaries, the first their leader, two
// good agents) x 5 landmarks (one obstacle, two food items, two forests) stepped by ONE kernel launch, one lane per environment.
// Reference: onpolicy/envs/mpe/environment.py:194-256 (action decoding: the MultiDiscrete split of the leader's action at :198-205,
// accel in place of the sensitivity, the leader's word from its second head), :49-50,142 (world.collaborative is not set: per-agent
// rewards), :179-185 (time-limit done); onpolicy/envs/mpe/core.py:207-322 (World.step: action force, soft-collision forces between
// every pair of colliding entities with a movable member, damping, the max_speed clamp, integration, state.c = action.c);
// onpolicy/envs/mpe/scenarios/simple_world_comm.py:18-52 (sizes, accel, max_speed, the landmark order), :100-112 (reset), :141-199
// (rewards), :225-288 (observation: forest membership decides who sees whom, the leader's word is broadcast); and the reset-on-done of
// the vec-env wrappers (envs/env_wrappers.py:146-152).
//
// Float64 as in the reference's NumPy code, contraction off.  As in simple_tag the contact force goes through exp and log1p and the
// boundary penalty through exp, and the device's are not NumPy's, so float outputs match the fp32 cast of the reference's
// (tests/golden/mpe_world_comm.npz) to 1e-6, not to the bit; the in_forest flags, the zeros of hidden entries, the word and the dones
// are equal.  State is device resident; resets draw from the counter-based Philox stream keyed by (seed, episode, index) — index
// layout in mpe_world_comm_core.h.  The leader's word is not state: the step writes it into the observations it returns.
#include "mpe_world_comm_core.h"

__device__ __forceinline__ void mpe_wc_obs_rows(const MpeWcArgs &a, int n, float *(&o)[MPE_WC_M]) {
#pragma unroll
  for (int m = 0; m < MPE_WC_M; ++m) o[m] = a.obs[m] + (size_t)n * mpe_wc_obs_dim(m);
}

__global__ __launch_bounds__(256) void mpe_world_comm_reset_kernel(MpeWcArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpeWcState s;
  s.episode = a.episode[n] + 1;
  s.tstep = 0;
  mpe_wc_reset_env(a, n, s, s.episode);
  mpe_wc_store(a, n, s, true);
  float *o[MPE_WC_M];
  mpe_wc_obs_rows(a, n, o);
  const float c[MPE_WC_C] = {0.f, 0.f, 0.f, 0.f};
  mpe_wc_write_obs(o, s, c);
}

__global__ __launch_bounds__(256) void mpe_world_comm_step_kernel(MpeWcArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpeWcState s;
  mpe_wc_load(a, n, s);
  MpeWcAction act;
  mpe_wc_decode(a, n, act);
  float *o[MPE_WC_M];
  mpe_wc_obs_rows(a, n, o);
  float reward[MPE_WC_M];
  const bool done = mpe_wc_step_env(a, n, act, s, o, reward);
#pragma unroll
  for (int m = 0; m < MPE_WC_M; ++m) {
    a.rewards[(size_t)n * MPE_WC_M + m] = reward[m];
    a.dones[(size_t)n * MPE_WC_M + m] = done ? 1 : 0;
  }
  mpe_wc_store(a, n, s, done);
}

// what both entry points refuse of the scenario's shape
static int mpe_world_comm_check_shape(const char *who, int32_t N, int32_t num_agents, int32_t num_landmarks) {
  MAPPO_REQUIRE(num_agents == MPE_WC_M, "%s: num_agents=%d: simple_world_comm is built for num_agents = 6 (4 adversaries, the first "
                "their leader, 2 good agents)", who, num_agents);
  MAPPO_REQUIRE(num_landmarks == 1, "%s: num_landmarks=%d: simple_world_comm is built for num_landmarks = 1 (besides it the scenario "
                "itself places 2 food items and 2 forests)", who, num_landmarks);
  MAPPO_REQUIRE(N >= 1, "%s: N=%d, needs at least one environment (N >= 1)", who, N);
  return MAPPO_OK;
}

static bool mpe_world_comm_all(float *const *obs) {
  for (int m = 0; m < MPE_WC_M; ++m)
    if (!obs[m]) return false;
  return true;
}

extern "C" int mappo_mpe_world_comm_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                                          float *const *obs, int32_t N, int32_t num_agents, int32_t num_landmarks, uint64_t seed,
                                          mappo_stream_t stream) {
  if (int rc = mpe_world_comm_check_shape("mpe_world_comm_reset", N, num_agents, num_landmarks)) return rc;
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && tstep && episode && obs && mpe_world_comm_all(obs),
                "mpe_world_comm_reset: null pointer");
  MpeWcArgs a = {};
  a.apos = agent_pos; a.avel = agent_vel; a.lpos = landmark_pos; a.tstep = tstep; a.episode = episode;
  for (int m = 0; m < MPE_WC_M; ++m) a.obs[m] = obs[m];
  a.N = N; a.seed = seed;
  hipLaunchKernelGGL(mpe_world_comm_reset_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_world_comm_reset");
  return MAPPO_OK;
}

extern "C" int mappo_mpe_world_comm_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                                         const float *const *actions, int32_t action_mode, float *const *obs, float *rewards,
                                         uint8_t *dones, int32_t N, int32_t num_agents, int32_t num_landmarks, int32_t episode_length,
                                         uint64_t seed, mappo_stream_t stream) {
  if (int rc = mpe_world_comm_check_shape("mpe_world_comm_step", N, num_agents, num_landmarks)) return rc;
  MAPPO_REQUIRE(action_mode == 0 || action_mode == 1, "mpe_world_comm_step: action_mode %d (0: one-hots, actions[0] [N][9] and "
                "actions[1..5] [N][5]; 1: actions[0] = indices [N][7])", action_mode);
  MAPPO_REQUIRE(episode_length >= 1, "mpe_world_comm_step: episode length %d, needs >= 1", episode_length);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && tstep && episode && actions && actions[0] && obs && mpe_world_comm_all(obs) &&
                rewards && dones, "mpe_world_comm_step: null pointer");
  MpeWcArgs a = {};
  if (action_mode == 0)
    for (int m = 1; m < MPE_WC_M; ++m) MAPPO_REQUIRE(actions[m], "mpe_world_comm_step: null pointer (actions[%d], action_mode 0)", m);
  a.apos = agent_pos; a.avel = agent_vel; a.lpos = landmark_pos; a.tstep = tstep; a.episode = episode;
  for (int m = 0; m < MPE_WC_M; ++m) { a.act[m] = action_mode == 0 ? actions[m] : (m == 0 ? actions[0] : nullptr); a.obs[m] = obs[m]; }
  a.rewards = rewards; a.dones = dones;
  a.N = N; a.T = episode_length; a.mode = action_mode; a.seed = seed;
  hipLaunchKernelGGL(mpe_world_comm_step_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_world_comm_step");
  return MAPPO_OK;
}
