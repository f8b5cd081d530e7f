// mpe_crypto_env.hip — GPU-vectorised MPE `simple_crypto`: N environments x (Eve, Bob, Alice) x L landmarks stepped by ONE kernel
// launch, one lane per environment.  Reference: onpolicy/envs/mpe/environment.py:194-256 (action decoding: an agent that does not move
// and is not silent speaks its whole action vector), :49-50,142 (world.collaborative is not set: per-agent rewards), :179-185
// (time-limit done); onpolicy/envs/mpe/core.py:280-287 (state.c = action.c, no noise); onpolicy/envs/mpe/scenarios/simple_crypto.py:
// 21-44 (nobody moves or collides, dim_c 4), :47-75 (reset), :94-121 (reward), :124-171 (observation); and the reset-on-done of the
// vec-env wrappers (envs/env_wrappers.py:146-152).
//
// There is no arithmetic to round: every observation is a one-hot or zeros and every reward is -2, 0 or 2, so the outputs EQUAL the
// fp32 cast of the reference's (tests/golden/mpe_crypto.npz).  State is device resident; resets draw from the counter-based Philox
// stream keyed by (seed, episode, index) — index layout in mpe_crypto_core.h.
#include "mpe_crypto_core.h"

__global__ __launch_bounds__(256) void mpe_crypto_reset_kernel(MpeCryptoArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpeCryptoState s;
  s.episode = a.episode[n] + 1;
  s.tstep = 0;
  mpe_crypto_reset_env(a, n, s, s.episode);
  mpe_crypto_store(a, n, s, true);
  mpe_crypto_write_obs(a.obs[0] + (size_t)n * MPE_CRYPTO_OBS_E, a.obs[1] + (size_t)n * MPE_CRYPTO_OBS_B, a.obs[2] + (size_t)n * MPE_CRYPTO_OBS_A, s);
}

__global__ __launch_bounds__(256) void mpe_crypto_step_kernel(MpeCryptoArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  MpeCryptoState s;
  mpe_crypto_load(a, n, s);
  const int stride = a.mode == 0 ? MPE_CRYPTO_C : 1;
  float reward[MPE_CRYPTO_M];
  const bool done = mpe_crypto_step_env(a, n, a.act + (size_t)n * MPE_CRYPTO_M * stride, stride, s, a.obs[0] + (size_t)n * MPE_CRYPTO_OBS_E,
                                        a.obs[1] + (size_t)n * MPE_CRYPTO_OBS_B, a.obs[2] + (size_t)n * MPE_CRYPTO_OBS_A, reward);
#pragma unroll
  for (int m = 0; m < MPE_CRYPTO_M; ++m) {
    a.rewards[(size_t)n * MPE_CRYPTO_M + m] = reward[m];
    a.dones[(size_t)n * MPE_CRYPTO_M + m] = done ? 1 : 0;
  }
  mpe_crypto_store(a, n, s, done);
}

// what both entry points refuse of the scenario's shape
static int mpe_crypto_check_shape(const char *who, int32_t N, int32_t num_agents, int32_t num_landmarks) {
  MAPPO_REQUIRE(num_agents == MPE_CRYPTO_M, "%s: num_agents=%d: simple_crypto is built for num_agents = 3 (adversary Eve, listener Bob, "
                "speaker Alice)", who, num_agents);
  MAPPO_REQUIRE(num_landmarks >= MPE_CRYPTO_MIN_L && num_landmarks <= MPE_CRYPTO_MAX_L, "%s: num_landmarks=%d: simple_crypto takes "
                "num_landmarks = 2, 3 or 4 (a landmark's colour is a one-hot of dim_c = 4)", who, num_landmarks);
  MAPPO_REQUIRE(N >= 1, "%s: N=%d, needs at least one environment (N >= 1)", who, N);
  return MAPPO_OK;
}

extern "C" int mappo_mpe_crypto_reset(int32_t *goal, int32_t *key, int32_t *comm, int32_t *tstep, int64_t *episode, float *obs_eve,
                                      float *obs_bob, float *obs_alice, int32_t N, int32_t num_agents, int32_t num_landmarks,
                                      uint64_t seed, mappo_stream_t stream) {
  if (int rc = mpe_crypto_check_shape("mpe_crypto_reset", N, num_agents, num_landmarks)) return rc;
  MAPPO_REQUIRE(goal && key && comm && tstep && episode && obs_eve && obs_bob && obs_alice, "mpe_crypto_reset: null pointer");
  MpeCryptoArgs a = {};
  a.goal = goal; a.key = key; a.comm = comm; a.tstep = tstep; a.episode = episode;
  a.obs[0] = obs_eve; a.obs[1] = obs_bob; a.obs[2] = obs_alice; a.N = N; a.L = num_landmarks; a.seed = seed;
  hipLaunchKernelGGL(mpe_crypto_reset_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_crypto_reset");
  return MAPPO_OK;
}

extern "C" int mappo_mpe_crypto_step(int32_t *goal, int32_t *key, int32_t *comm, int32_t *tstep, int64_t *episode, const float *actions,
                                     int32_t action_mode, float *obs_eve, float *obs_bob, float *obs_alice, float *rewards, uint8_t *dones,
                                     int32_t N, int32_t num_agents, int32_t num_landmarks, int32_t episode_length, uint64_t seed,
                                     mappo_stream_t stream) {
  if (int rc = mpe_crypto_check_shape("mpe_crypto_step", N, num_agents, num_landmarks)) return rc;
  MAPPO_REQUIRE(action_mode == 0 || action_mode == 1, "mpe_crypto_step: action_mode %d (0: one-hots [N][3][4]; 1: indices [N][3])",
                action_mode);
  MAPPO_REQUIRE(episode_length >= 1, "mpe_crypto_step: episode length %d, needs >= 1", episode_length);
  MAPPO_REQUIRE(goal && key && comm && tstep && episode && actions && obs_eve && obs_bob && obs_alice && rewards && dones,
                "mpe_crypto_step: null pointer");
  MpeCryptoArgs a = {};
  a.goal = goal; a.key = key; a.comm = comm; a.tstep = tstep; a.episode = episode;
  a.act = actions; a.obs[0] = obs_eve; a.obs[1] = obs_bob; a.obs[2] = obs_alice; a.rewards = rewards; a.dones = dones;
  a.N = N; a.T = episode_length; a.mode = action_mode; a.L = num_landmarks; a.seed = seed;
  hipLaunchKernelGGL(mpe_crypto_step_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH("mpe_crypto_step");
  return MAPPO_OK;
}
