// mpe_ragged_env.hip — the stepwise entry points of GPU-vectorised MPE simple_adversary, simple_tag, simple_push and simple_crypto: the
// shared kernels of mpe_ragged_env.h on each scenario's traits.  What a scenario computes, the reference sites it is held against and
// its Philox index layout are in its mpe_*_core.h.  An entry point is the scenario's own: its checks, in their order, and its state
// arrays; `mpe_*_args` fills what reset and step have in common.
#include "mpe_adv_core.h"
#include "mpe_crypto_core.h"
#include "mpe_push_core.h"                                          // includes mpe_tag_core.h
#include "mpe_ragged_env.h"

// ---- simple_adversary ----
static int mpe_adv_check_shape(const char *who, int32_t N, int32_t num_agents) {
  MAPPO_REQUIRE(num_agents == MPE_ADV_M, "%s: num_agents=%d: simple_adversary is built for num_agents = 3 (1 adversary, 2 good agents, 2 "
                "landmarks)", who, num_agents);
  MAPPO_REQUIRE(N >= 1, "%s: N=%d, needs at least one environment (N >= 1)", who, N);
  return MAPPO_OK;
}

static MpeAdvArgs mpe_adv_args(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep, int64_t *episode,
                               float *obs_adversary, float *obs_good1, float *obs_good2, int32_t N, uint64_t seed) {
  MpeAdvArgs a = {};
  a.apos = agent_pos; a.avel = agent_vel; a.lpos = landmark_pos; a.goal = goal; a.tstep = tstep; a.episode = episode;
  a.obs[0] = obs_adversary; a.obs[1] = obs_good1; a.obs[2] = obs_good2; a.N = N; a.seed = seed;
  return a;
}

extern "C" int mappo_mpe_adversary_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                                         int64_t *episode, float *obs_adversary, float *obs_good1, float *obs_good2, int32_t N,
                                         int32_t num_agents, uint64_t seed, mappo_stream_t stream) {
  if (int rc = mpe_adv_check_shape("mpe_adversary_reset", N, num_agents)) return rc;
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode && obs_adversary && obs_good1 && obs_good2,
                "mpe_adversary_reset: null pointer");
  const MpeAdvArgs a = mpe_adv_args(agent_pos, agent_vel, landmark_pos, goal, tstep, episode, obs_adversary, obs_good1, obs_good2, N, seed);
  return mpe_ragged_launch<mpe_ragged_reset_kernel<MpeAdv>>("mpe_adversary_reset", a, stream);
}

extern "C" int mappo_mpe_adversary_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                                        int64_t *episode, const float *actions, int32_t action_mode, float *obs_adversary,
                                        float *obs_good1, float *obs_good2, float *rewards, uint8_t *dones, int32_t N, int32_t num_agents,
                                        int32_t episode_length, uint64_t seed, mappo_stream_t stream) {
  if (int rc = mpe_adv_check_shape("mpe_adversary_step", N, num_agents)) return rc;
  MAPPO_REQUIRE(action_mode == 0 || action_mode == 1, "mpe_adversary_step: action_mode %d (0: one-hots [N][3][5]; 1: indices [N][3])",
                action_mode);
  MAPPO_REQUIRE(episode_length >= 1, "mpe_adversary_step: episode length %d, needs >= 1", episode_length);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode && actions && obs_adversary && obs_good1 && obs_good2 &&
                rewards && dones, "mpe_adversary_step: null pointer");
  MpeAdvArgs a = mpe_adv_args(agent_pos, agent_vel, landmark_pos, goal, tstep, episode, obs_adversary, obs_good1, obs_good2, N, seed);
  a.act = actions; a.rewards = rewards; a.dones = dones; a.T = episode_length; a.mode = action_mode;
  return mpe_ragged_launch<mpe_ragged_step_kernel<MpeAdv>>("mpe_adversary_step", a, stream);
}

// ---- simple_tag ----
static int mpe_tag_check_shape(const char *who, int32_t N, int32_t num_agents) {
  MAPPO_REQUIRE(num_agents == MPE_TAG_M, "%s: num_agents=%d: simple_tag is built for num_agents = 4 (3 adversaries, 1 good agent, 2 "
                "landmarks)", who, num_agents);
  MAPPO_REQUIRE(N >= 1, "%s: N=%d, needs at least one environment (N >= 1)", who, N);
  return MAPPO_OK;
}

static MpeTagArgs mpe_tag_args(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode, float *obs_adv0,
                               float *obs_adv1, float *obs_adv2, float *obs_good, int32_t N, uint64_t seed) {
  MpeTagArgs a = {};
  a.apos = agent_pos; a.avel = agent_vel; a.lpos = landmark_pos; a.tstep = tstep; a.episode = episode;
  a.obs[0] = obs_adv0; a.obs[1] = obs_adv1; a.obs[2] = obs_adv2; a.obs[3] = obs_good; a.N = N; a.seed = seed;
  return a;
}

extern "C" int mappo_mpe_tag_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                                   float *obs_adv0, float *obs_adv1, float *obs_adv2, float *obs_good, int32_t N, int32_t num_agents,
                                   uint64_t seed, mappo_stream_t stream) {
  if (int rc = mpe_tag_check_shape("mpe_tag_reset", N, num_agents)) return rc;
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && tstep && episode && obs_adv0 && obs_adv1 && obs_adv2 && obs_good,
                "mpe_tag_reset: null pointer");
  const MpeTagArgs a = mpe_tag_args(agent_pos, agent_vel, landmark_pos, tstep, episode, obs_adv0, obs_adv1, obs_adv2, obs_good, N, seed);
  return mpe_ragged_launch<mpe_ragged_reset_kernel<MpeTag>>("mpe_tag_reset", a, stream);
}

extern "C" int mappo_mpe_tag_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                                  const float *actions, int32_t action_mode, float *obs_adv0, float *obs_adv1, float *obs_adv2,
                                  float *obs_good, float *rewards, uint8_t *dones, int32_t N, int32_t num_agents, int32_t episode_length,
                                  uint64_t seed, mappo_stream_t stream) {
  if (int rc = mpe_tag_check_shape("mpe_tag_step", N, num_agents)) return rc;
  MAPPO_REQUIRE(action_mode == 0 || action_mode == 1, "mpe_tag_step: action_mode %d (0: one-hots [N][4][5]; 1: indices [N][4])", action_mode);
  MAPPO_REQUIRE(episode_length >= 1, "mpe_tag_step: episode length %d, needs >= 1", episode_length);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && tstep && episode && actions && obs_adv0 && obs_adv1 && obs_adv2 && obs_good &&
                rewards && dones, "mpe_tag_step: null pointer");
  MpeTagArgs a = mpe_tag_args(agent_pos, agent_vel, landmark_pos, tstep, episode, obs_adv0, obs_adv1, obs_adv2, obs_good, N, seed);
  a.act = actions; a.rewards = rewards; a.dones = dones; a.T = episode_length; a.mode = action_mode;
  return mpe_ragged_launch<mpe_ragged_step_kernel<MpeTag>>("mpe_tag_step", a, stream);
}

// ---- simple_push ----
static int mpe_push_check_shape(const char *who, int32_t N, int32_t num_agents) {
  MAPPO_REQUIRE(num_agents == MPE_PUSH_M, "%s: num_agents=%d: simple_push is built for num_agents = 2 (1 adversary, 1 good agent, 2 "
                "landmarks)", who, num_agents);
  MAPPO_REQUIRE(N >= 1, "%s: N=%d, needs at least one environment (N >= 1)", who, N);
  return MAPPO_OK;
}

static MpePushArgs mpe_push_args(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep, int64_t *episode,
                                 float *obs_adversary, float *obs_good, int32_t N, uint64_t seed) {
  MpePushArgs a = {};
  a.apos = agent_pos; a.avel = agent_vel; a.lpos = landmark_pos; a.goal = goal; a.tstep = tstep; a.episode = episode;
  a.obs[0] = obs_adversary; a.obs[1] = obs_good; a.N = N; a.seed = seed;
  return a;
}

extern "C" int mappo_mpe_push_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                                    int64_t *episode, float *obs_adversary, float *obs_good, int32_t N, int32_t num_agents, uint64_t seed,
                                    mappo_stream_t stream) {
  if (int rc = mpe_push_check_shape("mpe_push_reset", N, num_agents)) return rc;
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode && obs_adversary && obs_good, "mpe_push_reset: null pointer");
  const MpePushArgs a = mpe_push_args(agent_pos, agent_vel, landmark_pos, goal, tstep, episode, obs_adversary, obs_good, N, seed);
  return mpe_ragged_launch<mpe_ragged_reset_kernel<MpePush>>("mpe_push_reset", a, stream);
}

extern "C" int mappo_mpe_push_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                                   int64_t *episode, const float *actions, int32_t action_mode, float *obs_adversary, float *obs_good,
                                   float *rewards, uint8_t *dones, int32_t N, int32_t num_agents, int32_t episode_length, uint64_t seed,
                                   mappo_stream_t stream) {
  if (int rc = mpe_push_check_shape("mpe_push_step", N, num_agents)) return rc;
  MAPPO_REQUIRE(action_mode == 0 || action_mode == 1, "mpe_push_step: action_mode %d (0: one-hots [N][2][5]; 1: indices [N][2])", action_mode);
  MAPPO_REQUIRE(episode_length >= 1, "mpe_push_step: episode length %d, needs >= 1", episode_length);
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode && actions && obs_adversary && obs_good && rewards && dones,
                "mpe_push_step: null pointer");
  MpePushArgs a = mpe_push_args(agent_pos, agent_vel, landmark_pos, goal, tstep, episode, obs_adversary, obs_good, N, seed);
  a.act = actions; a.rewards = rewards; a.dones = dones; a.T = episode_length; a.mode = action_mode;
  return mpe_ragged_launch<mpe_ragged_step_kernel<MpePush>>("mpe_push_step", a, stream);
}

// ---- simple_crypto ----
static int mpe_crypto_check_shape(const char *who, int32_t N, int32_t num_agents, int32_t num_landmarks) {
  MAPPO_REQUIRE(num_agents == MPE_CRYPTO_M, "%s: num_agents=%d: simple_crypto is built for num_agents = 3 (adversary Eve, listener Bob, "
                "speaker Alice)", who, num_agents);
  MAPPO_REQUIRE(num_landmarks >= MPE_CRYPTO_MIN_L && num_landmarks <= MPE_CRYPTO_MAX_L, "%s: num_landmarks=%d: simple_crypto takes "
                "num_landmarks = 2, 3 or 4 (a landmark's colour is a one-hot of dim_c = 4)", who, num_landmarks);
  MAPPO_REQUIRE(N >= 1, "%s: N=%d, needs at least one environment (N >= 1)", who, N);
  return MAPPO_OK;
}

static MpeCryptoArgs mpe_crypto_args(int32_t *goal, int32_t *key, int32_t *comm, int32_t *tstep, int64_t *episode, float *obs_eve,
                                     float *obs_bob, float *obs_alice, int32_t N, int32_t num_landmarks, uint64_t seed) {
  MpeCryptoArgs a = {};
  a.goal = goal; a.key = key; a.comm = comm; a.tstep = tstep; a.episode = episode;
  a.obs[0] = obs_eve; a.obs[1] = obs_bob; a.obs[2] = obs_alice; a.N = N; a.L = num_landmarks; a.seed = seed;
  return a;
}

extern "C" int mappo_mpe_crypto_reset(int32_t *goal, int32_t *key, int32_t *comm, int32_t *tstep, int64_t *episode, float *obs_eve,
                                      float *obs_bob, float *obs_alice, int32_t N, int32_t num_agents, int32_t num_landmarks,
                                      uint64_t seed, mappo_stream_t stream) {
  if (int rc = mpe_crypto_check_shape("mpe_crypto_reset", N, num_agents, num_landmarks)) return rc;
  MAPPO_REQUIRE(goal && key && comm && tstep && episode && obs_eve && obs_bob && obs_alice, "mpe_crypto_reset: null pointer");
  const MpeCryptoArgs a = mpe_crypto_args(goal, key, comm, tstep, episode, obs_eve, obs_bob, obs_alice, N, num_landmarks, seed);
  return mpe_ragged_launch<mpe_ragged_reset_kernel<MpeCrypto>>("mpe_crypto_reset", a, stream);
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
  MpeCryptoArgs a = mpe_crypto_args(goal, key, comm, tstep, episode, obs_eve, obs_bob, obs_alice, N, num_landmarks, seed);
  a.act = actions; a.rewards = rewards; a.dones = dones; a.T = episode_length; a.mode = action_mode;
  return mpe_ragged_launch<mpe_ragged_step_kernel<MpeCrypto>>("mpe_crypto_step", a, stream);
}
