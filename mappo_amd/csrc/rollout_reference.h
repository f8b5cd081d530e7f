// rollout_reference.h — one rollout episode on the GPU-resident `simple_reference` environment in ONE launch
// (mappo_rollout_episode_reference): what T x (mappo_rollout_step_md + mappo_mpe_reference_step) + the bootstrap launch do, ~2 T + 1
// dependent launches, for the MultiDiscrete (5, 10) policy of that scenario.
//
// The three-role skeleton of rollout_spread.h (read its header first), with M = 2: a tile is G = 8 whole environments = all 16 rows,
// one workgroup of three waves per tile, two workgroup barriers per step (A_t: the actions of step t are in LDS and every read of
// observation tile t is done; B_t: observation tile t + 1 is in LDS), the same two in every role.  What differs:
//   * wave 0 (actor) runs tile16r_step in MODE 5 with the heads (5, 10): head k of row i draws Philox index (k << 32) | i with
//     counter `counter + t (+ *counter_dev)`, exactly as mappo_rollout_step_md does; actions / logp are [T][B][2], and the row's
//     two actions also go to the LDS action tile [16][2];
//   * wave 2 (environments), lanes 0 .. 7, steps mpe_ref_step_env (mpe_ref_core.h) with mode 1 on that tile.
// No role returns early: a wave whose rows or lanes do not exist (last partial tile) still walks all T steps and their 2 T barriers.
// Every value goes through the stepwise kernels' own code (tile16r_step, mpe_ref_step_env), so the buffer and the environment
// state end up bit-identical to the stepwise path's.
#pragma once
#include "mpe_ref_core.h"
#include "rollout_spread.h"

struct ReferenceEpisodeArgs {
  FwdArgs a, c;                    // a.actions / a.logp: [T][B][2], c.out: [T][B]
  MpeRefArgs env;                  // state arrays, N, T = the ENV's episode length, mode 1, seed
  float *obs_buf, *share_buf;      // [T + 1][B][21], [T + 1][B][S]
  float *rew_buf, *mask_buf;       // [T][B], [T + 1][B]
  float *next_values;              // [B]: the critic at step T
  int T, centralized;              // rollout steps
};

#define REF_EP_G (16 / MPE_REF_M)                                   // environments per tile (workgroup)
#define REF_EP_LDS_FLOATS (SPREAD_X_TILE + 16 * TP + 16 * MPE_REF_K)      // observation tile | logits tile | action tile [16][2]

template <bool RELU, int LN>
__global__ __launch_bounds__(SPREAD_WAVES * WAVE, 1) void rollout_episode_reference_kernel(ReferenceEpisodeArgs e) {
  extern __shared__ __align__(16) float lds[];
  float *X = lds, *tZ = lds + SPREAD_X_TILE, *act = tZ + 16 * TP;
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), j = lane & 15, q = lane >> 4;
  constexpr int M = MPE_REF_M, G = REF_EP_G, D = MPE_REF_OBS;
  const int T = e.T, S = e.c.desc.in_dim;
  const int64_t B = e.a.B;
  const int n0 = (int)blockIdx.x * G;                               // first environment / buffer row of this tile
  const int64_t i0 = (int64_t)n0 * M, i = i0 + j;
  const bool ok = i < B;
  const int jr = ok ? j : 0;
  if (wave == 0) {
    // ---- actor: step 0 reads buffer slot 0, as the stepwise path does; rows requested before the weights (forward16r_body) ----
    f32x4 x[4];
    spread_load_x(x, e.obs_buf + (ok ? i : 0) * D, D, q);
    Trunk16R<LN> tw;
    trunk16r_load<LN>(tw, e.a.params, e.a.off, e.a.desc, j, q);
    Head16R<5> hd;
    head16r_load<5>(hd, e.a.params, e.a.off, e.a.desc.out_dim, j, q);
    const MdHeads md = {MPE_REF_K, {5, MPE_REF_C, 0, 0}};           // the entry point admits no other heads
    const uint64_t ctr0 = e.a.counter + (e.a.counter_dev ? *e.a.counter_dev : 0ull);    // read once: the word is fixed for the launch
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B * MPE_REF_K;
      tile16r_step<RELU, LN, 5, false, true>(e.a, tw, hd, x, nullptr, e.a.actions + so, e.a.logp + so, ctr0 + (uint64_t)t, nullptr, tZ, i, ok,
                                             j, q, act, &md);
      __syncthreads();                                              // A_t
      __syncthreads();                                              // B_t
      spread_load_x(x, X + jr * D, D, q);
    }
  } else if (wave == 1) {
    // ---- critic: steps 0 .. T; the observation tile of step t >= 1 also goes to obs[t] / share_obs[t] from here ----
    f32x4 x[4];
    spread_load_x(x, e.share_buf + (ok ? i : 0) * S, S, q);
    Trunk16R<LN> tw;
    trunk16r_load<LN>(tw, e.c.params, e.c.off, e.c.desc, j, q);
    Head16R<0> hd;
    head16r_load<0>(hd, e.c.params, e.c.off, 1, j, q);
    const int Rv = (int)(B - i0 < 16 ? B - i0 : 16);                // rows of the tile that exist (the last tile may be partial)
    for (int t = 0;; ++t) {
      const int64_t so = (int64_t)t * B;
      if (t >= 1) {         // what insert_mpe writes (centralized: the environment's 2 rows side by side, once per agent)
        float *od = e.obs_buf + (so + i0) * D, *sd = e.share_buf + (so + i0) * S;
        for (int k = lane; k < Rv * D; k += WAVE) od[k] = X[k];
        if (e.centralized) {
          for (int k = lane; k < Rv * S; k += WAVE) { const int row = k / S; sd[k] = X[(row / M) * S + (k - row * S)]; }
        } else {
          for (int k = lane; k < Rv * S; k += WAVE) sd[k] = X[k];
        }
      }
      tile16r_step<RELU, LN, 0>(e.c, tw, hd, x, t == T ? e.next_values : e.c.out + so, nullptr, nullptr, 0ull, nullptr, tZ, i, ok, j, q);
      if (t == T) break;
      __syncthreads();                                              // A_t
      __syncthreads();                                              // B_t
      spread_load_x(x, X + (e.centralized ? (jr / M) * S : jr * D), S, q);
    }
  } else {
    // ---- environments: one lane each, the state stays in the lane for the whole episode ----
    const int n = n0 + lane;
    const bool env_lane = lane < G && n < e.env.N;
    double ap[MPE_REF_M][2] = {}, av[MPE_REF_M][2] = {}, lp[MPE_REF_L][2] = {};
    int g[MPE_REF_M] = {};
    int32_t tstep = 0;
    int64_t episode = 0;
    if (env_lane) {
      mpe_ref_load(e.env, n, ap, av, lp, g);
      tstep = e.env.tstep[n];
      episode = e.env.episode[n];
    }
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B;
      __syncthreads();                                              // A_t
      if (env_lane)         // obs -> the tile (rows 2 lane, 2 lane + 1), rewards -> slot t, masks -> slot t + 1
        mpe_ref_step_env(e.env, n, act + lane * M * MPE_REF_K, ap, av, lp, g, tstep, episode, X + lane * M * D, e.rew_buf + so + (int64_t)n * M,
                         nullptr, e.mask_buf + so + B + (int64_t)n * M);
      __syncthreads();                                              // B_t
    }
    if (env_lane) {         // the environment continues from here in either path
      mpe_ref_store(e.env, n, ap, av, lp, g, true);
      e.env.tstep[n] = tstep;
      e.env.episode[n] = episode;
    }
  }
}

template <bool R, int L>
static int reference_episode_launch(dim3 grid, size_t lds_bytes, hipStream_t st, const ReferenceEpisodeArgs &a) {
  hipLaunchKernelGGL((rollout_episode_reference_kernel<R, L>), grid, dim3(SPREAD_WAVES * WAVE), lds_bytes, st, a);
  return MAPPO_OK;
}

extern "C" int mappo_rollout_episode_reference(const float *actor_params, const mappo_net_desc *actor_desc, const float *critic_params,
                                               const mappo_net_desc *critic_desc, const int32_t *head_dims, int32_t n_heads, int32_t T,
                                               int32_t N, int32_t env_episode_length, uint64_t env_seed, double *agent_pos,
                                               double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep, int64_t *episode,
                                               int32_t deterministic, uint64_t seed, uint64_t counter, const uint64_t *counter_dev,
                                               float *obs_buf, float *share_buf, float *rew_buf, float *mask_buf, float *actions, float *logp,
                                               float *values, float *next_values, int32_t centralized, mappo_stream_t stream) {
  const char *who = "rollout_episode_reference";
  MAPPO_REQUIRE(head_dims, "%s: null head_dims", who);
  MAPPO_REQUIRE(n_heads == MPE_REF_K && head_dims[0] == 5 && head_dims[1] == MPE_REF_C, "%s: %d heads (%d, %d, ..): simple_reference has "
                "exactly the heads (5, %d)", who, n_heads, n_heads >= 1 ? head_dims[0] : 0, n_heads >= 2 ? head_dims[1] : 0, MPE_REF_C);
  MdHeads md;
  if (int rc = check_md(actor_desc, head_dims, n_heads, nullptr, who, md)) return rc;      // layer_N <= 1, not recurrent, in_dim <= 64
  if (int rc = check_desc(critic_desc, who)) return rc;
  MAPPO_REQUIRE(actor_desc->in_dim <= MAXD && critic_desc->in_dim <= MAXD, "%s: in_dim %d / %d: both networks must be narrow (<= %d)", who,
                actor_desc->in_dim, critic_desc->in_dim, MAXD);
  MAPPO_REQUIRE(actor_desc->in_dim == MPE_REF_OBS && actor_desc->out_dim == MPE_REF_A, "%s: actor in_dim %d / out_dim %d: simple_reference has "
                "%d observation features and %d logits", who, actor_desc->in_dim, actor_desc->out_dim, MPE_REF_OBS, MPE_REF_A);
  MAPPO_REQUIRE(actor_desc->layer_N == critic_desc->layer_N && actor_desc->use_relu == critic_desc->use_relu,
                "%s: actor and critic must share layer_N and the activation", who);
  MAPPO_REQUIRE(critic_desc->out_dim == 1, "%s: critic out_dim must be 1", who);
  MAPPO_REQUIRE(T >= 1 && N >= 1 && env_episode_length >= 1, "%s: bad shape T=%d N=%d env episode length %d (each needs >= 1)", who, T, N,
                env_episode_length);
  if (centralized)
    MAPPO_REQUIRE(critic_desc->in_dim == MPE_REF_M * MPE_REF_OBS, "%s: centralized critic needs in_dim 2 * 21 = %d (got %d)", who,
                  MPE_REF_M * MPE_REF_OBS, critic_desc->in_dim);
  else
    MAPPO_REQUIRE(critic_desc->in_dim == MPE_REF_OBS, "%s: critic in_dim %d != actor in_dim %d", who, critic_desc->in_dim, MPE_REF_OBS);
  MAPPO_REQUIRE(actor_params && critic_params && agent_pos && agent_vel && landmark_pos && goal && tstep && episode && obs_buf && share_buf &&
                rew_buf && mask_buf && actions && logp && values && next_values, "%s: bad arguments (null pointer)", who);
  MAPPO_CLEAR_STICKY();
  ReferenceEpisodeArgs e = {};
  const int64_t B = (int64_t)N * MPE_REF_M;
  e.a.params = actor_params; e.a.actions = actions; e.a.logp = logp; e.a.desc = *actor_desc; e.a.B = B; e.a.deterministic = deterministic;
  e.a.seed = seed; e.a.counter = counter; e.a.counter_dev = counter_dev; e.a.off = net_offsets(e.a.desc);
  e.c.params = critic_params; e.c.out = values; e.c.desc = *critic_desc; e.c.B = B; e.c.off = net_offsets(e.c.desc);
  e.env.apos = agent_pos; e.env.avel = agent_vel; e.env.lpos = landmark_pos; e.env.goal = goal; e.env.tstep = tstep; e.env.episode = episode;
  e.env.N = N; e.env.T = env_episode_length; e.env.mode = 1; e.env.seed = env_seed;
  e.obs_buf = obs_buf; e.share_buf = share_buf; e.rew_buf = rew_buf; e.mask_buf = mask_buf; e.next_values = next_values;
  e.T = T; e.centralized = centralized;
  const dim3 grid((unsigned)((N + REF_EP_G - 1) / REF_EP_G));
  const size_t lds_bytes = sizeof(float) * REF_EP_LDS_FLOATS;
  const bool relu = actor_desc->use_relu != 0;
  int rc;
  if (actor_desc->layer_N == 0) rc = relu ? reference_episode_launch<true, 0>(grid, lds_bytes, as_stream(stream), e) : reference_episode_launch<false, 0>(grid, lds_bytes, as_stream(stream), e);
  else rc = relu ? reference_episode_launch<true, 1>(grid, lds_bytes, as_stream(stream), e) : reference_episode_launch<false, 1>(grid, lds_bytes, as_stream(stream), e);
  if (rc) return rc;
  MAPPO_CHECK_LAUNCH("rollout_episode_reference");
  return MAPPO_OK;
}
