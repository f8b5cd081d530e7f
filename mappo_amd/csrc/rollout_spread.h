// rollout_spread.h — one rollout episode on the GPU-resident `simple_spread` environment in ONE launch (mappo_rollout_episode_spread):
// actor forward + sampling, the environment step, the buffer writes and the critic forward of every step, T steps and the bootstrap
// values.  The stepwise path is T x (mappo_rollout_step + mappo_mpe_spread_step) + the bootstrap launch, ~2 T + 1 dependent launches
// that each reload the weights.
//
// Environments never interact, the centralized critic's row needs only the M agents of one environment, sampling is keyed by
// (seed, counter + t, row) and tile16r_step computes a row independently of the tile that holds it — so a workgroup that owns
// whole environments walks all T steps by itself, with no communication between workgroups:
//   * a tile is G = floor(16 / M) whole environments = G M consecutive buffer rows (15 of 16 rows at M = 3), one workgroup of
//     three waves per tile, each wave with a role and a loop of its own (so the kernel's registers are the largest role's, not
//     the sum: the actor's weights and the environments' float64 state never live in the same wave);
//   * wave 0 (actor): tile16r_step in actor mode on the step's observation rows; the sampled actions also go to an LDS tile;
//   * wave 2 (environments): lanes 0 .. G - 1 step one environment each (mpe_step_env, float64, state in the lane for the whole
//     episode) on those actions and write the next observation tile into LDS, rewards[t] and masks[t + 1] into the buffer;
//   * wave 1 (critic): copies the step's observation tile from LDS into obs[t] / share_obs[t] (coalesced; t >= 1), then
//     tile16r_step in critic mode on the share rows; step T writes next_values.  The critic of step t runs beside the actor of
//     step t, off the critical path (actor -> environment -> actor);
//   * two workgroup barriers per step, the same two in every role: A_t (actions of step t are in LDS; every read of observation
//     tile t is done) and B_t (observation tile t + 1 is in LDS).
// Weights are loaded once per wave (registers, as in the other tile16r kernels).  Every value goes through the stepwise kernels'
// own code (tile16r_step, mpe_step_env), so the buffer and the environment state end up bit-identical to the stepwise path's.
#pragma once
#include "mpe_core.h"

struct SpreadEpisodeArgs {
  FwdArgs a, c;                    // a.actions / a.logp, c.out: [T][B]
  MpeArgs env;                     // state arrays, N, M, L, T = the ENV's episode length, mode 1, seed
  float *obs_buf, *share_buf;      // [T + 1][B][D], [T + 1][B][S]
  float *rew_buf, *mask_buf;       // [T][B], [T + 1][B]
  float *next_values;              // [B]: the critic at step T
  int T, G, centralized;           // rollout steps, environments per tile (workgroup)
};

#define SPREAD_X_TILE (16 * MAXD)                                   // floats of the observation tile
#define SPREAD_LDS_FLOATS (SPREAD_X_TILE + 16 * TP + 16)            // observation tile | logits tile | action tile
#define SPREAD_WAVES 3

// lane (j, q)'s inputs of tile row j from the observation tile in LDS (rows beyond the tile: row 0, zeroed by trunk16r_apply)
__device__ __forceinline__ void spread_load_x(f32x4 (&x)[4], const float *base, int Dn, int q) {
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) x[b][r] = base[min(16 * b + 4 * q + r, Dn - 1)];
}

template <bool RELU, int LN>
__global__ __launch_bounds__(SPREAD_WAVES * WAVE, 1) void rollout_episode_spread_kernel(SpreadEpisodeArgs e) {
  extern __shared__ __align__(16) float lds[];
  float *X = lds, *tZ = lds + SPREAD_X_TILE, *act = tZ + 16 * TP;
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), j = lane & 15, q = lane >> 4;
  const int M = e.env.M, G = e.G, R = G * M, T = e.T;
  const int D = e.a.desc.in_dim, S = e.c.desc.in_dim;
  const int64_t B = e.a.B;
  const int n0 = (int)blockIdx.x * G;                               // first environment / buffer row of this tile
  const int64_t i0 = (int64_t)n0 * M, i = i0 + j;
  const bool ok = j < R && i < B;
  const int jr = ok ? j : 0;
  if (wave == 0) {
    // ---- actor: step 0 reads buffer slot 0, as the stepwise path does; rows requested before the weights (forward16r_body) ----
    f32x4 x[4];
    spread_load_x(x, e.obs_buf + (ok ? i : 0) * D, D, q);
    Trunk16R<LN> tw;
    trunk16r_load<LN>(tw, e.a.params, e.a.off, e.a.desc, j, q);
    Head16R<1> hd;
    head16r_load<1>(hd, e.a.params, e.a.off, e.a.desc.out_dim, j, q);
    const uint64_t ctr0 = e.a.counter + (e.a.counter_dev ? *e.a.counter_dev : 0ull);    // read once: the word is fixed for the launch
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B;
      tile16r_step<RELU, LN, 1, false, true>(e.a, tw, hd, x, nullptr, e.a.actions + so, e.a.logp + so, ctr0 + (uint64_t)t, nullptr, tZ, i, ok,
                                             j, q, act);
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
    const int Rv = (int)(B - i0 < R ? B - i0 : R);                  // rows of the tile that exist (the last tile may be partial)
    for (int t = 0;; ++t) {
      const int64_t so = (int64_t)t * B;
      if (t >= 1) {         // what insert_mpe writes (centralized: the environment's M rows side by side, once per agent)
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
    double ap[MPE_MAX_M][2], av[MPE_MAX_M][2], lp[MPE_MAX_L][2];
    int32_t tstep = 0;
    int64_t episode = 0;
    if (env_lane) {
      mpe_load(e.env, n, ap, av, lp);
      tstep = e.env.tstep[n];
      episode = e.env.episode[n];
    }
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B;
      __syncthreads();                                              // A_t
      if (env_lane)         // obs -> the tile (rows lane M ..), rewards -> slot t, masks -> slot t + 1
        mpe_step_env(e.env, n, act + lane * M, ap, av, lp, tstep, episode, X + lane * M * D, e.rew_buf + so + (int64_t)n * M, nullptr,
                     e.mask_buf + so + B + (int64_t)n * M);
      __syncthreads();                                              // B_t
    }
    if (env_lane) {         // the environment continues from here in either path
      mpe_store(e.env, n, ap, av, lp, true);
      e.env.tstep[n] = tstep;
      e.env.episode[n] = episode;
    }
  }
}

template <bool R, int L>
static int spread_episode_launch(dim3 grid, size_t lds_bytes, hipStream_t st, const SpreadEpisodeArgs &a) {
  hipLaunchKernelGGL((rollout_episode_spread_kernel<R, L>), grid, dim3(SPREAD_WAVES * WAVE), lds_bytes, st, a);
  return MAPPO_OK;
}

extern "C" int mappo_rollout_episode_spread(const float *actor_params, const mappo_net_desc *actor_desc, const float *critic_params,
                                            const mappo_net_desc *critic_desc, int32_t T, int32_t N, int32_t M, int32_t L,
                                            int32_t env_episode_length, uint64_t env_seed, double *agent_pos, double *agent_vel,
                                            double *landmark_pos, int32_t *tstep, int64_t *episode, int32_t deterministic, uint64_t seed,
                                            uint64_t counter, const uint64_t *counter_dev, float *obs_buf, float *share_buf, float *rew_buf,
                                            float *mask_buf, float *actions, float *logp, float *values, float *next_values,
                                            int32_t centralized, mappo_stream_t stream) {
  const char *who = "rollout_episode_spread";
  if (int rc = check_desc(actor_desc, who)) return rc;
  if (int rc = check_desc(critic_desc, who)) return rc;
  MAPPO_REQUIRE(actor_desc->in_dim <= MAXD && critic_desc->in_dim <= MAXD, "%s: in_dim %d / %d: both networks must be narrow (<= %d)", who,
                actor_desc->in_dim, critic_desc->in_dim, MAXD);
  MAPPO_REQUIRE(actor_desc->layer_N == critic_desc->layer_N && actor_desc->use_relu == critic_desc->use_relu,
                "%s: actor and critic must share layer_N and the activation", who);
  MAPPO_REQUIRE(critic_desc->out_dim == 1, "%s: critic out_dim must be 1", who);
  MAPPO_REQUIRE(T >= 1 && N >= 1 && env_episode_length >= 1, "%s: bad shape T=%d N=%d env episode length %d", who, T, N, env_episode_length);
  MAPPO_REQUIRE(M >= 1 && M <= MPE_MAX_M && L >= 1 && L <= MPE_MAX_L, "%s: M=%d L=%d out of range (1 .. %d)", who, M, L, MPE_MAX_M);
  const int D = 4 + 2 * L + 4 * (M - 1);
  MAPPO_REQUIRE(actor_desc->in_dim == D && actor_desc->out_dim == 5, "%s: actor in_dim %d / out_dim %d: simple_spread with M=%d L=%d has "
                "%d observation features and 5 actions", who, actor_desc->in_dim, actor_desc->out_dim, M, L, D);
  if (centralized)
    MAPPO_REQUIRE(critic_desc->in_dim == M * D, "%s: centralized critic needs in_dim M*D = %d (got %d)", who, M * D, critic_desc->in_dim);
  else
    MAPPO_REQUIRE(critic_desc->in_dim == D, "%s: critic in_dim %d != actor in_dim %d", who, critic_desc->in_dim, D);
  MAPPO_REQUIRE(actor_params && critic_params && agent_pos && agent_vel && landmark_pos && tstep && episode && obs_buf && share_buf && rew_buf &&
                mask_buf && actions && logp && values && next_values, "%s: bad arguments (null pointer)", who);
  MAPPO_CLEAR_STICKY();
  SpreadEpisodeArgs e = {};
  const int64_t B = (int64_t)N * M;
  e.a.params = actor_params; e.a.actions = actions; e.a.logp = logp; e.a.desc = *actor_desc; e.a.B = B; e.a.deterministic = deterministic;
  e.a.seed = seed; e.a.counter = counter; e.a.counter_dev = counter_dev; e.a.off = net_offsets(e.a.desc);
  e.c.params = critic_params; e.c.out = values; e.c.desc = *critic_desc; e.c.B = B; e.c.off = net_offsets(e.c.desc);
  e.env.apos = agent_pos; e.env.avel = agent_vel; e.env.lpos = landmark_pos; e.env.tstep = tstep; e.env.episode = episode;
  e.env.N = N; e.env.M = M; e.env.L = L; e.env.T = env_episode_length; e.env.mode = 1; e.env.seed = env_seed;
  e.obs_buf = obs_buf; e.share_buf = share_buf; e.rew_buf = rew_buf; e.mask_buf = mask_buf; e.next_values = next_values;
  e.T = T; e.G = 16 / M; e.centralized = centralized;
  const dim3 grid((unsigned)((N + e.G - 1) / e.G));
  const size_t lds_bytes = sizeof(float) * SPREAD_LDS_FLOATS;
  const bool relu = actor_desc->use_relu != 0;
  int rc;
  switch (actor_desc->layer_N) {
    case 0: rc = relu ? spread_episode_launch<true, 0>(grid, lds_bytes, as_stream(stream), e) : spread_episode_launch<false, 0>(grid, lds_bytes, as_stream(stream), e); break;
    case 1: rc = relu ? spread_episode_launch<true, 1>(grid, lds_bytes, as_stream(stream), e) : spread_episode_launch<false, 1>(grid, lds_bytes, as_stream(stream), e); break;
    default: rc = relu ? spread_episode_launch<true, 2>(grid, lds_bytes, as_stream(stream), e) : spread_episode_launch<false, 2>(grid, lds_bytes, as_stream(stream), e); break;
  }
  if (rc) return rc;
  MAPPO_CHECK_LAUNCH("rollout_episode_spread");
  return MAPPO_OK;
}
