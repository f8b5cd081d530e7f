// rollout_crypto.h — one rollout episode on the GPU-resident `simple_crypto` environment in ONE launch (mappo_rollout_episode_crypto),
// for the SEPARATED runner: three agents (Eve 4 features, Bob and Alice 8 each, Discrete(4) each), each with its own actor, critic,
// per-agent reward and SeparatedReplayBuffer.  It does what T x (three mappo_rollout_step + mappo_mpe_crypto_step + the three agents'
// inserts) + the three bootstrap launches do, ~7 T + 3 dependent launches — here for an environment step that is a handful of integer
// compares, so the stepwise rollout is launch latency and nothing else.
//
// The role skeleton of rollout_adversary.h, unchanged (read its header, and rollout_comm.h's, first): a tile is 16 whole environments,
// one workgroup of FOUR waves per tile, one per SIMD, one row per environment and agent.
//   wave m = 0, 1, 2   agent m.  Its ACTOR has its weights in registers (Trunk16R / Head16R<1>): tile16r_step MODE 1 on the agent's
//           slice of the observation tile, Philox (seed_m, counter + t (+ *counter_dev_m), row = environment), the sampled symbol also
//           to the action tile.  Its CRITIC reads its weights from an LDS image (Trunk16L / Head16L of mlp_ep16l.h) and runs between
//           the step's two barriers, beside the environment step; step T writes next_values.
//   wave 3             the environments, lanes 0 .. 15: mpe_crypto_step_env (mpe_crypto_core.h) with mode 1 between the two barriers,
//           the state in the lane for the whole episode; each agent's OWN reward -> its rew_buf[t], 1 - done -> its mask_buf[t + 1].
//           Behind B_t the whole wave copies observation tile t + 1 into the three agents' obs[t + 1] / share_obs[t + 1] (what the
//           stepwise insert writes), beside the actors of step t + 1.
// and the same two workgroup barriers per step in every role (A_t: the actions of step t are in LDS and every read of observation
// tile t is in registers; B_t: observation tile t + 1 is in LDS), behind one barrier that closes the staging of the critic images,
// in which all four waves take part.  No role returns early: a wave whose rows or lanes do not exist (last partial tile) still
// walks all T steps and their barriers.
//
// What is narrow here: Eve's actor has in_dim 4, exactly one f32x4 of quarter q = 0 in block b = 0 — spread_load_x clamps every
// other slot's index to 3, inside the row, and trunk16r_apply zeroes the slots beyond in_dim before their first use; and every head
// has 4 logits, one quarter of head block 0 (the clamped repeat rows of Head16R fill the rest, as for the 3 logits of the speaker in
// rollout_comm.h).
//
// LDS (floats): three critic images, EplMap<LN>::total each (11424 at layer_N 1, 6880 at 0) | the observation tile [16][20] — a row
// is Eve's 4 features, then Bob's 8 and Alice's 8: the centralized share row as it stands, each network reads its slice | one
// [16][TP] logits tile per actor wave | the action tile, one column of 16 per agent.  At layer_N 1 that is
// 3 x 11424 + 320 + 3 x 528 + 48 = 36224 floats = 144 896 B (141.5 KB) of the 160 KB of a CU, at layer_N 0 22592 floats = 90 368 B:
// one workgroup per CU, which the grid (N / 16 workgroups) does not exceed before N = 4096 on 256 CUs.
// Every value goes through the stepwise kernels' own code (tile16r_step, mpe_crypto_step_env), so the three buffers and the
// environment state end up bit-identical to the stepwise path's.
#pragma once
#include "mpe_crypto_core.h"
#include "rollout_comm.h"

typedef SepEpisodeArgs<MpeCryptoArgs, MPE_CRYPTO_M> CryptoEpisodeArgs;   // agent 0: Eve, 1: Bob, 2: Alice

#define CRYPTO_EP_G 16                                              // environments per tile (workgroup)
#define CRYPTO_EP_WAVES 4
#define CRYPTO_X_TILE (16 * MPE_CRYPTO_SHARE)
template <int LN>
constexpr int crypto_ep_lds_floats() { return MPE_CRYPTO_M * EplMap<LN>::total + CRYPTO_X_TILE + MPE_CRYPTO_M * 16 * TP + MPE_CRYPTO_M * 16; }
static_assert(sizeof(float) * crypto_ep_lds_floats<1>() <= 160 * 1024, "the episode's LDS must fit one CU");
static_assert(MPE_CRYPTO_M < CRYPTO_EP_WAVES && CRYPTO_EP_G <= WAVE, "one wave per agent, one wave whose lanes step the tile's environments");

template <bool RELU, int LN>
__global__ __launch_bounds__(CRYPTO_EP_WAVES * WAVE, 1) void rollout_episode_crypto_kernel(CryptoEpisodeArgs e) {
  extern __shared__ __align__(16) float lds[];
  constexpr int IMG = EplMap<LN>::total, W = MPE_CRYPTO_SHARE;
  float *X = lds + MPE_CRYPTO_M * IMG, *tZ = X + CRYPTO_X_TILE, *act = tZ + MPE_CRYPTO_M * 16 * TP;
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), j = lane & 15, q = lane >> 4;
  const int T = e.T;
  const int64_t B = e.env.N;                                        // rows of every buffer: one per environment
  const int n0 = (int)blockIdx.x * CRYPTO_EP_G;                     // first environment / buffer row of this tile
  const int64_t i = (int64_t)n0 + j;
  const bool ok = i < B;
  const int jr = ok ? j : 0;
  if (wave < MPE_CRYPTO_M) {
    // ---- agent m: actor (registers) and critic (LDS image); step 0 reads buffer slot 0, as the stepwise path does ----
    const int m = wave;
    const int D = mpe_crypto_obs_dim(m), xo = mpe_crypto_obs_off(m);
    FwdArgs fa, fc;
    comm_fwd_args(fa, e.a[m], B, e.deterministic);
    comm_fwd_args(fc, e.c[m], B, 0);
    const int S = fc.desc.in_dim, so_x = e.centralized ? 0 : xo;    // 20 (centralized) or D
    f32x4 xa[4], xc[4];
    spread_load_x(xa, e.obs_buf[m] + (ok ? i : 0) * D, D, q);
    spread_load_x(xc, e.share_buf[m] + (ok ? i : 0) * S, S, q);
    Trunk16R<LN> tw;
    trunk16r_load<LN>(tw, fa.params, fa.off, fa.desc, j, q);
    Head16R<1> hd;
    head16r_load<1>(hd, fa.params, fa.off, fa.desc.out_dim, j, q);
    const uint64_t ctr0 = e.counter + (e.a[m].counter_dev ? *e.a[m].counter_dev : 0ull);      // read once: the word is fixed for the launch
#pragma unroll
    for (int k = 0; k < MPE_CRYPTO_M; ++k) epl_stage<LN, 1>(lds + k * IMG, e.c[k].params, e.c[k].off, e.c[k].desc);
    __syncthreads();                                                // the critic images are staged
    const float *img = lds + m * IMG;
    const Trunk16L<LN> cw = {img + j * EPL_WS + 4 * q, img + 4 * q};
    const Head16L<LN, 0> ch = {cw.m, cw.v};
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B;
      tile16r_step<RELU, LN, 1, false, true>(fa, tw, hd, xa, nullptr, fa.actions + so, fa.logp + so, ctr0 + (uint64_t)t, nullptr,
                                             tZ + m * 16 * TP, i, ok, j, q, act + m * 16);
      __syncthreads();                                              // A_t
      asm volatile("" ::: "memory");        // the image is loop-invariant: keep its reads inside the step (hoisted, they are a second register network)
      tile16r_step<RELU, LN, 0>(fc, cw, ch, xc, fc.out + so, nullptr, nullptr, 0ull, nullptr, tZ + m * 16 * TP, i, ok, j, q);
      __syncthreads();                                              // B_t
      spread_load_x(xa, X + jr * W + xo, D, q);
      spread_load_x(xc, X + jr * W + so_x, S, q);
    }
    asm volatile("" ::: "memory");
    tile16r_step<RELU, LN, 0>(fc, cw, ch, xc, e.next_values[m], nullptr, nullptr, 0ull, nullptr, tZ + m * 16 * TP, i, ok, j, q);
  } else {
    // ---- the environments, one lane each, the state stays in the lane for the whole episode; the buffer's observation rows ----
    const int n = n0 + lane;
    const bool env_lane = lane < CRYPTO_EP_G && n < e.env.N;
    const int Rv = (int)(B - n0 < 16 ? B - n0 : 16);                // rows of the tile that exist (the last tile may be partial)
    MpeCryptoState s = {};
    if (env_lane) mpe_crypto_load(e.env, n, s);
#pragma unroll
    for (int k = 0; k < MPE_CRYPTO_M; ++k) epl_stage<LN, 1>(lds + k * IMG, e.c[k].params, e.c[k].off, e.c[k].desc);
    __syncthreads();                                                // the critic images are staged
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B;
      __syncthreads();                                              // A_t
      if (env_lane) {       // obs -> the tile's row, each agent's own reward -> slot t, masks -> slot t + 1 of its buffer
        float reward[MPE_CRYPTO_M];
        float *row = X + lane * W;
        const bool done = mpe_crypto_step_env(e.env, n, act + lane, 16, s, row, row + mpe_crypto_obs_off(1), row + mpe_crypto_obs_off(2), reward);
#pragma unroll
        for (int k = 0; k < MPE_CRYPTO_M; ++k) {
          e.rew_buf[k][so + n] = reward[k];
          e.mask_buf[k][so + B + n] = done ? 0.f : 1.f;
        }
      }
      __syncthreads();                                              // B_t
      // what the stepwise inserts write into slot t + 1 (centralized: the tile's row as it stands); the next write of the tile is this
      // wave's own, behind A_{t + 1}
#pragma unroll
      for (int m = 0; m < MPE_CRYPTO_M; ++m) {
        const int D = mpe_crypto_obs_dim(m), xo = mpe_crypto_obs_off(m);
        float *od = e.obs_buf[m] + (so + B + n0) * D;
        for (int k = lane; k < Rv * D; k += WAVE) { const int r = k / D; od[k] = X[r * W + xo + (k - r * D)]; }
        if (e.centralized) {
          float *sd = e.share_buf[m] + (so + B + n0) * W;
          for (int k = lane; k < Rv * W; k += WAVE) sd[k] = X[k];
        } else {
          float *sd = e.share_buf[m] + (so + B + n0) * D;
          for (int k = lane; k < Rv * D; k += WAVE) { const int r = k / D; sd[k] = X[r * W + xo + (k - r * D)]; }
        }
      }
    }
    if (env_lane) mpe_crypto_store(e.env, n, s, true);              // the environment continues from here in either path
  }
}

extern "C" int mappo_rollout_episode_crypto(const mappo_comm_agent *agents, int32_t *goal, int32_t *key, int32_t *comm, int32_t *tstep,
                                            int64_t *episode, int32_t T, int32_t N, int32_t num_landmarks, int32_t env_episode_length,
                                            uint64_t env_seed, int32_t deterministic, uint64_t counter, int32_t centralized,
                                            mappo_stream_t stream) {
  const char *who = "rollout_episode_crypto";
  MAPPO_REQUIRE(agents, "%s: null agent descriptors (needs num_agents = 3 of them: Eve, Bob, Alice)", who);
  MAPPO_REQUIRE(num_landmarks >= MPE_CRYPTO_MIN_L && num_landmarks <= MPE_CRYPTO_MAX_L, "%s: num_landmarks=%d: simple_crypto takes "
                "num_landmarks = 2, 3 or 4 (a landmark's colour is a one-hot of dim_c = 4)", who, num_landmarks);
  const char *const name[MPE_CRYPTO_M] = {"Eve", "Bob", "Alice"};
  const int Dm[MPE_CRYPTO_M] = {MPE_CRYPTO_OBS_E, MPE_CRYPTO_OBS_B, MPE_CRYPTO_OBS_A}, Am[MPE_CRYPTO_M] = {MPE_CRYPTO_C, MPE_CRYPTO_C, MPE_CRYPTO_C};
  CryptoEpisodeArgs e;
  if (int rc = sep_episode_fill(e, who, agents, name, Dm, Am, MPE_CRYPTO_SHARE, centralized, deterministic, counter, T, N, env_episode_length)) return rc;
  MAPPO_REQUIRE(goal && key && comm && tstep && episode, "%s: bad arguments (null state pointer)", who);
  MAPPO_CLEAR_STICKY();
  e.env.goal = goal; e.env.key = key; e.env.comm = comm; e.env.tstep = tstep; e.env.episode = episode;
  e.env.N = N; e.env.T = env_episode_length; e.env.mode = 1; e.env.L = num_landmarks; e.env.seed = env_seed;
  const dim3 grid((unsigned)((N + CRYPTO_EP_G - 1) / CRYPTO_EP_G));
  if (int rc = dispatch_relu_ln<1>(agents[0].actor_desc.use_relu != 0, agents[0].actor_desc.layer_N, [&](auto R, auto L) {
        constexpr int lds_bytes = sizeof(float) * crypto_ep_lds_floats<L.value>();
        return launch_kernel<rollout_episode_crypto_kernel<R.value, L.value>, lds_bytes>(who, grid, dim3(CRYPTO_EP_WAVES * WAVE), lds_bytes, as_stream(stream), e);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}
