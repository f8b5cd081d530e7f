// rollout_sep_img.h — one rollout episode on a GPU-resident MPE environment of M = 3 agents in ONE launch, for the SEPARATED runner:
// each agent with its own actor, critic, per-agent reward and SeparatedReplayBuffer.  Two scenarios take this placement, through
// their traits Env (mpe_*_core.h):
//   simple_adversary (mappo_rollout_episode_adversary)   the adversary with 8 features, two good agents with 10 each, Discrete(5)
//   simple_crypto    (mappo_rollout_episode_crypto)      Eve with 4 features, Bob and Alice with 8 each, Discrete(4) — an environment
//           step that is a handful of integer compares, so the stepwise rollout is launch latency and nothing else
// It does what T x (three mappo_rollout_step + the environment's stepwise step + the three agents' inserts) + the three bootstrap
// launches do, ~7 T + 3 dependent launches.
//
// The role skeleton of rollout_comm.h (read its header first): a tile is 16 whole environments, one workgroup of FOUR waves per
// tile, one per SIMD, one row per environment and agent.  Six networks do not fit that kernel's plan of one network per wave in
// registers: at layer_N 1 a network is ~290 VGPRs (mlp_ep16l.h), so six waves would put two on a SIMD, halve every wave's register
// budget to 256 and spill; and six networks in the padded LDS image of mlp_ep16l.h are 6 x 45.7 KB = 274 KB against 160 KB per
// CU.  So the agents are split by wave and the two networks of an agent by where their weights live ("actor in registers, critic in
// an LDS image, fourth wave steps the envs"):
//   wave m = 0, 1, 2   agent m.  Its ACTOR has its weights in registers (Trunk16R / Head16R<1>) — it is the step's critical path
//           (actor -> environment -> actor): tile16r_step MODE 1 on the agent's slice of the observation tile, Philox (seed_m,
//           counter + t (+ *counter_dev_m), row = environment), the sampled action also to the action tile.  Its CRITIC reads its
//           weights from an LDS image (Trunk16L / Head16L of mlp_ep16l.h: the same 16-byte operands in the same order, so the same
//           bits) and runs between the step's two barriers, beside the environment step; step T writes next_values.
//   wave 3             the environments, lanes 0 .. 15: Env::step_env with mode 1 between the two barriers (sep_env_step), the state in
//           the lane for the whole episode; each agent's OWN reward -> its rew_buf[t], 1 - done -> its mask_buf[t + 1].  Behind B_t
//           the whole wave copies observation tile t + 1 into the three agents' obs[t + 1] / share_obs[t + 1] (sep_copy_rows: what
//           the stepwise insert writes), beside the actors of step t + 1; the next write of the tile is this wave's own, behind
//           A_{t + 1}.
// and the same two workgroup barriers per step in every role (A_t: the actions of step t are in LDS and every read of observation
// tile t is in registers; B_t: observation tile t + 1 is in LDS), behind one barrier that closes the staging of the critic images,
// in which all four waves take part.  No role returns early: a wave whose rows or lanes do not exist (last partial tile) still
// walks all T steps and their barriers.  An environment's three agents see the same environment step because the step sits behind
// A_t, which all three actors of the tile have passed.
//
// What is narrow in simple_crypto: Eve's actor has in_dim 4, exactly one f32x4 of quarter q = 0 in block b = 0 — spread_load_x clamps
// every other slot's index to 3, inside the row, and trunk16r_apply zeroes the slots beyond in_dim before their first use; and every
// head has 4 logits, one quarter of head block 0 (the clamped repeat rows of Head16R fill the rest, as for the 3 logits of the
// speaker in rollout_comm.h).
//
// LDS (floats): M critic images, EplMap<LN>::total each (11424 at layer_N 1, 6880 at 0) | the observation tile [16][Env::SHARE] — a
// row is the agents' observations side by side: the centralized share row as it stands, each network reads its slice | one [16][TP]
// logits tile per actor wave | the action tile, one column of 16 per agent.  At layer_N 1 that is
//   simple_adversary   3 x 11424 + 16 x 28 + 3 x 528 + 48 = 36352 floats = 145 408 B (142 KB)
//   simple_crypto      3 x 11424 + 16 x 20 + 3 x 528 + 48 = 36224 floats = 144 896 B (141.5 KB); at layer_N 0 22592 floats = 90 368 B
// of the 160 KB of a CU: one workgroup per CU, which the grid (N / 16 workgroups) does not exceed before N = 4096 on 256 CUs.
// Every value goes through the stepwise kernels' own code (tile16r_step, Env::step_env), so the three buffers and the environment
// state end up bit-identical to the stepwise path's.
#pragma once
#include "mpe_adv_core.h"
#include "mpe_crypto_core.h"
#include "rollout_comm.h"

template <class Env, int LN>
constexpr int sep_img_lds_floats() { return Env::M * EplMap<LN>::total + 16 * Env::SHARE + Env::M * 16 * TP + Env::M * 16; }

template <class Env, bool RELU, int LN>
__global__ __launch_bounds__(SEP_EP_WAVES * WAVE, 1) void rollout_episode_sep_img_kernel(SepEpisodeArgs<typename Env::Args, Env::M> e) {
  static_assert(sizeof(float) * sep_img_lds_floats<Env, 1>() <= LDS_LIMIT, "the episode's LDS must fit one CU");
  static_assert(Env::M < SEP_EP_WAVES && SEP_EP_G <= WAVE, "one wave per agent, one wave whose lanes step the tile's environments");
  extern __shared__ __align__(16) float lds[];
  constexpr int M = Env::M, IMG = EplMap<LN>::total, W = Env::SHARE;
  float *X = lds + M * IMG, *tZ = X + 16 * W, *act = tZ + M * 16 * TP;
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), j = lane & 15, q = lane >> 4;
  const int T = e.T;
  const int64_t B = e.env.N;                                        // rows of every buffer: one per environment
  const int n0 = (int)blockIdx.x * SEP_EP_G;                        // first environment / buffer row of this tile
  const int64_t i = (int64_t)n0 + j;
  const bool ok = i < B;
  const int jr = ok ? j : 0;
  if (wave < M) {
    // ---- agent m: actor (registers) and critic (LDS image); step 0 reads buffer slot 0, as the stepwise path does ----
    const int m = wave;
    const int D = Env::obs_dim(m), xo = Env::obs_off(m);
    FwdArgs fa, fc;
    comm_fwd_args(fa, e.a[m], B, e.deterministic);
    comm_fwd_args(fc, e.c[m], B, 0);
    const int S = fc.desc.in_dim, so_x = e.centralized ? 0 : xo;    // W (centralized) or D
    f32x4 xa[4], xc[4];
    spread_load_x(xa, e.obs_buf[m] + (ok ? i : 0) * D, D, q);
    spread_load_x(xc, e.share_buf[m] + (ok ? i : 0) * S, S, q);
    Trunk16R<LN> tw;
    trunk16r_load<LN>(tw, fa.params, fa.off, fa.desc, j, q);
    Head16R<1> hd;
    head16r_load<1>(hd, fa.params, fa.off, fa.desc.out_dim, j, q);
    const uint64_t ctr0 = e.counter + (e.a[m].counter_dev ? *e.a[m].counter_dev : 0ull);      // read once: the word is fixed for the launch
#pragma unroll
    for (int k = 0; k < M; ++k) epl_stage<LN, 1>(lds + k * IMG, e.c[k].params, e.c[k].off, e.c[k].desc);
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
    const bool env_lane = lane < SEP_EP_G && n < e.env.N;
    const int Rv = (int)(B - n0 < 16 ? B - n0 : 16);                // rows of the tile that exist (the last tile may be partial)
    typename Env::State s = {};
    if (env_lane) Env::load(e.env, n, s);
#pragma unroll
    for (int k = 0; k < M; ++k) epl_stage<LN, 1>(lds + k * IMG, e.c[k].params, e.c[k].off, e.c[k].desc);
    __syncthreads();                                                // the critic images are staged
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B;
      __syncthreads();                                              // A_t
      if (env_lane) sep_env_step<Env>(e, n, so, B, s, X, act, lane);
      __syncthreads();                                              // B_t
#pragma unroll
      for (int m = 0; m < M; ++m) sep_copy_rows<W>(e, X, m, Env::obs_dim(m), Env::obs_off(m), so + B + n0, Rv, lane);
    }
    if (env_lane) Env::store(e.env, n, s, true);                    // the environment continues from here in either path
  }
}

template <class Env>
struct SepImgEpisode {
  template <bool RELU, int LN>
  struct K {
    static constexpr auto kernel = rollout_episode_sep_img_kernel<Env, RELU, LN>;
    static constexpr int lds_bytes = sizeof(float) * sep_img_lds_floats<Env, LN>();
  };
};

extern "C" int mappo_rollout_episode_adversary(const mappo_comm_agent *agents, double *agent_pos, double *agent_vel, double *landmark_pos,
                                               int32_t *goal, int32_t *tstep, int64_t *episode, int32_t T, int32_t N,
                                               int32_t env_episode_length, uint64_t env_seed, int32_t deterministic, uint64_t counter,
                                               int32_t centralized, mappo_stream_t stream) {
  const char *who = "rollout_episode_adversary";
  MAPPO_REQUIRE(agents, "%s: null agent descriptors (needs num_agents = 3 of them: adversary, good agent 1, good agent 2)", who);
  const char *const name[MPE_ADV_M] = {"adversary", "good agent 1", "good agent 2"};
  const int Dm[MPE_ADV_M] = {MPE_ADV_OBS_A, MPE_ADV_OBS_G, MPE_ADV_OBS_G}, Am[MPE_ADV_M] = {MPE_ADV_U, MPE_ADV_U, MPE_ADV_U};
  SepEpisodeArgs<MpeAdvArgs, MPE_ADV_M> e;
  if (int rc = sep_episode_fill(e, who, agents, name, Dm, Am, MPE_ADV_SHARE, centralized, deterministic, counter, T, N, env_episode_length)) return rc;
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode, "%s: bad arguments (null state pointer)", who);
  MAPPO_CLEAR_STICKY();
  e.env.apos = agent_pos; e.env.avel = agent_vel; e.env.lpos = landmark_pos; e.env.goal = goal; e.env.tstep = tstep; e.env.episode = episode;
  e.env.N = N; e.env.T = env_episode_length; e.env.mode = 1; e.env.seed = env_seed;
  return sep_episode_launch<SepImgEpisode<MpeAdv>::K>(who, N, agents[0], e, stream);
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
  SepEpisodeArgs<MpeCryptoArgs, MPE_CRYPTO_M> e;
  if (int rc = sep_episode_fill(e, who, agents, name, Dm, Am, MPE_CRYPTO_SHARE, centralized, deterministic, counter, T, N, env_episode_length)) return rc;
  MAPPO_REQUIRE(goal && key && comm && tstep && episode, "%s: bad arguments (null state pointer)", who);
  MAPPO_CLEAR_STICKY();
  e.env.goal = goal; e.env.key = key; e.env.comm = comm; e.env.tstep = tstep; e.env.episode = episode;
  e.env.N = N; e.env.T = env_episode_length; e.env.mode = 1; e.env.L = num_landmarks; e.env.seed = env_seed;
  return sep_episode_launch<SepImgEpisode<MpeCrypto>::K>(who, N, agents[0], e, stream);
}
