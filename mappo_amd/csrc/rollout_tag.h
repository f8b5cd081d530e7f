// rollout_tag.h — one rollout episode on the GPU-resident `simple_tag` environment in ONE launch (mappo_rollout_episode_tag), for the
// SEPARATED runner: four agents (three adversaries with 16 features, the good agent with 14), each with its own actor, critic,
// per-agent reward and SeparatedReplayBuffer.  It does what T x (four mappo_rollout_step + mappo_mpe_tag_step + the four agents'
// inserts) + the four bootstrap launches do, ~9 T + 4 dependent launches.
//
// The two-barrier skeleton of rollout_comm.h / rollout_sep_img.h (read their headers first): a tile is 16 whole environments, one
// workgroup of FOUR waves per tile, one per SIMD.  Eight networks do not fit rollout_sep_img.h's placement: four critic images of
// EplMap<1>::total = 11424 floats plus the tiles are ~191 KB against 160 KB of LDS, and a fifth wave for the environments would put
// two waves on a SIMD and halve the register budget under an actor.  So here
//   wave m = 0, 1, 2   adversary m, both networks.  Its ACTOR has its weights in registers (Trunk16R / Head16R; 16 inputs, so one of
//           the four W1 column blocks is live) except the hidden layer's b2 / g2 / t2, which it reads from a 192-float LDS copy
//           (Trunk16A: 48 registers less, what the tanh build at layer_N 1 needed to stay out of scratch).  Its CRITIC is SPLIT: W1
//           in registers (64 VGPRs), everything else — vectors, the hidden layer, the head — in an LDS image without W1 (TagMap;
//           Trunk16S / Head16S).  The critic runs between the step's two barriers; step T writes next_values.
//   wave 3             the good agent and, in lanes 0 .. 15, the environments.  The environment step (mpe_tag_step_env, ~150 VGPRs
//           while it runs, the state in the lane for the whole episode) does not fit beside a register actor, so this actor reads
//           its weights from a whole LDS image (EplMap / Trunk16L / Head16L of mlp_ep16l.h); its critic is split like the others.
//           Order per step: actor, A_t, environments (mode 1; each agent's OWN reward -> its rew_buf[t], 1 - done -> its
//           mask_buf[t + 1]), critic, B_t.
// Every accessor struct returns the same 16-byte operands in the same order as Trunk16R, so tile16r_step computes the same bits.
// Behind B_t every wave copies its own agent's rows of observation tile t + 1 into its obs[t + 1] / share_obs[t + 1] (sep_copy_rows: what
// the stepwise insert writes) and takes its next inputs from the tile.  A_t: the actions of step t are in LDS and every read of
// observation tile t is done; B_t: observation tile t + 1 is in LDS.  No wave returns early: one whose rows or lanes do not exist
// (last partial tile) still walks all T steps and their barriers.
//
// LDS (floats): four critic images, TagMap<LN>::total each (5968 at layer_N 1, 1424 at 0) | the good agent's actor image,
// EplMap<LN>::total (11424 / 6880) | the observation tile [16][62] — a row is the adversaries' 16 | 16 | 16 features, then the good
// agent's 14: the centralized share row as it stands | one [16][TP] logits tile per wave | the action tile, one column of 16 per
// agent | the adversaries' b2 / g2 / t2, 3 x 192.  At layer_N 1: 4 x 5968 + 11424 + 992 + 4 x 528 + 64 + 576 = 39040 floats =
// 156160 B of 163840; at layer_N 0: 16320 floats = 65280 B.  One workgroup per CU.
// Every value goes through the stepwise kernels' own code (tile16r_step, mpe_tag_step_env), so the four buffers and the environment
// state end up bit-identical to the stepwise path's.
#pragma once
#include "mpe_tag_core.h"
#include "rollout_comm.h"

// the critic's LDS image: EplMap (mlp_ep16l.h) without W1 and with ONE head block
template <int LN>
struct TagMap {
  static constexpr int g0 = 0, t0 = g0 + HID, b1 = t0 + HID, g1 = b1 + HID, t1 = g1 + HID, hid = t1 + HID;
  static constexpr int HL = EPL_MAT + 3 * HID;                      // one hidden layer: w2, b2, g2, t2
  static constexpr int w2(int l) { return hid + l * HL; }
  static constexpr int b2(int l) { return w2(l) + EPL_MAT; }
  static constexpr int g2(int l) { return b2(l) + HID; }
  static constexpr int t2(int l) { return g2(l) + HID; }
  static constexpr int wh = hid + LN * HL, bh = wh + 16 * EPL_WS, total = bh + 16;
};

// lane (j, q)'s view of a split trunk: W1 in registers (as Trunk16R::w1), the rest in the image (as Trunk16L: m = image + j * EPL_WS
// + 4 q for matrix rows 16 bo + j, v = image + 4 q for vectors)
template <int LN>
struct Trunk16S {
  typedef TagMap<LN> Mp;
  f32x4 w1[4][4];
  const float *m, *v;
  __device__ __forceinline__ f32x4 W1(int bo, int b) const { return w1[bo][b]; }
  __device__ __forceinline__ f32x4 G0(int b) const { return lds4(v + Mp::g0 + 16 * b); }
  __device__ __forceinline__ f32x4 T0(int b) const { return lds4(v + Mp::t0 + 16 * b); }
  __device__ __forceinline__ f32x4 B1(int b) const { return lds4(v + Mp::b1 + 16 * b); }
  __device__ __forceinline__ f32x4 G1(int b) const { return lds4(v + Mp::g1 + 16 * b); }
  __device__ __forceinline__ f32x4 T1(int b) const { return lds4(v + Mp::t1 + 16 * b); }
  __device__ __forceinline__ f32x4 W2(int l, int bo, int b) const { return lds4(m + Mp::w2(l) + 16 * bo * EPL_WS + 16 * b); }
  __device__ __forceinline__ f32x4 B2(int l, int b) const { return lds4(v + Mp::b2(l) + 16 * b); }
  __device__ __forceinline__ f32x4 G2(int l, int b) const { return lds4(v + Mp::g2(l) + 16 * b); }
  __device__ __forceinline__ f32x4 T2(int l, int b) const { return lds4(v + Mp::t2(l) + 16 * b); }
};
template <int LN>
struct Head16S {                                                    // the critic's head (MODE 0: one block)
  static constexpr int NBH = 1;
  typedef TagMap<LN> Mp;
  const float *m, *v;
  __device__ __forceinline__ f32x4 WH(int bo, int b) const { return lds4(m + Mp::wh + 16 * bo * EPL_WS + 16 * b); }
  __device__ __forceinline__ f32x4 BH(int bo) const { return lds4(v + Mp::bh + 16 * bo); }
};

// An adversary's actor: Trunk16R with the hidden layer's three vectors (b2, g2, t2: 48 registers) read from LDS instead — v = their
// copy + 4 q, [b2 | g2 | t2] x 64 floats per hidden layer; every other operand is the register trunk's own
template <int LN>
struct Trunk16A {
  const Trunk16R<LN> &r;
  const float *v;
  __device__ __forceinline__ f32x4 W1(int bo, int b) const { return r.w1[bo][b]; }
  __device__ __forceinline__ f32x4 G0(int b) const { return r.g0[b]; }
  __device__ __forceinline__ f32x4 T0(int b) const { return r.t0[b]; }
  __device__ __forceinline__ f32x4 B1(int b) const { return r.b1v[b]; }
  __device__ __forceinline__ f32x4 G1(int b) const { return r.g1[b]; }
  __device__ __forceinline__ f32x4 T1(int b) const { return r.t1[b]; }
  __device__ __forceinline__ f32x4 W2(int l, int bo, int b) const { return r.w2[l][bo][b]; }
  __device__ __forceinline__ f32x4 B2(int l, int b) const { return lds4(v + l * 3 * HID + 16 * b); }
  __device__ __forceinline__ f32x4 G2(int l, int b) const { return lds4(v + l * 3 * HID + HID + 16 * b); }
  __device__ __forceinline__ f32x4 T2(int l, int b) const { return lds4(v + l * 3 * HID + 2 * HID + 16 * b); }
};
#define TAG_AVEC (3 * HID)                                          // floats of that copy per adversary (layer_N <= 1)

// Stage a critic into its image (every thread of the workgroup; the caller passes the barrier): epl_stage without W1, one head block.
template <int LN>
__device__ __forceinline__ void tag_stage(float *img, const float *P, const NetOff &o, const mappo_net_desc &d) {
  typedef TagMap<LN> Mp;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int D = d.in_dim, A = d.out_dim;
#pragma unroll
  for (int l = 0; l < LN; ++l)
    for (int e = tid; e < HID * 16; e += nt) {
      const int r = e >> 4, c = 4 * (e & 15);
      *reinterpret_cast<f32x4 *>(img + Mp::w2(l) + r * EPL_WS + c) = ld4ua(P + o.w2[l] + (size_t)r * HID + c);
    }
  for (int e = tid; e < 16 * 16; e += nt) {
    const int a = e >> 4, c = 4 * (e & 15);
    *reinterpret_cast<f32x4 *>(img + Mp::wh + a * EPL_WS + c) = ld4ua(P + o.wh + (size_t)min(a, A - 1) * HID + c);
  }
  const bool fnorm = d.use_feature_norm != 0;
  const int ofw = fnorm ? o.fn_w : o.w1, ofb = fnorm ? o.fn_b : o.w1;                // (as trunk16r_load)
  for (int k = tid; k < HID; k += nt) {
    img[Mp::g0 + k] = P[ofw + min(k, D - 1)];
    img[Mp::t0 + k] = P[ofb + min(k, D - 1)];
    img[Mp::b1 + k] = P[o.b1 + k]; img[Mp::g1 + k] = P[o.ln1_w + k]; img[Mp::t1 + k] = P[o.ln1_b + k];
#pragma unroll
    for (int l = 0; l < LN; ++l) { img[Mp::b2(l) + k] = P[o.b2[l] + k]; img[Mp::g2(l) + k] = P[o.ln2_w[l] + k]; img[Mp::t2(l) + k] = P[o.ln2_b[l] + k]; }
    if (k < 16) img[Mp::bh + k] = P[o.bh + min(k, A - 1)];
  }
}

typedef SepEpisodeArgs<MpeTagArgs, MPE_TAG_M> TagEpisodeArgs;         // agents 0 .. 2: adversaries, 3: the good agent

#define TAG_X_TILE (16 * MPE_TAG_SHARE)
template <int LN>
constexpr int tag_ep_lds_floats() {
  return MPE_TAG_M * TagMap<LN>::total + EplMap<LN>::total + TAG_X_TILE + MPE_TAG_M * 16 * TP + MPE_TAG_M * 16 + MPE_TAG_GOOD * TAG_AVEC;
}

// the critic's W1 into the split trunk's registers, as trunk16r_load reads it
template <int LN>
__device__ __forceinline__ void tag_load_w1(Trunk16S<LN> &cw, const FwdArgs &fc, int S, int j, int q) {
  const int NB1 = (S + 15) >> 4;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (b < NB1) {
#pragma unroll
      for (int bo = 0; bo < 4; ++bo) cw.w1[bo][b] = ld4ua(fc.params + fc.off.w1 + (size_t)(16 * bo + j) * S + 16 * b + 4 * q);
    }
}

template <bool RELU, int LN>
__global__ __launch_bounds__(SEP_EP_WAVES * WAVE, 1) void rollout_episode_tag_kernel(TagEpisodeArgs e) {
  extern __shared__ __align__(16) float lds[];
  constexpr int IMG = TagMap<LN>::total, W = MPE_TAG_SHARE, G = MPE_TAG_GOOD;
  float *aimg = lds + MPE_TAG_M * IMG;                              // the good agent's actor, whole (EplMap)
  float *X = aimg + EplMap<LN>::total, *tZ = X + TAG_X_TILE, *act = tZ + MPE_TAG_M * 16 * TP, *avec = act + MPE_TAG_M * 16;
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), j = lane & 15, q = lane >> 4;
  const int T = e.T;
  const int64_t B = e.env.N;                                        // rows of every buffer: one per environment
  const int n0 = (int)blockIdx.x * SEP_EP_G;                        // first environment / buffer row of this tile
  const int64_t i = (int64_t)n0 + j;
  const bool ok = i < B;
  const int jr = ok ? j : 0;
  const int Rv = (int)(B - n0 < 16 ? B - n0 : 16);                  // rows of the tile that exist (the last tile may be partial)
  if (wave < G) {
    // ---- adversary m: actor in registers, critic split; step 0 reads buffer slot 0, as the stepwise path does ----
    const int m = wave;
    constexpr int D = MPE_TAG_OBS_A;
    const int xo = MpeTag::obs_off(m);
    FwdArgs fa, fc;
    comm_fwd_args(fa, e.a[m], B, e.deterministic);
    comm_fwd_args(fc, e.c[m], B, 0);
    const int S = fc.desc.in_dim, so_x = e.centralized ? 0 : xo;    // 62 (centralized) or D
    f32x4 xa[4], xc[4];
    spread_load_x(xa, e.obs_buf[m] + (ok ? i : 0) * D, D, q);
    spread_load_x(xc, e.share_buf[m] + (ok ? i : 0) * S, S, q);
    Trunk16R<LN> tw;
    trunk16r_load<LN>(tw, fa.params, fa.off, fa.desc, j, q);
    Head16R<1> hd;
    head16r_load<1>(hd, fa.params, fa.off, fa.desc.out_dim, j, q);
    const uint64_t ctr0 = e.counter + (e.a[m].counter_dev ? *e.a[m].counter_dev : 0ull);      // read once: the word is fixed for the launch
    const float *img = lds + m * IMG;
    Trunk16S<LN> cw;
    cw.m = img + j * EPL_WS + 4 * q; cw.v = img + 4 * q;
    tag_load_w1<LN>(cw, fc, S, j, q);
    const Head16S<LN> ch = {cw.m, cw.v};
#pragma unroll
    for (int k = 0; k < MPE_TAG_M; ++k) tag_stage<LN>(lds + k * IMG, e.c[k].params, e.c[k].off, e.c[k].desc);
    epl_stage<LN, 2>(aimg, e.a[G].params, e.a[G].off, e.a[G].desc);
    if constexpr (LN > 0)                                           // this actor's b2 | g2 | t2 (this wave alone reads them)
      for (int k = lane; k < HID; k += WAVE) {
        avec[m * TAG_AVEC + k] = fa.params[fa.off.b2[0] + k]; avec[m * TAG_AVEC + HID + k] = fa.params[fa.off.ln2_w[0] + k];
        avec[m * TAG_AVEC + 2 * HID + k] = fa.params[fa.off.ln2_b[0] + k];
      }
    const Trunk16A<LN> ta = {tw, avec + m * TAG_AVEC + 4 * q};
    __syncthreads();                                                // the images are staged
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B;
      asm volatile("" ::: "memory");
      tile16r_step<RELU, LN, 1, false, true>(fa, ta, hd, xa, nullptr, fa.actions + so, fa.logp + so, ctr0 + (uint64_t)t, nullptr,
                                             tZ + m * 16 * TP, i, ok, j, q, act + m * 16);
      __syncthreads();                                              // A_t
      asm volatile("" ::: "memory");        // the image is loop-invariant: keep its reads inside the step (hoisted, they are a second register network)
      tile16r_step<RELU, LN, 0>(fc, cw, ch, xc, fc.out + so, nullptr, nullptr, 0ull, nullptr, tZ + m * 16 * TP, i, ok, j, q);
      __syncthreads();                                              // B_t
      sep_copy_rows<W>(e, X, m, D, xo, so + B + n0, Rv, lane);      // the tile's next write is behind A_{t + 1}, which this wave reaches after these reads
      spread_load_x(xa, X + jr * W + xo, D, q);
      spread_load_x(xc, X + jr * W + so_x, S, q);
    }
    asm volatile("" ::: "memory");
    tile16r_step<RELU, LN, 0>(fc, cw, ch, xc, e.next_values[m], nullptr, nullptr, 0ull, nullptr, tZ + m * 16 * TP, i, ok, j, q);
  } else {
    // ---- the good agent — actor from its LDS image, critic split — and, in lanes 0 .. 15, the environments: the state stays in the
    // lane for the whole episode ----
    constexpr int m = G, D = MPE_TAG_OBS_G, xo = MpeTag::obs_off(G);
    const int n = n0 + lane;
    const bool env_lane = lane < SEP_EP_G && n < e.env.N;
    MpeTagState s = {};
    if (env_lane) mpe_tag_load(e.env, n, s);
    FwdArgs fa, fc;
    comm_fwd_args(fa, e.a[m], B, e.deterministic);
    comm_fwd_args(fc, e.c[m], B, 0);
    const int S = fc.desc.in_dim, so_x = e.centralized ? 0 : xo;
    f32x4 xa[4], xc[4];
    spread_load_x(xa, e.obs_buf[m] + (ok ? i : 0) * D, D, q);
    spread_load_x(xc, e.share_buf[m] + (ok ? i : 0) * S, S, q);
    const uint64_t ctr0 = e.counter + (e.a[m].counter_dev ? *e.a[m].counter_dev : 0ull);
    const Trunk16L<LN> tw = {aimg + j * EPL_WS + 4 * q, aimg + 4 * q};
    const Head16L<LN, 1> hd = {tw.m, tw.v};
    const float *img = lds + m * IMG;
    Trunk16S<LN> cw;
    cw.m = img + j * EPL_WS + 4 * q; cw.v = img + 4 * q;
    tag_load_w1<LN>(cw, fc, S, j, q);
    const Head16S<LN> ch = {cw.m, cw.v};
#pragma unroll
    for (int k = 0; k < MPE_TAG_M; ++k) tag_stage<LN>(lds + k * IMG, e.c[k].params, e.c[k].off, e.c[k].desc);
    epl_stage<LN, 2>(aimg, e.a[G].params, e.a[G].off, e.a[G].desc);
    __syncthreads();                                                // the images are staged
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B;
      asm volatile("" ::: "memory");
      tile16r_step<RELU, LN, 1, false, true>(fa, tw, hd, xa, nullptr, fa.actions + so, fa.logp + so, ctr0 + (uint64_t)t, nullptr,
                                             tZ + m * 16 * TP, i, ok, j, q, act + m * 16);
      __syncthreads();                                              // A_t
      if (env_lane) {       // sep_env_step, kept inline: through the shared function the register allocation moved and a rollout took 2 % longer
        float reward[MPE_TAG_M];
        float *row = X + lane * W;
        const bool done = mpe_tag_step_env(e.env, n, act + lane, 16, s, row, row + MpeTag::obs_off(1), row + MpeTag::obs_off(2),
                                           row + MpeTag::obs_off(3), reward);
#pragma unroll
        for (int k = 0; k < MPE_TAG_M; ++k) {
          e.rew_buf[k][so + n] = reward[k];
          e.mask_buf[k][so + B + n] = done ? 0.f : 1.f;
        }
      }
      asm volatile("" ::: "memory");
      tile16r_step<RELU, LN, 0>(fc, cw, ch, xc, fc.out + so, nullptr, nullptr, 0ull, nullptr, tZ + m * 16 * TP, i, ok, j, q);
      __syncthreads();                                              // B_t
      sep_copy_rows<W>(e, X, m, D, xo, so + B + n0, Rv, lane);
      spread_load_x(xa, X + jr * W + xo, D, q);
      spread_load_x(xc, X + jr * W + so_x, S, q);
    }
    asm volatile("" ::: "memory");
    tile16r_step<RELU, LN, 0>(fc, cw, ch, xc, e.next_values[m], nullptr, nullptr, 0ull, nullptr, tZ + m * 16 * TP, i, ok, j, q);
    if (env_lane) mpe_tag_store(e.env, n, s, true);                 // the environment continues from here in either path
  }
}

template <bool RELU, int LN>
struct TagEpisode {
  static constexpr auto kernel = rollout_episode_tag_kernel<RELU, LN>;
  static constexpr int lds_bytes = sizeof(float) * tag_ep_lds_floats<LN>();
};

extern "C" int mappo_rollout_episode_tag(const mappo_comm_agent *agents, double *agent_pos, double *agent_vel, double *landmark_pos,
                                         int32_t *tstep, int64_t *episode, int32_t T, int32_t N, int32_t env_episode_length,
                                         uint64_t env_seed, int32_t deterministic, uint64_t counter, int32_t centralized,
                                         mappo_stream_t stream) {
  const char *who = "rollout_episode_tag";
  MAPPO_REQUIRE(agents, "%s: null agent descriptors (needs num_agents = 4 of them: adversaries 0, 1, 2, then the good agent)", who);
  const char *const name[MPE_TAG_M] = {"adversary 0", "adversary 1", "adversary 2", "good agent"};
  const int Dm[MPE_TAG_M] = {MPE_TAG_OBS_A, MPE_TAG_OBS_A, MPE_TAG_OBS_A, MPE_TAG_OBS_G}, Am[MPE_TAG_M] = {MPE_TAG_U, MPE_TAG_U, MPE_TAG_U, MPE_TAG_U};
  TagEpisodeArgs e;
  if (int rc = sep_episode_fill(e, who, agents, name, Dm, Am, MPE_TAG_SHARE, centralized, deterministic, counter, T, N, env_episode_length)) return rc;
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && tstep && episode, "%s: bad arguments (null state pointer)", who);
  MAPPO_CLEAR_STICKY();
  e.env.apos = agent_pos; e.env.avel = agent_vel; e.env.lpos = landmark_pos; e.env.tstep = tstep; e.env.episode = episode;
  e.env.N = N; e.env.T = env_episode_length; e.env.mode = 1; e.env.seed = env_seed;
  return sep_episode_launch<TagEpisode>(who, N, agents[0], e, stream);
}
