// rollout_world_comm.h — one rollout episode on the GPU-resident `simple_world_comm` environment in ONE launch
// (mappo_rollout_episode_world_comm), for the SEPARATED runner: six agents — the leader (34 features, MultiDiscrete (5, 4)), three
// more adversaries (34, Discrete(5)) and two good agents (28, Discrete(5)) — each with its own actor, per-agent reward and
// SeparatedReplayBuffer.  It does what T x (mappo_rollout_step_md for the leader + five mappo_rollout_step + mappo_mpe_world_comm_step
// in mode 1 + the six agents' inserts) do, WITHOUT the values: twelve networks do not fit one workgroup (six 192-wide critics are no
// LDS images, and the registers go to the actors and the environment step), and no value is needed while the rollout runs.  So this
// launch runs the six ACTORS and the ENVIRONMENTS, and the caller runs each critic once afterwards over all T + 1 share_obs slots.
//
// The two-barrier skeleton of rollout_comm.h / rollout_tag.h (read their headers first): a tile is 16 whole environments, one
// workgroup per tile, one row per environment and agent.  FOUR waves, one per SIMD — three actor waves of two agents each, and one
// wave for the environments:
//   wave 0             the leader, then adversary 1.  The leader: tile16r_step MODE 5 with the heads (5, 4) — 9 logits, one head
//           block; head k of row n draws Philox index (k << 32) | n; actions / logp [T][N][2]; the row's move and word also go to
//           the action tile.  Every other agent m: tile16r_step MODE 1, Discrete(5), actions / logp [T][N]; its index goes to the
//           action tile.
//   wave 1             adversaries 2 and 3.
//   wave 2             the good agents 4 and 5.
//   wave 3, lanes 0 .. 15   the environments, between the two barriers: the tile's seven indices -> MpeWcAction (mpe_wc_move_idx /
//           mpe_wc_word_idx, what mpe_wc_decode does in mode 1), mpe_wc_step_env on the state the lane holds for the whole episode
//           (mpe_wc_load once, mpe_wc_store(.., true) at the end), the six observations straight into the tile's row; each agent's
//           OWN reward -> its rew_buf[t], 1 - done -> its mask_buf[t + 1].  The leader's word reaches the adversaries' rows through
//           mpe_wc_step_env itself (zeros where the environment reset).
// Every agent draws with its own seed and counter + t + *counter_dev.  A_t: all seven action columns of step t are in LDS and every
// read of observation tile t is done; B_t: observation tile t + 1 is in LDS.  Nothing runs between the barriers but the environments.
// Behind B_t every actor wave copies its two agents' rows of tile t + 1 into their obs[t + 1] and share_obs[t + 1] (the whole
// 192-float row when centralized, its own rows otherwise: what the stepwise insert writes) and takes its next inputs from the tile.
// No wave returns early: one whose rows or lanes do not exist (last partial tile) still walks the staging barrier and all 2 T step
// barriers.
//
// Placement.  One wave per actor and one for the environments, seven waves on four SIMDs, would be two waves per SIMD and 256
// registers each.  The environment step alone fits that (mpe_world_comm_step_kernel: 254 VGPRs) — but not inside the loop over the
// T steps: with the state carried from step to step and what the compiler keeps across the loop, the environment wave needs ~395
// registers (256 VGPRs + 138 AGPRs under a 512 budget) and, held to 256, spills 568 B per lane even with no actor in the kernel
// (1.9 KB with them); keeping the state in LDS between the steps or stepping all 64 lanes without the divergent branch did not
// lower it (the per-instantiation figures of both placements and the compile line are in DESIGN.md §3).
// So the workgroup has FOUR waves, 512 registers each, and an actor wave runs its two agents one after the other — the
// actors are short next to the float64 environment step.  LDS is 163840 B = 40960 floats; the observation tile, six logits tiles
// and the action tile take 6368, which leaves room for three whole actor images (EplMap<1>::total = 11424) at most, and six images
// without W1 (5984 each here) are 1312 floats too many.  So every actor is SPLIT, W1 in registers and the rest in an LDS image (as
// the critics of rollout_tag.h), and the two good agents, whose 28 inputs need only two of W1's four column blocks (32 VGPRs; 34
// inputs need three: 48), also keep the hidden layer's W2 in registers (64 VGPRs), which takes that matrix out of their images:
//   adversaries 0 .. 3   registers: W1[..][3 blocks] = 48 VGPRs | image WcMap<LN, true>:  vectors, W2, b2 / g2 / t2, head
//   good agents 4, 5     registers: W1[..][2 blocks] + W2 = 96 VGPRs | image WcMap<LN, false>: vectors, b2 / g2 / t2, head
// (two of them per wave: 96 / 192 VGPRs of weights).  The kernel fixes in_dim / out_dim of each actor to the scenario's constants
// (the host has checked them), so the unused column blocks and the second head block of MODE 1 are not compiled.  Every accessor
// returns the same 16-byte operands in the same order as Trunk16R / Head16R, so tile16r_step computes the same bits.  All four
// instantiations (relu / tanh x layer_N 0 / 1): 256 VGPRs + 144 .. 146 AGPRs, no scratch, one wave per SIMD.
//
// LDS (floats): four adversary images, WcMap<LN, true>::total each (5984 at layer_N 1, 1440 at 0) | two good-agent images,
// WcMap<LN, false>::total (1632 / 1440) | the observation tile [16][192], rows 193 floats apart — the six observations side by side,
// the centralized share row as it stands; the odd stride keeps the 16 environment lanes, and the 16 rows an actor's lanes read, on
// different banks | one [16][TP] logits tile per actor | the action tile: the leader's [16][2], then one column of 16 per agent
// 1 .. 5.  At layer_N 1: 4 x 5984 + 2 x 1632 + 3088 + 6 x 528 + 112 = 33568 floats = 134272 B of 163840; at layer_N 0: 15008 floats
// = 60032 B.  One workgroup per CU.
// Every value goes through the stepwise kernels' own code (tile16r_step, mpe_wc_step_env), so the six buffers and the environment
// state end up bit-identical to the stepwise entry points'.
#pragma once
#include "mpe_world_comm_core.h"
#include "rollout_comm.h"

// an actor's LDS image: EplMap (mlp_ep16l.h) without W1, with ONE head block of weights and both blocks of the head's bias (MODE 1
// reads the second block's bias before it drops it); W2L: the hidden layer's matrix is in the image (else in registers)
template <int LN, bool W2L>
struct WcMap {
  static constexpr int g0 = 0, t0 = g0 + HID, b1 = t0 + HID, g1 = b1 + HID, t1 = g1 + HID, hid = t1 + HID;
  static constexpr int MAT = W2L ? EPL_MAT : 0;
  static constexpr int HL = MAT + 3 * HID;                          // one hidden layer: (w2,) b2, g2, t2
  static constexpr int w2(int l) { return hid + l * HL; }
  static constexpr int b2(int l) { return w2(l) + MAT; }
  static constexpr int g2(int l) { return b2(l) + HID; }
  static constexpr int t2(int l) { return g2(l) + HID; }
  static constexpr int wh = hid + LN * HL, bh = wh + 16 * EPL_WS, total = bh + 32;
};

// lane (j, q)'s view of a split actor trunk: NB1 column blocks of W1 in registers (as Trunk16R::w1), W2 in registers too unless W2L,
// the rest in the image (as Trunk16L: m = image + j * EPL_WS + 4 q for matrix rows 16 bo + j, v = image + 4 q for vectors)
template <int LN, int NB1, bool W2L>
struct Trunk16W {
  typedef WcMap<LN, W2L> Mp;
  f32x4 w1[4][NB1];
  f32x4 w2[W2L || LN == 0 ? 1 : 4][W2L || LN == 0 ? 1 : 4];
  const float *m, *v;
  __device__ __forceinline__ f32x4 W1(int bo, int b) const { return w1[bo][b < NB1 ? b : 0]; }
  __device__ __forceinline__ f32x4 G0(int b) const { return lds4(v + Mp::g0 + 16 * b); }
  __device__ __forceinline__ f32x4 T0(int b) const { return lds4(v + Mp::t0 + 16 * b); }
  __device__ __forceinline__ f32x4 B1(int b) const { return lds4(v + Mp::b1 + 16 * b); }
  __device__ __forceinline__ f32x4 G1(int b) const { return lds4(v + Mp::g1 + 16 * b); }
  __device__ __forceinline__ f32x4 T1(int b) const { return lds4(v + Mp::t1 + 16 * b); }
  __device__ __forceinline__ f32x4 W2(int l, int bo, int b) const {
    if constexpr (W2L) return lds4(m + Mp::w2(l) + 16 * bo * EPL_WS + 16 * b);
    else return w2[bo][b];
  }
  __device__ __forceinline__ f32x4 B2(int l, int b) const { return lds4(v + Mp::b2(l) + 16 * b); }
  __device__ __forceinline__ f32x4 G2(int l, int b) const { return lds4(v + Mp::g2(l) + 16 * b); }
  __device__ __forceinline__ f32x4 T2(int l, int b) const { return lds4(v + Mp::t2(l) + 16 * b); }
};
template <int LN, bool W2L, int MODE>
struct Head16W {
  static constexpr int NBH = Head16R<MODE>::NBH;
  typedef WcMap<LN, W2L> Mp;
  const float *m, *v;
  __device__ __forceinline__ f32x4 WH(int bo, int b) const { return lds4(m + Mp::wh + 16 * bo * EPL_WS + 16 * b); }     // (out_dim <= 16: block 0 alone is read)
  __device__ __forceinline__ f32x4 BH(int bo) const { return lds4(v + Mp::bh + 16 * bo); }
};

// Stage an actor into its image (every thread of the workgroup; the caller passes the barrier): epl_stage without W1, one head block
template <int LN, bool W2L>
__device__ __forceinline__ void wc_stage(float *img, const float *P, const NetOff &o, const mappo_net_desc &d) {
  typedef WcMap<LN, W2L> Mp;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int D = d.in_dim, A = d.out_dim;
  if constexpr (W2L) {
#pragma unroll
    for (int l = 0; l < LN; ++l)
      for (int e = tid; e < HID * 16; e += nt) {
        const int r = e >> 4, c = 4 * (e & 15);
        *reinterpret_cast<f32x4 *>(img + Mp::w2(l) + r * EPL_WS + c) = ld4ua(P + o.w2[l] + (size_t)r * HID + c);
      }
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
    if (k < 32) img[Mp::bh + k] = P[o.bh + min(k, A - 1)];
  }
}

// the six actors only: with the critics' CommNet the block would not fit the kernel arguments
struct WcEpisodeArgs {
  CommNet a[MPE_WC_M];                                              // agent 0: the leader, 1 .. 3: adversaries, 4, 5: good agents
  MpeWcArgs env;                                                    // state arrays, N, T = the ENV's episode length, mode 1, seed
  float *obs_buf[MPE_WC_M], *share_buf[MPE_WC_M];                   // [T + 1][N][D_m], [T + 1][N][S_m]
  float *rew_buf[MPE_WC_M], *mask_buf[MPE_WC_M];                    // [T][N], [T + 1][N]
  uint64_t counter;
  int T, centralized, deterministic;                                // rollout steps
};
static_assert(sizeof(WcEpisodeArgs) <= 4096, "the episode's argument block must stay under the 4 KB kernel-argument limit");

#define WC_EP_G 16                                                  // environments per tile (workgroup)
#define WC_EP_WAVES 4                                               // three actor waves of two agents each, then the environments
#define WC_XS (MPE_WC_SHARE + 1)                                    // floats between two rows of the observation tile
#define WC_ACT_TILE (16 * MPE_WC_ACT_IDX)                           // the leader's [16][2], then agents 1 .. 5: [16] each
template <int LN>
constexpr int wc_ep_lds_floats() {
  return MPE_WC_ADV * WcMap<LN, true>::total + (MPE_WC_M - MPE_WC_ADV) * WcMap<LN, false>::total + 16 * WC_XS + MPE_WC_M * 16 * TP + WC_ACT_TILE;
}
template <int LN>
constexpr int wc_img_off(int m) {
  return m < MPE_WC_ADV ? m * WcMap<LN, true>::total : MPE_WC_ADV * WcMap<LN, true>::total + (m - MPE_WC_ADV) * WcMap<LN, false>::total;
}

// all six images (every thread of the workgroup; the caller passes the barrier)
template <int LN>
__device__ __forceinline__ void wc_stage_all(const WcEpisodeArgs &e, float *lds) {
#pragma unroll
  for (int k = 0; k < MPE_WC_ADV; ++k) wc_stage<LN, true>(lds + wc_img_off<LN>(k), e.a[k].params, e.a[k].off, e.a[k].desc);
#pragma unroll
  for (int k = MPE_WC_ADV; k < MPE_WC_M; ++k) wc_stage<LN, false>(lds + wc_img_off<LN>(k), e.a[k].params, e.a[k].off, e.a[k].desc);
}

// One agent's actor in the lane: its inputs, its W1 (and W2) registers, its view of the image.  D / A: the scenario's constants
// for this agent; MODE 5 (K = 2 heads) for the leader.  A wave holds two of these and runs them one after the other.
template <bool RELU, int LN, int MODE, int D, int A, bool W2L>
struct WcActor {
  static constexpr int NB1 = (D + 15) / 16, K = MODE == 5 ? 2 : 1;
  FwdArgs fa;
  f32x4 xa[4];
  Trunk16W<LN, NB1, W2L> tw;
  uint64_t ctr0;
  float *tZ, *act_m;
  int m, xo;

  // the loads that do not need the images: step 0 reads buffer slot 0, as the stepwise path does
  __device__ __forceinline__ void init(const WcEpisodeArgs &e, float *lds, int m_, int64_t i, bool ok, int j, int q) {
    m = m_; xo = mpe_wc_obs_off(m);
    float *X = lds + wc_img_off<LN>(MPE_WC_M), *act = X + 16 * WC_XS + MPE_WC_M * 16 * TP;
    tZ = X + 16 * WC_XS + m * 16 * TP;
    act_m = m == 0 ? act : act + 16 * (m + 1);                      // the leader's [16][2] | agent m's column
    const float *img = lds + wc_img_off<LN>(m);
    comm_fwd_args(fa, e.a[m], e.env.N, e.deterministic);
    fa.desc.in_dim = D; fa.desc.out_dim = A;                        // what the host has checked, as constants
    spread_load_x(xa, e.obs_buf[m] + (ok ? i : 0) * D, D, q);
    tw.m = img + j * EPL_WS + 4 * q; tw.v = img + 4 * q;
#pragma unroll
    for (int b = 0; b < NB1; ++b)
#pragma unroll
      for (int bo = 0; bo < 4; ++bo) tw.w1[bo][b] = ld4ua(fa.params + fa.off.w1 + (size_t)(16 * bo + j) * D + 16 * b + 4 * q);   // (as trunk16r_load)
    if constexpr (!W2L && LN > 0) {
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int bo = 0; bo < 4; ++bo) tw.w2[bo][b] = ld4ua(fa.params + fa.off.w2[0] + (size_t)(16 * bo + j) * HID + 16 * b + 4 * q);
    }
    ctr0 = e.counter + (e.a[m].counter_dev ? *e.a[m].counter_dev : 0ull);        // read once: the word is fixed for the launch
  }
  // the actor of step t: actions / logp slot t and the action tile
  __device__ __forceinline__ void step(int t, int64_t B, int64_t i, bool ok, int j, int q) {
    const int64_t so = (int64_t)t * B * K;
    const Head16W<LN, W2L, MODE> hd = {tw.m, tw.v};
    const MdHeads md = {2, {MPE_WC_U, MPE_WC_C, 0, 0}};             // the leader's heads; the entry point admits no others
    asm volatile("" ::: "memory");          // the image is loop-invariant: keep its reads inside the step (hoisted, they are a register network)
    tile16r_step<RELU, LN, MODE, false, true>(fa, tw, hd, xa, nullptr, fa.actions + so, fa.logp + so, ctr0 + (uint64_t)t, nullptr, tZ, i, ok, j,
                                              q, act_m, &md);
  }
  // behind B_t: what the stepwise insert writes into agent m's slot t + 1 (row0 = (t + 1) N + n0), and the next inputs.  The tile's
  // next write is behind A_{t + 1}, which this wave reaches after these reads
  __device__ __forceinline__ void next(const WcEpisodeArgs &e, const float *X, int64_t row0, int Rv, int jr, int lane, int q) {
    float *od = e.obs_buf[m] + row0 * D;
    for (int k = lane; k < Rv * D; k += WAVE) { const int r = k / D; od[k] = X[r * WC_XS + xo + (k - r * D)]; }
    if (e.centralized) {
      float *sd = e.share_buf[m] + row0 * MPE_WC_SHARE;
      for (int k = lane; k < Rv * MPE_WC_SHARE; k += WAVE) { const int r = k / MPE_WC_SHARE; sd[k] = X[r * WC_XS + (k - r * MPE_WC_SHARE)]; }
    } else {
      float *sd = e.share_buf[m] + row0 * D;
      for (int k = lane; k < Rv * D; k += WAVE) { const int r = k / D; sd[k] = X[r * WC_XS + xo + (k - r * D)]; }
    }
    spread_load_x(xa, X + jr * WC_XS + xo, D, q);
  }
};

// An actor wave over the whole episode: agents m0 and m0 + 1, actor type A0 and A1
template <int LN, class A0, class A1>
__device__ __forceinline__ void wc_actor_wave(const WcEpisodeArgs &e, float *lds, const int m0, const int lane, const int n0) {
  const float *X = lds + wc_img_off<LN>(MPE_WC_M);
  const int j = lane & 15, q = lane >> 4;
  const int T = e.T;
  const int64_t B = e.env.N;                                        // rows of every buffer: one per environment
  const int64_t i = (int64_t)n0 + j;
  const bool ok = i < B;
  const int jr = ok ? j : 0;
  const int Rv = (int)(B - n0 < 16 ? B - n0 : 16);                  // rows of the tile that exist (the last tile may be partial)
  A0 a0;
  A1 a1;
  a0.init(e, lds, m0, i, ok, j, q);
  a1.init(e, lds, m0 + 1, i, ok, j, q);
  wc_stage_all<LN>(e, lds);
  __syncthreads();                                                  // the images are staged
  for (int t = 0; t < T; ++t) {
    a0.step(t, B, i, ok, j, q);
    a1.step(t, B, i, ok, j, q);
    __syncthreads();                                                // A_t
    __syncthreads();                                                // B_t
    const int64_t row0 = (int64_t)(t + 1) * B + n0;
    a0.next(e, X, row0, Rv, jr, lane, q);
    a1.next(e, X, row0, Rv, jr, lane, q);
  }
}

// The environment wave, lanes 0 .. 15: the state stays in the lane for the whole episode
template <int LN>
__device__ __forceinline__ void wc_env_wave(const WcEpisodeArgs &e, float *lds, const int lane, const int n0) {
  float *X = lds + wc_img_off<LN>(MPE_WC_M);
  const float *act = X + 16 * WC_XS + MPE_WC_M * 16 * TP;
  const int T = e.T;
  const int64_t B = e.env.N;
  const int n = n0 + lane;
  const bool env_lane = lane < WC_EP_G && n < e.env.N;
  MpeWcState s = {};
  if (env_lane) mpe_wc_load(e.env, n, s);
  wc_stage_all<LN>(e, lds);
  __syncthreads();                                                  // the images are staged
  for (int t = 0; t < T; ++t) {
    const int64_t so = (int64_t)t * B;
    __syncthreads();                                                // A_t
    if (env_lane) {         // obs -> the tile's row, each agent's own reward -> slot t, masks -> slot t + 1 of its buffer
      MpeWcAction d;
      mpe_wc_move_idx(act[2 * lane], d.u[0]);
      mpe_wc_word_idx(act[2 * lane + 1], d.c);
#pragma unroll
      for (int m = 1; m < MPE_WC_M; ++m) mpe_wc_move_idx(act[16 * (m + 1) + lane], d.u[m]);
      float *row = X + lane * WC_XS;
      float *const o[MPE_WC_M] = {row, row + mpe_wc_obs_off(1), row + mpe_wc_obs_off(2), row + mpe_wc_obs_off(3), row + mpe_wc_obs_off(4),
                                  row + mpe_wc_obs_off(5)};
      float reward[MPE_WC_M];
      const bool done = mpe_wc_step_env(e.env, n, d, s, o, reward);
#pragma unroll
      for (int k = 0; k < MPE_WC_M; ++k) {
        e.rew_buf[k][so + n] = reward[k];
        e.mask_buf[k][so + B + n] = done ? 0.f : 1.f;
      }
    }
    __syncthreads();                                                // B_t
  }
  if (env_lane) mpe_wc_store(e.env, n, s, true);                    // the environment continues from here in either path
}

template <bool RELU, int LN>
__global__ __launch_bounds__(WC_EP_WAVES * WAVE, 1) void rollout_episode_world_comm_kernel(WcEpisodeArgs e) {
  extern __shared__ __align__(16) float lds[];
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const int n0 = (int)blockIdx.x * WC_EP_G;                         // first environment / buffer row of this tile
  typedef WcActor<RELU, LN, 5, MPE_WC_OBS_A, MPE_WC_ACT_LEADER, true> Leader;
  typedef WcActor<RELU, LN, 1, MPE_WC_OBS_A, MPE_WC_U, true> Adversary;
  typedef WcActor<RELU, LN, 1, MPE_WC_OBS_G, MPE_WC_U, false> Good;
  if (wave == 0) wc_actor_wave<LN, Leader, Adversary>(e, lds, 0, lane, n0);
  else if (wave == 1) wc_actor_wave<LN, Adversary, Adversary>(e, lds, 2, lane, n0);
  else if (wave == 2) wc_actor_wave<LN, Good, Good>(e, lds, MPE_WC_ADV, lane, n0);
  else wc_env_wave<LN>(e, lds, lane, n0);
}

extern "C" int mappo_rollout_episode_world_comm(const mappo_comm_agent *agents, double *agent_pos, double *agent_vel, double *landmark_pos,
                                                int32_t *tstep, int64_t *episode, int32_t T, int32_t N, int32_t env_episode_length,
                                                uint64_t env_seed, int32_t deterministic, uint64_t counter, int32_t centralized,
                                                mappo_stream_t stream) {
  const char *who = "rollout_episode_world_comm";
  MAPPO_REQUIRE(agents, "%s: null agent descriptors (needs num_agents = 6 of them: the leader, adversaries 1, 2, 3, then the two good agents)",
                who);
  const char *const name[MPE_WC_M] = {"leader", "adversary 1", "adversary 2", "adversary 3", "good agent 4", "good agent 5"};
  const int Dm[MPE_WC_M] = {MPE_WC_OBS_A, MPE_WC_OBS_A, MPE_WC_OBS_A, MPE_WC_OBS_A, MPE_WC_OBS_G, MPE_WC_OBS_G};
  const int Am[MPE_WC_M] = {MPE_WC_ACT_LEADER, MPE_WC_U, MPE_WC_U, MPE_WC_U, MPE_WC_U, MPE_WC_U};
  SepEpisodeArgs<MpeWcArgs, MPE_WC_M> h;                            // the checks and the fill of the siblings; the critics stay on the host
  if (int rc = sep_episode_fill(h, who, agents, name, Dm, Am, MPE_WC_SHARE, centralized, deterministic, counter, T, N, env_episode_length)) return rc;
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && tstep && episode, "%s: bad arguments (null state pointer)", who);
  MAPPO_CLEAR_STICKY();
  WcEpisodeArgs e = {};
  for (int m = 0; m < MPE_WC_M; ++m) {
    e.a[m] = h.a[m];
    e.obs_buf[m] = h.obs_buf[m]; e.share_buf[m] = h.share_buf[m]; e.rew_buf[m] = h.rew_buf[m]; e.mask_buf[m] = h.mask_buf[m];
  }
  e.counter = counter; e.T = T; e.centralized = centralized; e.deterministic = deterministic;
  e.env.apos = agent_pos; e.env.avel = agent_vel; e.env.lpos = landmark_pos; e.env.tstep = tstep; e.env.episode = episode;
  e.env.N = N; e.env.T = env_episode_length; e.env.mode = 1; e.env.seed = env_seed;
  const dim3 grid((unsigned)((N + WC_EP_G - 1) / WC_EP_G));
  if (int rc = dispatch_relu_ln<1>(agents[0].actor_desc.use_relu != 0, agents[0].actor_desc.layer_N, [&](auto R, auto L) {
        constexpr int lds_bytes = sizeof(float) * wc_ep_lds_floats<L.value>();
        return launch_kernel<rollout_episode_world_comm_kernel<R.value, L.value>, lds_bytes>(who, grid, dim3(WC_EP_WAVES * WAVE), lds_bytes,
                                                                                            as_stream(stream), e);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}
