// mlp_ep16l.h — the one-launch rollout episode (mappo_rollout_episode) with the weights in LDS and several waves per SIMD.
//
// episode16r_body (mlp_fwd16.h) keeps a network in registers: ~290 VGPRs at layer_N 1, one wave per SIMD, so every dependency of
// that wave (MFMA -> LayerNorm -> MFMA, the sampling epilogue's LDS round trips, the drain in front of the stores, the row loads)
// is paid in full.  Here a workgroup of up to 16 waves serves ONE network: it stages that network once into LDS, passes one
// workgroup barrier, and its waves then walk the network's (step, tile) items with their A operands read from LDS — the same
// 16-byte operands the register path holds (Trunk16R::w1[bo][b] = W1[16 bo + j][16 b + 4 q .. + 3], likewise w2 / wh), through
// the same tile16r_step: every MFMA sees identical operands in identical order, so the buffer stays bit-identical to the
// stepwise path's.  What a wave keeps in registers is the tile's activations and the next item's rows: 4 waves per SIMD.
//
// LDS image of one network (floats; EPL_WS = 68: rows 16 bo + j, j = 0 .. 15, of a quarter q start 4 banks apart, so one
// ds_read_b128 of 16 lanes covers the 64 banks once):
//   w1 [64][68]   row r, columns c < 16 ceil(in_dim / 16) = P[w1 + r in_dim + c] — what the register path reads, including the
//                 up to 15 floats past in_dim (the next row or the bias behind W1; they meet zero inputs)
//   g0, t0 [64]   feature-norm affine at the clamped index min(k, in_dim - 1) (no feature norm: W1's first floats, never used)
//   b1, g1, t1 [64]
//   per hidden layer l: w2 [64][68], b2, g2, t2 [64]
//   wh [16 NBH][68]  row a = P[wh + min(a, A - 1) 64 ..] (the clamped repeat rows of Head16R), bh [16 NBH] likewise
#pragma once

#define EPL_WS 68
#define EPL_MAT (HID * EPL_WS)

template <int LN>
struct EplMap {
  static constexpr int w1 = 0, g0 = w1 + EPL_MAT, t0 = g0 + HID, b1 = t0 + HID, g1 = b1 + HID, t1 = g1 + HID, hid = t1 + HID;
  static constexpr int HL = EPL_MAT + 3 * HID;                      // one hidden layer: w2, b2, g2, t2
  static constexpr int w2(int l) { return hid + l * HL; }
  static constexpr int b2(int l) { return w2(l) + EPL_MAT; }
  static constexpr int g2(int l) { return b2(l) + HID; }
  static constexpr int t2(int l) { return g2(l) + HID; }
  static constexpr int wh = hid + LN * HL, bh = wh + 32 * EPL_WS, total = bh + 32;      // (sized for the actor's two head blocks)
};

__device__ __forceinline__ f32x4 lds4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }

// lane (j, q)'s view of the staged trunk: m = image + j * EPL_WS + 4 q (matrix rows 16 bo + j), v = image + 4 q (vectors)
template <int LN>
struct Trunk16L {
  typedef EplMap<LN> Mp;
  const float *m, *v;
  __device__ __forceinline__ f32x4 W1(int bo, int b) const { return lds4(m + Mp::w1 + 16 * bo * EPL_WS + 16 * b); }
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
template <int LN, int MODE>
struct Head16L {
  static constexpr int NBH = Head16R<MODE>::NBH;
  typedef EplMap<LN> Mp;
  const float *m, *v;
  __device__ __forceinline__ f32x4 WH(int bo, int b) const { return lds4(m + Mp::wh + 16 * bo * EPL_WS + 16 * b); }
  __device__ __forceinline__ f32x4 BH(int bo) const { return lds4(v + Mp::bh + 16 * bo); }
};

// Stage one network into the image (every thread of the workgroup; the caller passes the barrier).  Matrix rows move as the
// 16-byte pieces the register path loads (4-byte aligned in global memory, 16-byte aligned in the image).
template <int LN, int NBH>
__device__ __forceinline__ void epl_stage(float *img, const float *P, const NetOff &o, const mappo_net_desc &d) {
  typedef EplMap<LN> Mp;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int D = d.in_dim, A = d.out_dim, Q1 = 4 * ((D + 15) >> 4);                 // 16-byte pieces of a W1 row
  for (int e = tid; e < HID * Q1; e += nt) {
    const int r = e / Q1, c = 4 * (e - r * Q1);
    *reinterpret_cast<f32x4 *>(img + Mp::w1 + r * EPL_WS + c) = ld4ua(P + o.w1 + (size_t)r * D + c);
  }
#pragma unroll
  for (int l = 0; l < LN; ++l)
    for (int e = tid; e < HID * 16; e += nt) {
      const int r = e >> 4, c = 4 * (e & 15);
      *reinterpret_cast<f32x4 *>(img + Mp::w2(l) + r * EPL_WS + c) = ld4ua(P + o.w2[l] + (size_t)r * HID + c);
    }
  for (int e = tid; e < 16 * NBH * 16; e += nt) {
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
    if (k < 16 * NBH) img[Mp::bh + k] = P[o.bh + min(k, A - 1)];
  }
}

// One network over a whole episode, weights in LDS: the items of episode16r_body (t * n_tiles + tile), dealt to the network's nw
// waves (wave w takes w, w + nw, ..), the next item's rows requested before the current item's math.  EVERY wave of the workgroup
// comes through here — one without an item too: it helps staging and must reach the barrier.  Rows travel as 16-byte pieces
// (ld4_row_raw / ld4_row_fix: elements 16 b + 4 q .. + 3 of the row, zeros beyond in_dim) where in_dim >= 4: trunk16r_apply
// zeroes every slot beyond in_dim before its first use, so x[b][r] is what the dword loads of episode16r_body deliver.
template <bool RELU, int LN, int MODE>
__device__ __forceinline__ void episode16l_body(const FwdArgs &p, const EpisodeSrc &s, const int M, const int n_steps, const int n_last,
                                                float *last_out, float *img, float *tZ, const int w, const int nw) {
  const int lane = threadIdx.x & (WAVE - 1), j = lane & 15, q = lane >> 4;
  const int D = p.desc.in_dim;
  const int64_t n_tiles = (p.B + 15) / 16, n_items = (int64_t)n_steps * n_tiles;
  const bool wide = D >= 4, al4 = (D & 3) == 0;
  auto load_x = [&](int64_t it, f32x4 (&xv)[4]) {
    const int t = (int)(it / n_tiles);
    const int64_t i = (it - t * n_tiles) * 16 + j;
    const int64_t row = i < p.B ? i : 0;
    const float *base = t == 0 ? s.x0 : s.xp + (int64_t)(t - 1) * s.xp_st;
    const int64_t sn = t == 0 ? s.x0_sn : s.xp_sn, sm = t == 0 ? s.x0_sm : s.xp_sm;
    const float *rp = base + (row / M) * sn + (row % M) * sm;
    if (wide) {
#pragma unroll
      for (int b = 0; b < 4; ++b) xv[b] = ld4_row_raw(rp, 16 * b + 4 * q, D);
    } else {                                                                        // in_dim < 4: features 0 .. 2 sit in (b = 0, q = 0)
#pragma unroll
      for (int r = 0; r < 3; ++r) xv[0][r] = rp[min(r, D - 1)];
    }
  };
  f32x4 xn[4] = {};
  if (w < n_items) load_x(w, xn);                                                   // the first item's rows under the staging
  epl_stage<LN, Head16R<MODE>::NBH>(img, p.params, p.off, p.desc);
  const uint64_t ctr0 = p.counter + (MODE == 1 && p.counter_dev ? *p.counter_dev : 0ull);      // read once: the word is fixed for the launch
  __syncthreads();
  const Trunk16L<LN> tw = {img + j * EPL_WS + 4 * q, img + 4 * q};
  const Head16L<LN, MODE> hd = {tw.m, tw.v};
  for (int64_t it = w; it < n_items; it += nw) {
    asm volatile("" ::: "memory");          // the image is loop-invariant: keep its reads inside the item (hoisted, they are the register body)
    const int t = (int)(it / n_tiles);
    const int64_t i = (it - t * n_tiles) * 16 + j;
    const bool ok = i < p.B;
    f32x4 x[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) x[b] = wide ? ld4_row_fix(xn[b], 16 * b + 4 * q, D, al4) : xn[b];
    if (it + nw < n_items) load_x(it + nw, xn);                                     // the next item's rows under this item's math
    const int64_t so = (int64_t)t * p.B;
    float *out = MODE == 0 ? (t == n_last ? last_out : p.out + so) : nullptr;
    tile16r_step<RELU, LN, MODE, true>(p, tw, hd, x, out, MODE == 1 ? p.actions + so : nullptr, MODE == 1 ? p.logp + so : nullptr,
                                       ctr0 + (uint64_t)t, nullptr, tZ, i, ok, j, q);
  }
}

// Workgroups [0, gA) serve the actor, [gA, gridDim.x) the critic (one workgroup per CU; the host splits them by item cost).  Within
// a network of g workgroups wave `wave` of workgroup `b` is wave number wave * g + b: the waves that get one item more than the
// rest (the first n_items mod nw) then spread evenly over the CUs, and within a CU over its SIMDs.  Every wave copies its share
// of the episode insert afterwards.  LDS: the network image, then one [16][TP] logits tile per wave.
#ifndef EPL_MAX_WAVES
#define EPL_MAX_WAVES 16
#endif
template <bool RELU, int LN>
__global__ __launch_bounds__(EPL_MAX_WAVES * WAVE) void rollout_episode_lds_kernel(EpisodeArgs e) {
  extern __shared__ __align__(16) float lds[];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), nwv = (int)(blockDim.x / WAVE);
  const int wg = (int)blockIdx.x, gA = e.wA, gC = (int)gridDim.x - gA;
  float *tZ = lds + EplMap<LN>::total + wave * 16 * TP;
  if (wg < gA) episode16l_body<RELU, LN, 1>(e.a, e.sa, e.M, e.T, -1, nullptr, lds, tZ, wave * gA + wg, gA * nwv);
  else episode16l_body<RELU, LN, 0>(e.c, e.sc, e.M, e.T + 1, e.T, e.next_values, lds, tZ, wave * gC + (wg - gA), gC * nwv);
  insert_mpe_episode_body<4>(e.ins, e.ins_obs_st, e.ins_rew_st, e.ins_done_st, e.T, wg * nwv + wave, (int)gridDim.x * nwv);
}
