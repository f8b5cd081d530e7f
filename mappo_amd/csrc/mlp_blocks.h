// mlp_blocks.h — device building blocks shared by the 32-sample-tile MLP kernels (mlp_fwd.h, mlp_upd.h, mlp_upd2.h) and, for the
// LDS map and the weight staging, by the 16-sample-tile kernels: LdsMap / lds_map*, weight staging, RowPrefetch, the LayerNorm and
// tile helpers, raw_to_grad.  Needs mlp_core.h only.
//
// The network (onpolicy/algorithms/utils/mlp.py:6-55 with its head, distributions.py:55-68 logits, r_actor_critic.py:136-165 v_out):
//
//   trunk:  x -> LN_D -> Linear(D,64) -> act -> LN_64 -> [Linear(64,64) -> act -> LN_64] x layer_N -> head
//
// Formulation of the 32-sample-tile kernels: everything is computed TRANSPOSED, Y^T[f][s] = W[f][:] . X^T[:][s], with
// v_mfma_f32_32x32x2_f32.  A wavefront owns a tile of 32 samples; in the MFMA accumulator layout a lane then holds ONE sample
// (column) and 32 of its 64 features (rows, the other 32 sit in lane^32), so bias, activation and LayerNorm are per-lane register
// loops plus one cross-half exchange — no LDS transposes, no atomics.  Weights sit in LDS for the lifetime of the workgroup
// (k-major, row stride 65/33 so that both the forward A-operand read W[f][k] (lanes <-> f) and the backward read W^T (lanes <-> k)
// are bank-conflict free); each wave keeps its activations in private LDS tiles [feature][sample] (row stride 33), which serve as
// B operand of the next layer (lanes <-> sample) and, read transposed (lanes <-> feature, k <-> sample), as both operands of the
// weight-gradient products.  A tile stores the NORMALISED value xhat = (a - mean) * rstd of its LayerNorm; the affine (gamma, beta)
// is applied when the tile is read as an operand (two broadcast LDS reads + one FMA per MFMA pair), so the backward pass finds
// xhat in the tile and only mean/rstd/sign-mask (3 registers) survive from the forward.
//
// Which kernel family serves which shape (hidden == 64, out_dim <= 32, layer_N <= 2, in_dim <= 2048):
//
//   forward   mlp_forward_kernel (mlp_fwd.h)                    in_dim <= 64: mappo_mlp_forward / mappo_actor_act
//             features16 / rollout step / episode (mlp_fwd16.h) in_dim <= 64, weights in registers, 16-sample tiles
//             wide_forward16* (mlp_wide16.h)                    in_dim 65..512
//             wide_forward_sliced (mlp_wide_sliced.h)           in_dim 513..2048
//   update    upd16   one wave per 16-sample tile (mlp_upd16.h)     in_dim <= 64, layer_N <= 1, actor out_dim <= 16, LDS layout fits
//             upd16x  the same from z1 on, layer 1 in mlp_wide16.h  in_dim 65..512, layer_N <= 1, actor out_dim <= 16
//                     (in_dim 513..2048: layer 1 in mlp_wide_sliced.h)
//             upd2    pair kernel (mlp_upd2.h)                      in_dim <= 64 otherwise
//             wide    K-chunked kernel (mlp_upd.h)                  in_dim 65..2048 otherwise (layer_N = 2, external head gradient)
//   The dual launch takes upd16d (both networks upd16) or upd2d (the pair kernel for both).  The dispatch itself is launch_update
//   and mappo_actor_critic_update in mlp.hip; the limits and the cross-unit launchers are declared in mlp_launch.h.
#pragma once
#include "mlp_core.h"

// ------------------------------------------------------------------------------------------------
// LDS carve-up (floats); every region starts on a 16-byte boundary.  Dp = in_dim rounded up to even.
// Per wave: tX [Dp rows] | tH [(layer_N+1) x 64 rows] | tZ [32 rows: head output / head gradient as [s][a]].
// ------------------------------------------------------------------------------------------------
struct LdsMap {
  int w1, w2[MAPPO_MAX_LAYER_N], wh;
  int fn_w, fn_b, b1, ln1_w, ln1_b, b2[MAPPO_MAX_LAYER_N], ln2_w[MAPPO_MAX_LAYER_N], ln2_b[MAPPO_MAX_LAYER_N], bh;
  int scratch;       // n_waves x 192 floats: exchange buffers / epilogue scratch of the update kernels
  int tiles, x_rows, wave_stride, total;
  int fn_size;       // floats reserved per feature-norm vector (64, or in_dim rounded up to 64 for wide inputs)
};


__host__ __device__ inline LdsMap lds_map(const mappo_net_desc &d, int n_waves) {
  LdsMap m;
  int p = 0;
  const bool xw = d.in_dim > MAXD;
  const int Dp = xw ? MAXD : ((d.in_dim + 1) & ~1);          // wide inputs: one 64-column chunk of W1 / of the rows at a time
  m.fn_size = xw ? ((d.in_dim + 63) / 64) * 64 : MAXD;
  m.w1 = p; p = al4(p + Dp * WP);
  for (int l = 0; l < MAPPO_MAX_LAYER_N; ++l) { m.w2[l] = p; if (l < d.layer_N) p = al4(p + HID * WP); }
  m.wh = p; p = al4(p + HID * HP);
  m.fn_w = p; p += m.fn_size; m.fn_b = p; p += m.fn_size;
  m.b1 = p; p += HID; m.ln1_w = p; p += HID; m.ln1_b = p; p += HID;
  for (int l = 0; l < MAPPO_MAX_LAYER_N; ++l) {
    m.b2[l] = p; m.ln2_w[l] = p; m.ln2_b[l] = p;
    if (l < d.layer_N) { m.b2[l] = p; p += HID; m.ln2_w[l] = p; p += HID; m.ln2_b[l] = p; p += HID; }
  }
  m.bh = p; p += 32;
  m.scratch = p; p += n_waves * 192;           // update kernels: exchange buffers + epilogue scratch
  m.tiles = p;
  m.x_rows = Dp;
  m.wave_stride = al4((Dp + (d.layer_N + 1) * HID + TS) * TP);
  p += n_waves * m.wave_stride;
  m.total = p;
  return m;
}

// The part of the map the register-resident tail (mlp_fwd16.h: forward16_tail after stage_tail_1shot) reads — no W1 chunk area, no
// feature-norm vectors, no per-wave tiles: what a kernel that keeps W1' elsewhere in LDS puts behind it (wide_features16_resident_kernel).
__host__ __device__ inline LdsMap lds_map_tail(const mappo_net_desc &d) {
  LdsMap m = lds_map(d, 1);
  int p = 0;
  m.w1 = 0; m.fn_w = 0; m.fn_b = 0; m.fn_size = 0;
  for (int l = 0; l < MAPPO_MAX_LAYER_N; ++l) { m.w2[l] = p; if (l < d.layer_N) p = al4(p + HID * WP); }
  m.wh = p; p = al4(p + HID * HP);
  m.b1 = p; p += HID; m.ln1_w = p; p += HID; m.ln1_b = p; p += HID;
  for (int l = 0; l < MAPPO_MAX_LAYER_N; ++l) {
    m.b2[l] = p; m.ln2_w[l] = p; m.ln2_b[l] = p;
    if (l < d.layer_N) { m.b2[l] = p; p += HID; m.ln2_w[l] = p; p += HID; m.ln2_b[l] = p; p += HID; }
  }
  m.bh = p; p += 32;
  m.scratch = p;
  m.tiles = p;
  m.wave_stride = 0;
  m.total = p;
  return m;
}

// Workgroup-cooperative staging of one weight matrix: global W[f][k] (row-major, K columns) -> LDS dst[k*stride + f],
// rows k in [K, Kpad) zeroed.  Loads are UNCONDITIONAL (clamped index) and all issued before the first LDS write, so a
// thread pays one memory latency for its whole share (a predicated load is waited for individually by hipcc).
__device__ __forceinline__ void stage_weight_T(float *dst, const float *__restrict__ src, int F, int K, int Kpad, int stride) {
  const int total = F * K;
  const int nthr = blockDim.x, tid = threadIdx.x;
  if ((((uintptr_t)src) & 15) == 0 && (total & 3) == 0) {
    const int n4 = total >> 2;
    for (int i0 = 0; i0 < n4; i0 += 8 * nthr) {
      float4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = reinterpret_cast<const float4 *>(src)[min(i0 + j * nthr + tid, n4 - 1)];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + j * nthr + tid;
        if (i < n4) {
          const int e = i << 2;
          int f = e / K, k = e - f * K;
          const float vv[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            dst[k * stride + f] = vv[c];
            if (++k == K) { k = 0; ++f; }
          }
        }
      }
    }
  } else {
    for (int e0 = 0; e0 < total; e0 += 8 * nthr) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[min(e0 + j * nthr + tid, total - 1)];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int e = e0 + j * nthr + tid;
        if (e < total) { const int f = e / K; dst[(e - f * K) * stride + f] = v[j]; }
      }
    }
  }
  for (int e = tid; e < F * (Kpad - K); e += nthr) {
    const int f = e % F, k = K + e / F;
    dst[k * stride + f] = 0.f;
  }
}

// All per-feature vectors of the network in ONE pass: element e of the concatenated LDS vector area
// [fn_w 64 | fn_b 64 | b1 ln1_w ln1_b | (b2 ln2_w ln2_b) x LN | bh 32] maps to a global offset or a fill value.
template <int LN>
__device__ __forceinline__ void stage_vectors(float *lds, const LdsMap &m, const float *__restrict__ params, const NetOff &o,
                                              const mappo_net_desc &d) {
  const int D = d.in_dim, A = d.out_dim;
  const int FN = m.fn_size;
  const int n_total = 2 * FN + 3 * HID * (1 + LN) + 32;
  const int nthr = blockDim.x, tid = threadIdx.x;
  for (int e0 = 0; e0 < n_total; e0 += 4 * nthr) {
    float v[4]; int dsti[4]; bool wr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = e0 + j * nthr + tid;
      int src = -1; float fill = 0.f; int dst = m.fn_w;
      wr[j] = e < n_total;
      if (e < FN) { dst = m.fn_w + e; if (d.use_feature_norm) { if (e < D) src = o.fn_w + e; } else fill = e < D ? 1.f : 0.f; }
      else if (e < 2 * FN) { const int i = e - FN; dst = m.fn_b + i; if (d.use_feature_norm && i < D) src = o.fn_b + i; }
      else if (e < 2 * FN + 3 * HID) { const int i = e - 2 * FN; dst = m.b1 + i; src = o.b1 + i; }
      else if (e < 2 * FN + 3 * HID * (1 + LN)) {
        const int i = e - 2 * FN - 3 * HID, l = i / (3 * HID), r = i - l * 3 * HID;
        dst = (l == 0 ? m.b2[0] : m.b2[LN > 1 ? 1 : 0]) + r;
        src = (l == 0 ? o.b2[0] : o.b2[LN > 1 ? 1 : 0]) + r;
      } else { const int i = e - 2 * FN - 3 * HID * (1 + LN); dst = m.bh + i; if (i < A) src = o.bh + i; }
      const float ld = params[src >= 0 ? src : 0];        // unconditional load, selected below
      v[j] = src >= 0 ? ld : fill;
      dsti[j] = dst;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) if (wr[j]) lds[dsti[j]] = v[j];
  }
}

template <int LN>
__device__ __forceinline__ void stage_all_weights(float *lds, const LdsMap &m, const float *__restrict__ params,
                                                  const NetOff &o, const mappo_net_desc &d) {
  const int D = d.in_dim, Dp = (D + 1) & ~1, A = d.out_dim;
  stage_vectors<LN>(lds, m, params, o, d);
  if (D <= MAXD) stage_weight_T(lds + m.w1, params + o.w1, HID, D, Dp, WP);      // wide inputs stream W1 chunk by chunk
#pragma unroll
  for (int l = 0; l < LN; ++l) stage_weight_T(lds + m.w2[l], params + o.w2[l], HID, HID, HID, WP);
  // head: dst[k*HP + a] = Wh[a][k]; columns a >= A are zero
  {
    const int nthr = blockDim.x, tid = threadIdx.x, total = HID * 32, real = A * HID;
    for (int e0 = 0; e0 < total; e0 += 8 * nthr) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = params[o.wh + min(e0 + j * nthr + tid, real - 1)];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int e = e0 + j * nthr + tid;
        if (e < total) { const int a = e >> 6, k = e & 63; lds[m.wh + k * HP + a] = (e < real) ? v[j] : 0.f; }
      }
    }
  }
}

// One-shot variant for in_dim <= 64 and >= 256 threads: EVERY global load of the staging (vectors, W1, W2.., head) is
// issued before the first LDS store, so a thread pays one memory latency for the whole network instead of one per
// matrix (four to five dependent L2 / Infinity-Cache round trips otherwise — a large part of a rollout-sized launch).
// Falls back to stage_all_weights when the float4 views are not available (odd in_dim, unaligned params, small block).
template <int LN>
__device__ __forceinline__ void stage_all_weights_1shot(float *lds, const LdsMap &m, const float *__restrict__ params,
                                                        const NetOff &o, const mappo_net_desc &d) {
  const int D = d.in_dim, Dp = (D + 1) & ~1, A = d.out_dim;
  const int nthr = blockDim.x, tid = threadIdx.x;
  const int FN = m.fn_size;
  const int n_vec = 2 * FN + 3 * HID * (1 + LN) + 32;
  if (nthr < 256 || (D & 1) || D > MAXD || ((((uintptr_t)params) & 15) != 0) || n_vec > 4 * nthr) {
    stage_all_weights<LN>(lds, m, params, o, d);
    return;
  }
  // ---- loads ----
  const float4 *g1 = reinterpret_cast<const float4 *>(params + o.w1), *gh = reinterpret_cast<const float4 *>(params + o.wh);
  const int n4_1 = 16 * D, n4_h = 16 * A;
  float4 w1v[4], w2v[LN > 0 ? LN : 1][4], whv[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) w1v[j] = g1[min(j * nthr + tid, n4_1 - 1)];
#pragma unroll
  for (int l = 0; l < LN; ++l) {
    const float4 *g2 = reinterpret_cast<const float4 *>(params + o.w2[l]);
#pragma unroll
    for (int j = 0; j < 4; ++j) w2v[l][j] = g2[min(j * nthr + tid, 1023)];
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) whv[j] = gh[min(j * nthr + tid, n4_h - 1)];
  float vv[4]; int vdst[4]; bool vwr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = j * nthr + tid;
    int src = -1; float fill = 0.f; int dst = m.fn_w;
    vwr[j] = e < n_vec;
    if (e < FN) { dst = m.fn_w + e; if (d.use_feature_norm) { if (e < D) src = o.fn_w + e; } else fill = e < D ? 1.f : 0.f; }
    else if (e < 2 * FN) { const int i = e - FN; dst = m.fn_b + i; if (d.use_feature_norm && i < D) src = o.fn_b + i; }
    else if (e < 2 * FN + 3 * HID) { const int i = e - 2 * FN; dst = m.b1 + i; src = o.b1 + i; }
    else if (e < 2 * FN + 3 * HID * (1 + LN)) {
      const int i = e - 2 * FN - 3 * HID, l = i / (3 * HID), r = i - l * 3 * HID;
      dst = (l == 0 ? m.b2[0] : m.b2[LN > 1 ? 1 : 0]) + r;
      src = (l == 0 ? o.b2[0] : o.b2[LN > 1 ? 1 : 0]) + r;
    } else { const int i = e - 2 * FN - 3 * HID * (1 + LN); dst = m.bh + i; if (i < A) src = o.bh + i; }
    const float ld = params[src >= 0 ? src : 0];
    vv[j] = src >= 0 ? ld : fill;
    vdst[j] = dst;
  }
  // ---- stores ----
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = j * nthr + tid;
    if (i < n4_1) {
      const int e = i << 2;
      int f = e / D, k = e - f * D;
      const float t[4] = {w1v[j].x, w1v[j].y, w1v[j].z, w1v[j].w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        lds[m.w1 + k * WP + f] = t[c];
        if (++k == D) { k = 0; ++f; }
      }
    }
  }
  for (int e = tid; e < HID * (Dp - D); e += nthr) lds[m.w1 + (D + e / HID) * WP + (e % HID)] = 0.f;
#pragma unroll
  for (int l = 0; l < LN; ++l)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = j * nthr + tid;
      if (i < 1024) {
        const int e = i << 2, f = e >> 6, k = e & 63;
        float *q = lds + m.w2[l] + k * WP + f;
        q[0] = w2v[l][j].x; q[WP] = w2v[l][j].y; q[2 * WP] = w2v[l][j].z; q[3 * WP] = w2v[l][j].w;
      }
    }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = j * nthr + tid;
    if (i < n4_h) {
      const int e = i << 2, a = e >> 6, k = e & 63;
      float *q = lds + m.wh + k * HP + a;
      q[0] = whv[j].x; q[HP] = whv[j].y; q[2 * HP] = whv[j].z; q[3 * HP] = whv[j].w;
    }
  }
  for (int e = tid; e < HID * (32 - A); e += nthr) { const int k = e / (32 - A), a = A + e - k * (32 - A); lds[m.wh + k * HP + a] = 0.f; }
#pragma unroll
  for (int j = 0; j < 4; ++j) if (vwr[j]) lds[vdst[j]] = vv[j];
}

// ------------------------------------------------------------------------------------------------
// input rows.  Lane (s = lane & 31, half = lane >> 5) fetches features k = 2j + half of sample s of the NEXT tile
// into registers (NV = ceil(D/2) <= 16 | 32); at the top of the tile the LayerNorm over the D input features
// (mlp.py:45,51-52) is a per-lane register loop plus one cross-half exchange, and xhat0 goes to tX[k][s] in the
// layout the B operand of layer 1 reads.  (A wave load touches 32 rows, one word each; the rows of a tile are
// re-touched by the next j while still in L1.)
// ------------------------------------------------------------------------------------------------
template <bool WIDE>
struct RowPrefetch {
  float v[WIDE ? TS : TS / 2];
  int my_row;         // source row of sample lane&31 of the prefetched tile (both halves hold it)
  int n_valid;
  bool flat;          // v holds the float4 chunks 4*(lane + 64 j) of the tile's contiguous [32][D] block (see below)
};

// Two fetch modes.  Gather (any row list, partial tiles, odd D): lane (s, half) loads x[row_s][2j + half] — every wave
// load touches 32 rows, one word each.  Flat (rows == nullptr, full tile, even D, 16-B aligned x): the tile is one
// contiguous block of 32*D floats, fetched as fully coalesced float4s (8x fewer cache lines touched per instruction);
// commit_rows then routes it through an LDS staging area to reach the lane <-> sample layout.
template <bool WIDE>
__device__ __forceinline__ void prefetch_rows(RowPrefetch<WIDE> &pf, const float *__restrict__ x,
                                              const int32_t *__restrict__ rows, int64_t base, int64_t B, int D, int lane,
                                              int64_t x_sn = 0, int64_t x_sm = 0, int x_M = 0) {
  const int s = lane & 31, half = lane >> 5;
  pf.n_valid = (int)max((int64_t)0, min((int64_t)TS, B - base));
  pf.my_row = 0;
  const bool ok = s < pf.n_valid;
  if (ok) pf.my_row = rows ? rows[base + s] : (int)(base + s);
  constexpr int NV = WIDE ? TS : TS / 2;
  pf.flat = rows == nullptr && x_M == 0 && pf.n_valid == TS && (D & 1) == 0 && (((uintptr_t)x) & 15) == 0;
  if (pf.flat) {
    const float4 *src4 = reinterpret_cast<const float4 *>(x + base * D);
    const int n4 = TS * D / 4;
#pragma unroll
    for (int j = 0; j < NV / 4; ++j) {
      const float4 q = src4[min(lane + 64 * j, n4 - 1)];
      pf.v[4 * j + 0] = q.x; pf.v[4 * j + 1] = q.y; pf.v[4 * j + 2] = q.z; pf.v[4 * j + 3] = q.w;
    }
    return;
  }
  const int64_t row_off = x_M ? (int64_t)(pf.my_row / x_M) * x_sn + (int64_t)(pf.my_row % x_M) * x_sm : (int64_t)pf.my_row * D;
  const float *src = x + row_off + half;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    pf.v[j] = 0.f;
    if (ok && 2 * j + half < D) pf.v[j] = src[2 * j];
  }
}

// tX[k][s] <- xhat0 (feature LayerNorm, affine applied on read) or the raw input when feature norm is off, for ALL
// k < 2*NV: rows k >= D receive a finite filler (they spill into the activation tiles, dead at this point); nothing
// reads them with a non-zero weight (W1's padding rows are zero, gradient columns k >= D are dropped).  Writing them
// unconditionally keeps 32 loop-invariant lane predicates out of the tile loop (hipcc hoists each into an SGPR pair
// and then spills them).
// tF: >= 32*(D+2) floats of wave-private LDS that are dead at this point (the activation tiles), staging of the flat mode.
// magic = 2^32 / D + 1 (flat mode: e / D == umulhi(e, magic) for the small e used here).
template <bool WIDE>
__device__ __forceinline__ void commit_rows(float *tX, float *tF, const RowPrefetch<WIDE> &pf, int D, uint32_t magic, int lane,
                                            bool feature_norm) {
  const int s = lane & 31, half = lane >> 5;
  constexpr int NV = WIDE ? TS : TS / 2;
  float v[NV];
  if (pf.flat) {
    // row stride D when D = 2 (mod 4) (lanes (s, half) then read 64 distinct banks), D + 2 when D = 0 (mod 4)
    const bool pad = (D & 3) == 0;
    const int stride = pad ? D + 2 : D;
#pragma unroll
    for (int j = 0; j < NV / 4; ++j) {
      const int e4 = 4 * (lane + 64 * j);
      if (e4 < TS * D) {
        if (!pad) {
          *reinterpret_cast<float4 *>(tF + e4) = make_float4(pf.v[4 * j], pf.v[4 * j + 1], pf.v[4 * j + 2], pf.v[4 * j + 3]);
        } else {
          const int r = (int)__umulhi((uint32_t)e4, magic), k = e4 - r * D;
          float2 *q = reinterpret_cast<float2 *>(tF + r * stride + k);
          q[0] = make_float2(pf.v[4 * j], pf.v[4 * j + 1]);
          q[1] = make_float2(pf.v[4 * j + 2], pf.v[4 * j + 3]);
        }
      }
    }
    wave_lds_sync();
    const float *rowp = tF + s * stride + half;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      v[j] = 0.f;
      if (2 * j < D) v[j] = rowp[2 * j];           // D is even here: the bound is wave-uniform (scalar branch, no lane mask)
    }
  } else {
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = pf.v[j];   // slots beyond D hold 0
  }
  float mean = 0.f, rstd = 1.f;
  if (feature_norm) {
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) sum += v[j];
    mean = xhalf_sum(sum) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) { const float c = v[j] - mean; q += c * c; }
    // the NV - ceil((D - half)/2) empty slots of this lane each added (0 - mean)^2: take them out again
    const int n_empty = NV - ((D - half + 1) >> 1);
    q -= (float)n_empty * mean * mean;
    rstd = 1.0f / sqrtf(fmaxf(xhalf_sum(q), 0.f) / (float)D + LN_EPS);
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) tX[(2 * j + half) * TP + s] = (v[j] - mean) * rstd;
}

// ---- wide inputs (in_dim > 64) ----
// 64 columns [c0, c0+kc) of W1[64][D] -> sW[kk*WP + f]; rows kk in [kc, 64) zeroed.  Workgroup-cooperative, batched loads.
__device__ __forceinline__ void stage_w1_chunk(float *dst, const float *__restrict__ w1, int D, int c0, int kc) {
  const int nthr = blockDim.x, tid = threadIdx.x, total = HID * kc;
  for (int e0 = 0; e0 < total; e0 += 8 * nthr) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = min(e0 + j * nthr + tid, total - 1);
      const int f = e / kc, kk = e - f * kc;
      v[j] = w1[f * D + c0 + kk];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = e0 + j * nthr + tid;
      if (e < total) { const int f = e / kc; dst[(e - f * kc) * WP + f] = v[j]; }
    }
  }
  for (int e = tid; e < HID * (MAXD - kc); e += nthr) dst[(kc + e / HID) * WP + (e % HID)] = 0.f;
}

// LayerNorm statistics of a full input row (two passes over the row, which stays in L1/L2 between them)
__device__ __forceinline__ void wide_row_stats(const float *__restrict__ xr, int D, bool ok, int half, bool feature_norm, float &mean,
                                               float &rstd) {
  mean = 0.f; rstd = 1.f;
  if (!feature_norm) return;
  // unconditional loads (a lane without a row reads row 0: finite values nobody uses) and eight of them in flight per trip:
  // as a predicated one-load-per-trip loop the two passes cost ~160 memory round trips each
  float s0 = 0.f;
#pragma unroll 8
  for (int k = half; k < D; k += 2) s0 += xr[k];
  mean = xhalf_sum(s0) / (float)D;
  float q = 0.f;
#pragma unroll 8
  for (int k = half; k < D; k += 2) { const float c = xr[k] - mean; q += c * c; }
  rstd = 1.0f / sqrtf(xhalf_sum(q) / (float)D + LN_EPS);
}

// tX[kk][s] <- xhat0 of columns [c0, c0+64) of this lane's row
__device__ __forceinline__ void wide_commit_chunk(float *tX, const float *__restrict__ xr, int D, int c0, bool ok, float mean, float rstd,
                                                  int l31, int half) {
  float v[TS];
#pragma unroll
  for (int j = 0; j < TS; ++j) v[j] = xr[min(c0 + 2 * j + half, D - 1)];          // unconditional, clamped: all 32 in flight
#pragma unroll
  for (int j = 0; j < TS; ++j) {
    const int k = c0 + 2 * j + half;
    tX[(2 * j + half) * TP + l31] = (ok && k < D) ? (v[j] - mean) * rstd : 0.f;   // padding columns / rows contribute 0
  }
}

// acc (2 tiles of 32 features) <- bias
__device__ __forceinline__ void init_bias(f32x16 (&acc)[2], const float *sB, int half) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 b = vec4_of(sB, t, q, half);
      acc[t][4 * q + 0] = b.x; acc[t][4 * q + 1] = b.y; acc[t][4 * q + 2] = b.z; acc[t][4 * q + 3] = b.w;
    }
}

// act + LayerNorm(64) statistics in the accumulator layout.  On return acc holds a = act(z).
template <bool RELU>
__device__ __forceinline__ void act_ln_stats(f32x16 (&acc)[2], float &mean, float &rstd) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[t][r] = act_fwd<RELU>(acc[t][r]); s += acc[t][r]; }
  mean = xhalf_sum(s) * (1.f / HID);
  float q = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { const float c = acc[t][r] - mean; q += c * c; }
  rstd = 1.0f / sqrtf(xhalf_sum(q) * (1.f / HID) + LN_EPS);
}

// tile[f][s] <- xhat = (a - mean) * rstd   (the LayerNorm affine is applied by whoever reads the tile)
__device__ __forceinline__ void xhat_to_tile(float *tile, const f32x16 (&a)[2], float mean, float rstd, int l31, int half) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[(32 * t + ROWMAP(r, half)) * TP + l31] = (a[t][r] - mean) * rstd;
}

// acc[t] += W-tile . (tin * gamma + beta)   (forward layer; weights k-major in LDS, K = 2*ksteps); operands of
// step kk+1 are fetched from LDS before the MFMAs of step kk issue
__device__ __forceinline__ void layer_mfma(f32x16 (&acc)[2], const float *sW, const float *tin, const float *sG,
                                           const float *sBt, int ksteps, int l31, int half) {
  // unrolled so that hipcc issues the LDS reads of several k-steps ahead of the MFMA chain that consumes them
#pragma unroll 8
  for (int kk = 0; kk < ksteps; ++kk) {
    const int k = 2 * kk + half;
    const float b = tin[k * TP + l31] * sG[k] + sBt[k];
    const float a0 = sW[k * WP + l31], a1 = sW[k * WP + 32 + l31];
    acc[0] = mfma(a0, b, acc[0]);
    acc[1] = mfma(a1, b, acc[1]);
  }
}

template <int LN>
struct TileStats {
  float mean[LN + 1], rstd[LN + 1];
  uint32_t pos[LN + 1];   // bit (16*t + r): post-activation value > 0 (exact ReLU gate for the backward pass)
};

__device__ __forceinline__ uint32_t positive_mask(const f32x16 (&a)[2]) {
  uint32_t mk = 0u;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) mk |= (a[t][r] > 0.f ? 1u : 0u) << (16 * t + r);
  return mk;
}

// LayerNorm affine parameters (LDS offsets) of the tile that feeds hidden layer l / the head
template <int LN>
__device__ __forceinline__ int ln_w_of(const LdsMap &m, int l) { return l == 0 ? m.ln1_w : m.ln2_w[l - 1]; }
template <int LN>
__device__ __forceinline__ int ln_b_of(const LdsMap &m, int l) { return l == 0 ? m.ln1_b : m.ln2_b[l - 1]; }

// forward of one 32-sample tile: tX (xhat0) -> tH[0..LN] (xhat of every LayerNorm); statistics kept for backward
template <bool RELU, int LN>
__device__ __forceinline__ void tile_forward_rest(const float *lds, const LdsMap &m, float *tH, f32x16 (&acc)[2], int l31, int half,
                                                  TileStats<LN> &st);

template <bool RELU, int LN>
__device__ __forceinline__ void tile_forward(const float *lds, const LdsMap &m, float *tX, float *tH, int D, int l31, int half,
                                             TileStats<LN> &st) {
  const int Dp = (D + 1) & ~1;
  f32x16 acc[2];
  init_bias(acc, lds + m.b1, half);
  layer_mfma(acc, lds + m.w1, tX, lds + m.fn_w, lds + m.fn_b, Dp / 2, l31, half);
  tile_forward_rest<RELU, LN>(lds, m, tH, acc, l31, half, st);
}

// wide inputs: layer 1 accumulated over 64-column chunks; every wave of the workgroup must call this the same
// number of times (block barriers around the shared W1 chunk)
template <bool RELU, int LN>
__device__ __forceinline__ void tile_forward_wide(float *lds, const LdsMap &m, const float *__restrict__ w1, const float *__restrict__ xr,
                                                  bool ok, float mean0, float rstd0, float *tX, float *tH, int D, int l31, int half,
                                                  TileStats<LN> &st) {
  f32x16 acc[2];
  init_bias(acc, lds + m.b1, half);
  for (int c0 = 0; c0 < D; c0 += MAXD) {
    const int kc = min(MAXD, D - c0);
    __syncthreads();                                   // the previous chunk of W1 is no longer being read
    stage_w1_chunk(lds + m.w1, w1, D, c0, kc);
    wide_commit_chunk(tX, xr, D, c0, ok, mean0, rstd0, l31, half);
    __syncthreads();
    layer_mfma(acc, lds + m.w1, tX, lds + m.fn_w + c0, lds + m.fn_b + c0, (kc + 1) / 2, l31, half);
  }
  tile_forward_rest<RELU, LN>(lds, m, tH, acc, l31, half, st);
}

template <bool RELU, int LN>
__device__ __forceinline__ void tile_forward_rest(const float *lds, const LdsMap &m, float *tH, f32x16 (&acc)[2], int l31, int half,
                                                  TileStats<LN> &st) {
  act_ln_stats<RELU>(acc, st.mean[0], st.rstd[0]);
  st.pos[0] = positive_mask(acc);
  xhat_to_tile(tH, acc, st.mean[0], st.rstd[0], l31, half);
  wave_lds_sync();
#pragma unroll
  for (int l = 0; l < LN; ++l) {
    init_bias(acc, lds + m.b2[l], half);
    layer_mfma(acc, lds + m.w2[l], tH + l * HID * TP, lds + ln_w_of<LN>(m, l), lds + ln_b_of<LN>(m, l), HID / 2, l31, half);
    act_ln_stats<RELU>(acc, st.mean[l + 1], st.rstd[l + 1]);
    st.pos[l + 1] = positive_mask(acc);
    xhat_to_tile(tH + (l + 1) * HID * TP, acc, st.mean[l + 1], st.rstd[l + 1], l31, half);
    wave_lds_sync();
  }
}

// head: out^T[a][s] (a < 32) = Wh . h_last + bh, accumulator layout
__device__ __forceinline__ f32x16 head_forward(const float *lds, const LdsMap &m, const float *tLast, const float *sG,
                                               const float *sBt, int l31, int half) {
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 b = *reinterpret_cast<const float4 *>(lds + m.bh + 8 * q + 4 * half);
    acc[4 * q + 0] = b.x; acc[4 * q + 1] = b.y; acc[4 * q + 2] = b.z; acc[4 * q + 3] = b.w;
  }
  const float *sW = lds + m.wh;
#pragma unroll 16
  for (int kk = 0; kk < HID / 2; ++kk) {
    const int k = 2 * kk + half;
    acc = mfma(sW[k * HP + l31], tLast[k * TP + l31] * sG[k] + sBt[k], acc);
  }
  return acc;
}

// sum over the 32 samples of row `f` (= lane) of a [64][TP] tile
__device__ __forceinline__ float tile_row_sum(const float *tile, int lane) {
  float s0 = 0.f, s1 = 0.f;
#pragma unroll 4
  for (int j = 0; j < TS; j += 2) { s0 += tile[lane * TP + j]; s1 += tile[lane * TP + j + 1]; }
  return s0 + s1;
}

__device__ __forceinline__ void regs_to_tile(float *tile, const f32x16 (&v)[2], int l31, int half) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[(32 * t + ROWMAP(r, half)) * TP + l31] = v[t][r];
}

// LayerNorm + activation backward in the accumulator layout.
//   in : dH = d/d(h) with h = xhat*gamma + beta the LayerNorm output; `tile` holds xhat
//   out: dH <- d/d(z) (pre-activation), also written over `tile` (each lane rewrites exactly the words it read)
// AFFINE = false (every LayerNorm that feeds a weight matrix of this kernel): the LayerNorm weight/bias gradients
// are NOT accumulated here — they follow from the raw products G = dz_next . xhat^T the dW MFMAs accumulate anyway
// (d gamma[k] = sum_f W_next[f][k] G[f][k], d beta[k] = sum_f W_next[f][k] db_next[f]; see the epilogue).
// AFFINE = true (HEAD 3: the gradient arrives at the trunk output, no weight matrix behind it): gG/gB (lane =
// feature) += sum_s dy*xhat, sum_s dy through two transposed row sums.
template <bool RELU, bool AFFINE>
__device__ __forceinline__ void ln_act_backward(f32x16 (&dH)[2], float *tile, float mean, float rstd, uint32_t pos,
                                                const float *sG, float &gG, float &gB, int lane, int l31, int half) {
  f32x16 xh[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) xh[t][r] = tile[(32 * t + ROWMAP(r, half)) * TP + l31];
  if (AFFINE) {
    wave_lds_sync();
    regs_to_tile(tile, dH, l31, half);
    wave_lds_sync();
    gB += tile_row_sum(tile, lane);
    wave_lds_sync();
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) tile[(32 * t + ROWMAP(r, half)) * TP + l31] = dH[t][r] * xh[t][r];
    wave_lds_sync();
    gG += tile_row_sum(tile, lane);
    wave_lds_sync();
  }
  float m1 = 0.f, m2 = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 g4 = vec4_of(sG, t, q, half);
      const float gq[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int r = 4 * q + c;
        const float dxh = dH[t][r] * gq[c];
        dH[t][r] = dxh;
        m1 += dxh;
        m2 += dxh * xh[t][r];
      }
    }
  m1 = xhalf_sum(m1) * (1.f / HID);
  m2 = xhalf_sum(m2) * (1.f / HID);
  const float inv_rstd = 1.0f / rstd;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float da = rstd * (dH[t][r] - m1 - xh[t][r] * m2);
      if (RELU) {
        dH[t][r] = ((pos >> (16 * t + r)) & 1u) ? da : 0.f;          // exact gate saved by the forward
      } else {
        const float a = xh[t][r] * inv_rstd + mean;                  // tanh output recovered from xhat
        dH[t][r] = da * (1.f - a * a);
      }
    }
  regs_to_tile(tile, dH, l31, half);
  wave_lds_sync();
}

// Epilogue of the update kernel, per wave and in registers: raw products -> gradient partials.
// With h_in = xhat_in*gamma + beta feeding z = W h_in + b,  G[f][k] = sum_s dz[f][s] xhat_in[k][s],  db[f] = sum_s dz[f][s]:
//   dW[f][k] = gamma[k] G[f][k] + beta[k] db[f]      d gamma[k] = sum_f W[f][k] G[f][k]      d beta[k] = sum_f W[f][k] db[f]
// (linear in G and db, so applying them to each wave's partial sums commutes with the reductions that follow).
// g[ti][tj]: accumulator tiles, rows f = 32 ti + ROWMAP(r, half), columns k = 32 tj + l31.  dbv: db, lane = f.
// sW: the consumer's weights in LDS, k-major (sW[k*wstride + f]).  On return g holds dW, dgam/dbet (lane = k) the affine grads.
template <int NTI>
__device__ __forceinline__ void raw_to_grad(f32x16 (&g)[NTI][2], float dbv, float *scr, const float *sW, int wstride, const float *sG,
                                            const float *sBt, int K, bool two_k_tiles, int lane, int l31, int half, float &dgam,
                                            float &dbet) {
  scr[lane] = dbv;
  wave_lds_sync();
  float dg[2] = {0.f, 0.f}, dt[2] = {0.f, 0.f};
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    if (tj == 1 && !two_k_tiles) break;
    const int k = 32 * tj + l31;
    const bool valid = k < K;
    const int kc = valid ? k : 0;
    const float gam = valid ? sG[kc] : 0.f, bet = valid ? sBt[kc] : 0.f;
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti) {
      float w[16], d[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) { const int f = 32 * ti + ROWMAP(r, half); w[r] = sW[kc * wstride + f]; d[r] = scr[f]; }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float wv = valid ? w[r] : 0.f;
        dg[tj] += wv * g[ti][tj][r];
        dt[tj] += wv * d[r];
        g[ti][tj][r] = gam * g[ti][tj][r] + bet * d[r];
      }
    }
  }
  const float a0 = xhalf_sum(dg[0]), a1 = xhalf_sum(dg[1]), b0 = xhalf_sum(dt[0]), b1 = xhalf_sum(dt[1]);
  dgam = half ? a1 : a0;
  dbet = half ? b1 : b0;
  wave_lds_sync();
}
