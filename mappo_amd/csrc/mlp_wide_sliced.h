// mlp_wide_sliced.h — layer 1 of the MLP trunk for inputs wider than the tuned wide kernels take (in_dim 513..2048: SMAC critics
// on concatenated observations, stacked frames, the agent-specific state of the large maps), on v_mfma_f32_16x16x4_f32.
//
// The kernels of mlp_wide16.h are shaped by 512 columns: wide_l1_fwd16_kernel stages W1' whole in LDS (132 KB at 512), every
// forward keeps a sample's whole row in registers (128 VGPRs at 512), wide_l1_bwd16_kernel deals the gradient's 64-column chunks
// over the 8 waves of a workgroup.  None of that scales, and none of it is touched: widths up to 512 keep those kernels.  Here
//   * sliced_layer1 walks ALL ceil(in_dim / 64) column chunks with 16 + 2 x 16 registers per lane: W1' (gamma folded in) streams
//     through the double-buffered [64][68] LDS tile of wide16_layer1, the row's chunk c + 1 and the weights' chunk c + 1 are
//     fetched under the 64 MFMAs of chunk c, one barrier per chunk;
//   * the feature-norm statistics cannot come out of a slice (mean and rstd run over the whole row), and the forward entry points
//     (mappo_mlp_forward, mappo_actor_act, mappo_mlp_features) have no workspace a separate statistics kernel could leave them in.
//     So the wave that owns a tile computes them itself, in the exact two-pass form, in two passes over its 16 rows before the
//     products (the rows — 128 KB per tile at 2048 columns — come back from L2 for the second and third pass); the update path
//     gets them from the same kernel through the workspace (mean0 / rstd0), as from wide_l1_fwd16_kernel;
//   * the folded bias b1' = b1 + W1 beta0 is summed by the staging threads over every chunk of the first tile;
//   * the row end is handled in the last chunk only (ld4_row: a 16-byte load that stays inside the row, zeros beyond it);
//   * wide_l1_bwd_sliced_kernel is the general tile loop of wide_l1_bwd16_kernel with a column base: blockIdx.y is a 512-column
//     slice, wave w owns chunk w of it.  The epilogues are per column, so the slices are independent; each computes the bias sums
//     db it needs itself (64 adds per tile on its chunk-0 wave) and none writes them (the update kernel owns db1).
// Registers / occupancy: see DESIGN.md §3, "Inputs beyond 512 columns".
#pragma once
#include "mlp_wide16.h"

// Layer 1 for every 16-sample tile of this wave: calls tail(acc, i, ok, mean, rstd) with acc = z1 of sample i, bias included
// (accumulator layout: lane (n, q) holds features 16 b + 4 q + r).  512 threads; sW: [2][64 * RS16] chunk buffers, sB: [64]
// folded bias.  pre() runs once, before the first barrier (the caller's own staging).  Row forms as in wide16_layer1: gather
// through p.rows, or strided (n, m) rows (p.x_M > 0).
template <class Pre, class Tail>
__device__ __forceinline__ void sliced_layer1(const Wide16Args &p, float (*sW)[HID * RS16], float *sB, const int bid, const int nb,
                                              Pre &&pre, Tail &&tail) {
  constexpr int NW = 8, TPR = 8, CW = 8, CV = 2;               // waves, threads per weight row, floats (vectors) per thread and chunk
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = p.D;
  const bool fnorm = p.fn_w >= 0;
  const bool al4 = (D & 3) == 0;
  const float inv_D = 1.0f / (float)D;
  const int64_t n_tiles = (p.B + 15) / 16;
  const int64_t n_groups = (n_tiles + NW - 1) / NW;            // NW tiles (one per wave) share the weight stream
  const int nch = (D + 63) / 64, c_last = nch - 1;

  const int wf = tid / TPR, wp = tid % TPR;                    // this thread's share of a weight chunk: row wf, columns CW wp ..
  float bacc = 0.f;                                            // its part of (W1 beta0)[wf]
  auto fetch_chunk = [&](int c, f32x4 (&w)[CV], bool with_bias) {
    const float *wrow = p.params + p.w1 + (size_t)wf * D, *g = p.params + p.fn_w, *bt = p.params + p.fn_b;
    const int k0 = 64 * c + CW * wp;
    f32x4 gm[CV], be[CV];
    if (c < c_last) {
#pragma unroll
      for (int j4 = 0; j4 < CV; ++j4) w[j4] = ld4u(wrow + k0 + 4 * j4);
      if (fnorm) {
#pragma unroll
        for (int j4 = 0; j4 < CV; ++j4) { gm[j4] = ld4u(g + k0 + 4 * j4); be[j4] = ld4u(bt + k0 + 4 * j4); }
      }
    } else {
#pragma unroll
      for (int j4 = 0; j4 < CV; ++j4) w[j4] = ld4_row(wrow, k0 + 4 * j4, D, al4);
      if (fnorm) {
#pragma unroll
        for (int j4 = 0; j4 < CV; ++j4) { gm[j4] = ld4_row(g, k0 + 4 * j4, D, al4); be[j4] = ld4_row(bt, k0 + 4 * j4, D, al4); }
      }
    }
    if (fnorm) {
      if (with_bias) {
#pragma unroll
        for (int j4 = 0; j4 < CV; ++j4) { const f32x4 t = w[j4] * be[j4]; bacc += (t[0] + t[1]) + (t[2] + t[3]); }
      }
#pragma unroll
      for (int j4 = 0; j4 < CV; ++j4) w[j4] *= gm[j4];
    }
  };
  auto store_chunk = [&](int buf, const f32x4 (&w)[CV]) {
    float *dst = &sW[buf][wf * RS16 + CW * wp];
#pragma unroll
    for (int j4 = 0; j4 < CV; ++j4) st4(dst + 4 * j4, w[j4]);
  };
  auto row_ptr = [&](int64_t grp) {
    const int64_t i = (grp * NW + wave) * 16 + n;
    const int64_t row = i < p.B ? (p.rows ? (int64_t)p.rows[i] : i) : 0;
    return p.x + (p.x_M ? (row / p.x_M) * p.x_sn + (row % p.x_M) * p.x_sm : row * D);
  };
  // columns 64 c + 16 j4 + 4 q + t of this lane's sample: v[j4][t] (zeros beyond the row)
  auto load_x = [&](const float *xr, int c, f32x4 (&v)[4]) {
    if (c < c_last) {
      const float *xc = xr + 64 * c + 4 * q;
#pragma unroll
      for (int j4 = 0; j4 < 4; ++j4) v[j4] = ld4u(xc + 16 * j4);
    } else {
#pragma unroll
      for (int j4 = 0; j4 < 4; ++j4) v[j4] = ld4_row(xr, 64 * c + 16 * j4 + 4 * q, D, al4);
    }
  };
  // x - mean, zeros beyond the row
  auto centre = [&](f32x4 (&v)[4], int c, const f32x4 mean4) {
#pragma unroll
    for (int j4 = 0; j4 < 4; ++j4) {
      f32x4 d = v[j4] - mean4;
      if (c == c_last) {
#pragma unroll
        for (int t = 0; t < 4; ++t) d[t] = (64 * c + 16 * j4 + 4 * q + t < D) ? d[t] : 0.f;
      }
      v[j4] = d;
    }
  };

  pre();
  bool first = true;
  for (int64_t grp = bid; grp < n_groups; grp += nb) {         // (uniform over the workgroup: every wave meets every barrier)
    const int64_t i = (grp * NW + wave) * 16 + n;
    const bool ok = i < p.B;
    const float *xr = row_ptr(grp);
    f32x4 wN[CV];
    fetch_chunk(0, wN, first);
    // ---- LayerNorm statistics over the D inputs: exact two-pass form, two passes over the tile's rows ----
    float mean = 0.f, rstd = 1.f;
    if (fnorm) {
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int c = 0; c < nch; ++c) {
        f32x4 v[4];
        load_x(xr, c, v);
        s4 += (v[0] + v[1]) + (v[2] + v[3]);
      }
      mean = quad_sum16((s4[0] + s4[1]) + (s4[2] + s4[3])) * inv_D;
      const f32x4 mean4 = {mean, mean, mean, mean};
      f32x4 v4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int c = 0; c < nch; ++c) {
        f32x4 v[4];
        load_x(xr, c, v);
        centre(v, c, mean4);
        v4 += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
      }
      rstd = 1.0f / sqrtf(quad_sum16((v4[0] + v4[1]) + (v4[2] + v4[3])) * inv_D + LN_EPS);
    }
    const f32x4 mean4 = {mean, mean, mean, mean};
    // ---- z1 = b1' + rstd W1' (x - mean), chunk by chunk ----
    f32x4 xc[4], xn[4];
    load_x(xr, 0, xc);
    store_chunk(0, wN);                                        // (buffer 0 is free: the barrier after the previous tile's last chunk)
    f32x4 acc[4];
#pragma unroll
    for (int bo = 0; bo < 4; ++bo) acc[bo] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
      const bool more = c < c_last;
      if (more) { fetch_chunk(c + 1, wN, first); load_x(xr, c + 1, xn); }
      centre(xc, c, mean4);
      const float *Wc = &sW[c & 1][n * RS16 + 4 * q];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        f32x4 a[4];
#pragma unroll
        for (int bo = 0; bo < 4; ++bo) a[bo] = ld4(Wc + 16 * bo * RS16 + 16 * jj);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int bo = 0; bo < 4; ++bo) acc[bo] = mfma16(a[bo][t], xc[jj][t], acc[bo]);
      }
      if (more) {
        store_chunk((c + 1) & 1, wN);                          // (that buffer's readers passed the barrier of chunk c - 1)
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) xc[j4] = xn[j4];
      }
      __syncthreads();
    }
    if (first) {                                               // every chunk has been fetched: the folded bias of row wf
      float t = bacc;
#pragma unroll
      for (int off = 1; off < TPR; off <<= 1) t += __shfl_xor(t, off, WAVE);
      if (wp == 0) sB[wf] = p.params[p.b1 + wf] + (p.fn_b >= 0 ? t : 0.f);
      __syncthreads();
      first = false;
    }
    const f32x4 rstd4 = {rstd, rstd, rstd, rstd};
#pragma unroll
    for (int bo = 0; bo < 4; ++bo) acc[bo] = acc[bo] * rstd4 + ld4(sB + 16 * bo + 4 * q);
    tail(acc, i, ok, mean, rstd);
  }
}

// (A) of the update path: z1 [B][64] and the row statistics into the wide workspace (the outputs of wide_l1_fwd16_kernel)
template <int UNIT = 0>             // (a template so that every translation unit that includes this header may hold a copy)
__global__ __launch_bounds__(512, 2) void wide_l1_fwd_sliced_kernel(Wide16Args p) {
  __shared__ __align__(16) float sW[2][HID * RS16];
  __shared__ __align__(16) float sB[HID];
  const int q = (threadIdx.x & 63) >> 4;
  sliced_layer1(p, sW, sB, blockIdx.x, gridDim.x, []() {},
    [&](f32x4 (&acc)[4], int64_t i, bool ok, float mean, float rstd) __attribute__((always_inline)) {
      if (ok) {
        if (q == 0 && p.mean0) { p.mean0[i] = mean; p.rstd0[i] = rstd; }
#pragma unroll
        for (int b = 0; b < 4; ++b) st4(p.z1 + i * HID + 16 * b + 4 * q, acc[b]);
      }
    });
}

// The whole forward in one launch (mappo_mlp_forward / mappo_actor_act / mappo_mlp_features / the rollout step's networks): layer 1
// as above, then the register-resident tail of the narrow kernels (mlp_fwd16.h) on the same tile.  Dynamic LDS: the tail's map
// (lds_map_tail) followed by one [16][TP] logits tile per wave.
template <bool RELU, int LN, int MODE>
__global__ __launch_bounds__(512, 2) void wide_forward_sliced_kernel(Wide16Args w, FwdArgs p) {
  extern __shared__ __align__(16) float lds[];
  __shared__ __align__(16) float sW[2][HID * RS16];
  __shared__ __align__(16) float sB[HID];
  const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float *tZ = lds + p.map.tiles + wave * p.map.wave_stride;
  sliced_layer1(w, sW, sB, blockIdx.x, gridDim.x,
    [&]() __attribute__((always_inline)) { stage_tail_1shot<LN>(lds, p.map, p.params, p.off, p.desc); },
    [&](f32x4 (&acc)[4], int64_t i, bool ok, float, float) __attribute__((always_inline)) {
      forward16_tail<RELU, LN, MODE>(p, lds, p.map, acc, i, ok, j, q, tZ);
    });
}

// (B): weight gradient of layer 1 and the feature-norm gradients from the blocked dz1 and the row statistics in the wide
// workspace (layout, operand maps and the raw-product epilogue: wide_l1_bwd16_kernel).  Grid (slab rows, 512-column slices):
// workgroup (x, y) walks the tiles x, x + gridDim.x, ..; its wave w owns columns [512 y + 64 w, + 64) and writes them into slab
// row x.  Waves whose chunk starts beyond the row idle.
template <bool FNORM, bool GATHER>
__global__ __launch_bounds__(512, 2) void wide_l1_bwd_sliced_kernel(WideBwd16Args p) {
  __shared__ __align__(16) float sDb[HID];
  const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c0 = 512 * (int)blockIdx.y + 64 * wave;
  const bool active = c0 < p.D;                                // (wave 0 always is: gridDim.y = ceil(D / 512))
  const bool edge = c0 + 64 > p.D;                             // this wave's chunk holds the row end: clamped loads, masked columns
  const bool al4 = (p.D & 3) == 0;
  const int kcol = c0 + 4 * n, kcl = min(kcol, p.D - 4);       // this lane's 4 columns; where its 16-byte load starts
  const int64_t Bp = wide16_bp(p.B);
  const float *dz = p.wide_ws, *st_mean = p.wide_ws + 64 * Bp, *st_rstd = p.wide_ws + 65 * Bp;
  f32x4 G[4][4];
  float db[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int bf = 0; bf < 4; ++bf)
#pragma unroll
    for (int bk = 0; bk < 4; ++bk) G[bf][bk] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t n_full = p.B >> 4;                             // full tiles; tile n_full is the partial one (if any)
  const int64_t n_tiles = (p.B + 15) >> 4;
  const int64_t stride = gridDim.x;

  auto fetch_rows = [&](int (&ridx)[4], int64_t tile) __attribute__((always_inline)) {
    const int64_t s0 = tile * 16 + 4 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j) ridx[j] = p.rows[min(s0 + j, p.B - 1)];      // (the partial tile stays inside rows[])
  };
  auto fetch = [&](WideBwdOps &o, int64_t tile, const int (&ridx)[4]) __attribute__((always_inline)) {
    const float *dzt = dz + tile * 1024 + n * 16 + 4 * q;      // (padded to whole tiles: always in bounds)
#pragma unroll
    for (int bf = 0; bf < 4; ++bf) o.a[bf] = ld4(dzt + 256 * bf);
    o.mean = ld4(st_mean + tile * 16 + 4 * q);
    o.rstd = ld4(st_rstd + tile * 16 + 4 * q);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t row = GATHER ? (int64_t)ridx[j] : min(tile * 16 + 4 * q + j, p.B - 1);
      o.b[j] = ld4u(p.x + row * p.D + kcl);
    }
  };
  auto compute = [&](WideBwdOps &o, int64_t tile) __attribute__((always_inline)) {
    if (tile == n_full) {                                      // partial tile: samples beyond the batch contribute nothing
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool v = tile * 16 + 4 * q + j < p.B;
#pragma unroll
        for (int bf = 0; bf < 4; ++bf) o.a[bf][j] = v ? o.a[bf][j] : 0.f;
        o.mean[j] = v ? o.mean[j] : 0.f; o.rstd[j] = v ? o.rstd[j] : 0.f;
      }
    }
    if (edge) {                                                // zeros beyond the row
#pragma unroll
      for (int j = 0; j < 4; ++j) o.b[j] = ld4_row_fix(o.b[j], kcol, p.D, al4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 xh = o.b[j];
      if (FNORM) {
        const f32x4 m4 = {o.mean[j], o.mean[j], o.mean[j], o.mean[j]}, r4 = {o.rstd[j], o.rstd[j], o.rstd[j], o.rstd[j]};
        xh = (xh - m4) * r4;
        if (edge) {
#pragma unroll
          for (int bk = 0; bk < 4; ++bk) xh[bk] = (kcol + bk < p.D) ? xh[bk] : 0.f;
        }
      }
#pragma unroll
      for (int bf = 0; bf < 4; ++bf)
#pragma unroll
        for (int bk = 0; bk < 4; ++bk) G[bf][bk] = mfma16(o.a[bf][j], xh[bk], G[bf][bk]);
    }
    if (wave == 0) {
#pragma unroll
      for (int bf = 0; bf < 4; ++bf) db[bf] += (o.a[bf][0] + o.a[bf][1]) + (o.a[bf][2] + o.a[bf][3]);
    }
  };
  if (active) {
    // three operand sets: the loads of a tile are issued two tiles before its products; with a row gather the indices are fetched
    // one tile further ahead still
    int64_t tile = blockIdx.x;
    WideBwdOps o0, o1, o2;
    int r0[4] = {0, 0, 0, 0}, r1[4] = {0, 0, 0, 0}, r2[4] = {0, 0, 0, 0};
    if (GATHER) {
      if (tile < n_tiles) fetch_rows(r0, tile);
      if (tile + stride < n_tiles) fetch_rows(r1, tile + stride);
      if (tile + 2 * stride < n_tiles) fetch_rows(r2, tile + 2 * stride);
    }
    if (tile < n_tiles) fetch(o0, tile, r0);
    if (tile + stride < n_tiles) fetch(o1, tile + stride, r1);
    while (tile < n_tiles) {
      if (tile + 2 * stride < n_tiles) fetch(o2, tile + 2 * stride, r2);
      if (GATHER && tile + 3 * stride < n_tiles) fetch_rows(r0, tile + 3 * stride);
      compute(o0, tile);
      tile += stride;
      if (tile >= n_tiles) break;
      if (tile + 2 * stride < n_tiles) fetch(o0, tile + 2 * stride, r0);
      if (GATHER && tile + 3 * stride < n_tiles) fetch_rows(r1, tile + 3 * stride);
      compute(o1, tile);
      tile += stride;
      if (tile >= n_tiles) break;
      if (tile + 2 * stride < n_tiles) fetch(o1, tile + 2 * stride, r1);
      if (GATHER && tile + 3 * stride < n_tiles) fetch_rows(r2, tile + 3 * stride);
      compute(o2, tile);
      tile += stride;
    }
  }
  // ---- bias sums of this workgroup's tiles: lane (m, q) of wave 0 holds the sum over its samples of dz1[16 bf + m] ----
  if (wave == 0) {
#pragma unroll
    for (int bf = 0; bf < 4; ++bf) {
      const float d = quad_sum16(db[bf]);
      if (q == 0) sDb[16 * bf + n] = d;
    }
  }
  __syncthreads();
  if (!active) return;
  // ---- raw products -> gradients, per wave ----
  float *slab = p.slabs + (size_t)blockIdx.x * p.slab_stride + p.slab_col0;
  float dgam[4] = {0.f, 0.f, 0.f, 0.f}, dbet[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int bk = 0; bk < 4; ++bk) {
    const int k = c0 + 4 * n + bk;
    const bool kv = k < p.D;
    const int kc = kv ? k : p.D - 1;
    const float gam = FNORM ? p.params[p.fn_w + kc] : 1.f, bet = FNORM ? p.params[p.fn_b + kc] : 0.f;
#pragma unroll
    for (int bf = 0; bf < 4; ++bf) {
      const f32x4 dbq = ld4(&sDb[16 * bf + 4 * q]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int f = 16 * bf + 4 * q + i;
        const float g = G[bf][bk][i];
        if (FNORM) {
          const float w = p.params[p.w1 + f * p.D + kc];
          dgam[bk] += w * g; dbet[bk] += w * dbq[i];
        }
        if (kv) slab[p.w1 + f * p.D + k] = gam * g + bet * dbq[i];
      }
    }
    if (FNORM) {
      const float dg = quad_sum16(dgam[bk]), dt = quad_sum16(dbet[bk]);
      if (q == 0 && kv) { slab[p.fn_w + k] = dg; slab[p.fn_b + k] = dt; }
    }
  }
}
