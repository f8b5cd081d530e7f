// mlp_upd.h — mlp_update_kernel, the K-chunked update kernel for wide inputs (in_dim 65..2048: it walks any number of 64-column chunks) where the 16-sample-tile kernels
// do not apply: layer_N = 2 and the external-gradient head of mappo_mlp_backward.  One wave per 32-sample tile; the workgroup
// streams 64-column chunks of W1 through LDS, each wave re-normalises its rows chunk by chunk; dz1 and the row statistics go to a
// feature-major HBM scratch from which wide_l1_bwd_kernel (mlp.hip) computes the W1 / feature-norm gradients.  The forward is
// recomputed per tile, the dW accumulators stay in registers across the persistent tile loop, and every workgroup writes ONE
// partial-gradient slab, summed by mappo_slab_reduce (deterministic, no float atomics).
//   HEAD 0: head gradient supplied by the caller (mappo_mlp_backward)
//   HEAD 1: actor  — PPO clipped surrogate + entropy computed in the kernel from the logits
//   HEAD 2: critic — clipped Huber|MSE value loss computed in the kernel from the values
//   HEAD 3: gradient w.r.t. the trunk output supplied by the caller (mappo_trunk_backward)
// Needs mlp_upd_args.h, mlp_stamps.h.
#pragma once
#include "mlp_upd_args.h"
#include "mlp_stamps.h"

#define UPD_THREADS 256
template <bool RELU, int LN, int HEAD>
__global__ __launch_bounds__(UPD_THREADS, 1) void mlp_update_kernel(UpdArgs p) {
  extern __shared__ __align__(16) float lds[];
  __shared__ double red_smem[16 * 4];
  const int n_waves = blockDim.x / WAVE;
  const NetOff &o = p.off;
  const LdsMap &m = p.map;
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), l31 = lane & 31, half = lane >> 5;
  const int D = p.desc.in_dim, A = p.desc.out_dim;
  const int64_t n_tiles = (p.B + TS - 1) / TS;
  const int64_t n_btiles = (n_tiles + n_waves - 1) / n_waves;    // uniform tile loop (block barriers around the W1 chunks)
  STAMP_DECL
  stage_all_weights<LN>(lds, m, p.params, o, p.desc);
  __syncthreads();
  STAMP(0);   // staging
  float *tX = lds + m.tiles + wave * m.wave_stride;
  float *tH = tX + m.x_rows * TP;
  float *tZ = tH + (LN + 1) * HID * TP;

  // loss constants (HEAD 1/2): denominators are GLOBAL (mb_moments), see ppo_loss.hip
  LossScales ls = {0.f, 0.f, 0.f, 1.f};
  if (HEAD == 1 || HEAD == 2) ls = loss_scales(p.cfg, p.mb_moments, p.vn_state);
  double lacc[4] = {0.0, 0.0, 0.0, 0.0};   // actor: sum w*min(s1,s2), sum w*H, sum ratio | critic: sum w_v*l

  // ---- gradient accumulators (registers, live across the tile loop) ----
  f32x16 gWh[1][2], gW2[LN > 0 ? LN : 1][2][2];       // (W1 / feature-norm gradients: wide_l1_bwd_kernel)
  // raw products: gW*[f][k] = sum_s dz[f][s] * xhat_in[k][s] (LayerNorm affine of the input NOT applied), gB = sum_s dz.
  // The epilogue turns them into weight, LayerNorm-affine and feature-norm gradients.
  float gBh = 0.f;
  float gB[LN + 1];
  float gLnW = 0.f, gLnB = 0.f;          // HEAD 3 only: affine of the last LayerNorm (the gradient arrives behind it)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) gWh[0][i][r] = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int l = 0; l < LN; ++l) gW2[l][i][j][r] = 0.f;
  }
#pragma unroll
  for (int l = 0; l <= LN; ++l) gB[l] = 0.f;

  for (int64_t tb = blockIdx.x; tb < n_btiles; tb += gridDim.x) {
    const int64_t tile = tb * n_waves + wave;
    const int64_t base = tile * TS;
    LossPrefetch cur;
    TileStats<LN> st;
    float mean0 = 0.f, rstd0 = 1.f;
    const int n_valid = (int)max((int64_t)0, min((int64_t)TS, p.B - base));
    const bool ok = l31 < n_valid;
    const int64_t row = ok ? (p.rows ? (int64_t)p.rows[base + l31] : base + l31) : 0;
    prefetch_loss<HEAD>(cur, p, row, n_valid, lane, A);
    const float *xr = p.x + row * D;
    wide_row_stats(xr, D, ok, half, p.desc.use_feature_norm != 0, mean0, rstd0);
    STAMP(1);
    tile_forward_wide<RELU, LN>(lds, m, p.params + o.w1, xr, ok, mean0, rstd0, tX, tH, D, l31, half, st);
    float *tLast = tH + LN * HID * TP;
    STAMP(2);   // trunk forward

    // ---- head gradient into tZ[s][a] ----
    if (HEAD == 3) {
      // nothing: the gradient arrives at the trunk output (loaded below)
    } else if (HEAD == 0) {
      for (int e = lane; e < TS * A; e += WAVE) {
        const int s = e / A, a = e - s * A;
        tZ[s * TP + a] = (s < n_valid) ? p.dout[base * A + e] : 0.f;
      }
    } else {
      const f32x16 z = head_forward(lds, m, tLast, lds + ln_w_of<LN>(m, LN), lds + ln_b_of<LN>(m, LN), l31, half);
      if (HEAD == 1) {
        head_to_tile(tZ, z, A, l31, half);
        wave_lds_sync();
        if (lane < TS) {
          float *zl = tZ + lane * TP;
          if (lane < n_valid) {
            actor_loss_lane(zl, A, cur.dead, (int)cur.f0, cur.f1, cur.f2, cur.f3, p.cfg, ls.scale_pi, lacc);
          } else {
            for (int a = 0; a < A; ++a) zl[a] = 0.f;
          }
        }
      } else {
        // value loss (r_mappo.py:62-87); the value of sample s is register 0 of lane s (half 0)
        if (lane < TS) {
          float dvv = 0.f;
          if (lane < n_valid) dvv = critic_loss_lane(z[0], cur.f0, cur.f1, cur.f2, p.cfg, ls, lacc);
          tZ[lane * TP] = dvv;
        }
      }
    }
    wave_lds_sync();
    STAMP(3);   // head forward + loss

    // ---- (A) raw head products:  gWh[a][f] += sum_s dz[s][a] * xhat_last[f][s] ----
    if (HEAD != 3) {
      float bsum = 0.f;
#pragma unroll 2
      for (int ss = 0; ss < TS / 2; ++ss) {
        const int s = 2 * ss + half;
        const float av = (l31 < A) ? tZ[s * TP + l31] : 0.f;
        bsum += av;
        gWh[0][0] = mfma(av, tLast[l31 * TP + s], gWh[0][0]);
        gWh[0][1] = mfma(av, tLast[(32 + l31) * TP + s], gWh[0][1]);
      }
      gBh += xhalf_sum(bsum);
    }
    // ---- (B) d h_last = Wh^T . dz ----
    f32x16 dH[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) dH[t][r] = 0.f;
    if (HEAD == 3) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (l31 < n_valid) dH[t][r] = p.dHT[(int64_t)(32 * t + ROWMAP(r, half)) * p.B + base + l31];
    } else {
      const float *sW = lds + m.wh;
      for (int kk = 0; kk < (A + 1) / 2; ++kk) {
        const int a = 2 * kk + half;
        const float b = (a < A) ? tZ[l31 * TP + a] : 0.f;
        dH[0] = mfma(sW[l31 * HP + a], b, dH[0]);
        dH[1] = mfma(sW[(32 + l31) * HP + a], b, dH[1]);
      }
    }
    STAMP(4);   // head grads (A), (B)
    // ---- hidden layers, last to first ----
#pragma unroll
    for (int l = LN; l >= 1; --l) {
      float *tCur = tH + l * HID * TP;          // xhat of this layer's LayerNorm -> scratch -> dz
      float *tPrev = tH + (l - 1) * HID * TP;   // xhat of the layer's input
      if (HEAD == 3 && l == LN)
        ln_act_backward<RELU, true>(dH, tCur, st.mean[l], st.rstd[l], st.pos[l], lds + m.ln2_w[l - 1], gLnW, gLnB, lane, l31, half);
      else
        ln_act_backward<RELU, false>(dH, tCur, st.mean[l], st.rstd[l], st.pos[l], lds + m.ln2_w[l - 1], gLnW, gLnB, lane, l31, half);
      gB[l] += tile_row_sum(tCur, lane);
      STAMP(5);   // LN + act backward (hidden)
      // gW2[f_out][k_in] += sum_s dz[f_out][s] * xhat_prev[k_in][s]
      {
#pragma unroll 2
        for (int ss = 0; ss < TS / 2; ++ss) {
          const int s = 2 * ss + half;
          const float a0 = tCur[l31 * TP + s], a1 = tCur[(32 + l31) * TP + s];
          const float b0 = tPrev[l31 * TP + s], b1 = tPrev[(32 + l31) * TP + s];
          gW2[l - 1][0][0] = mfma(a0, b0, gW2[l - 1][0][0]);
          gW2[l - 1][0][1] = mfma(a0, b1, gW2[l - 1][0][1]);
          gW2[l - 1][1][0] = mfma(a1, b0, gW2[l - 1][1][0]);
          gW2[l - 1][1][1] = mfma(a1, b1, gW2[l - 1][1][1]);
        }
      }
      STAMP(6);   // dW2
      // d h_prev = W2^T . dz
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dH[t][r] = 0.f;
      {
        const float *sW = lds + m.w2[l - 1];
#pragma unroll 2
        for (int kk = 0; kk < HID / 2; ++kk) {
          const int fo = 2 * kk + half;
          const float b = tCur[fo * TP + l31];
          dH[0] = mfma(sW[l31 * WP + fo], b, dH[0]);
          dH[1] = mfma(sW[(32 + l31) * WP + fo], b, dH[1]);
        }
      }
      wave_lds_sync();
      STAMP(7);   // dH (hidden)
    }
    // ---- layer 1 ----
    {
      float *tCur = tH;
      if (HEAD == 3 && LN == 0)
        ln_act_backward<RELU, true>(dH, tCur, st.mean[0], st.rstd[0], st.pos[0], lds + m.ln1_w, gLnW, gLnB, lane, l31, half);
      else
        ln_act_backward<RELU, false>(dH, tCur, st.mean[0], st.rstd[0], st.pos[0], lds + m.ln1_w, gLnW, gLnB, lane, l31, half);
      gB[0] += tile_row_sum(tCur, lane);
      STAMP(8);   // LN + act backward (layer 1)
      // dz1 (feature-major) and the row statistics go to HBM; wide_l1_bwd_kernel turns them into dW1 and the feature-norm
      // gradients (64 x in_dim accumulators do not fit one wave's registers)
      float *dz1T = p.wide_ws, *stats = p.wide_ws + (int64_t)HID * p.B;
      if (l31 < n_valid) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) dz1T[(int64_t)(32 * t + ROWMAP(r, half)) * p.B + base + l31] = dH[t][r];
        if (half == 0) { stats[base + l31] = mean0; stats[p.B + base + l31] = rstd0; }
      }
      wave_lds_sync();
    }
  }

  // ---- loss statistics of this workgroup ----
  if (HEAD == 1 || HEAD == 2) {
    block_sum<4>(lacc, red_smem);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double *q = p.partials + (size_t)blockIdx.x * 4 + k;
        *q = p.cfg.accumulate_partials ? *q + lacc[k] : lacc[k];
      }
    }
  }

  // ---- raw products -> gradient partials (per wave, registers; see raw_to_grad) ----
  float vLnW[LN + 1], vLnB[LN + 1];      // lane = k
  {
    float *scr = lds + m.scratch + wave * HID;
#pragma unroll
    for (int j = 0; j <= LN; ++j) { vLnW[j] = 0.f; vLnB[j] = 0.f; }
    if (HEAD != 3) {
      raw_to_grad<1>(gWh, (lane < TS && l31 < A) ? gBh : 0.f, scr, lds + m.wh, HP, lds + ln_w_of<LN>(m, LN), lds + ln_b_of<LN>(m, LN),
                     HID, true, lane, l31, half, vLnW[LN], vLnB[LN]);
    } else {
      vLnW[LN] = gLnW; vLnB[LN] = gLnB;
    }
#pragma unroll
    for (int l = LN - 1; l >= 0; --l)
      raw_to_grad<2>(gW2[l], gB[l + 1], scr, lds + m.w2[l], WP, lds + ln_w_of<LN>(m, l), lds + ln_b_of<LN>(m, l), HID, true, lane, l31,
                     half, vLnW[l], vLnB[l]);
  }
  STAMP(11);

  // ---- reduce the waves' accumulators through LDS (two regions, waves pair up) and write the slab ----
  __syncthreads();
  const int rb = p.red_base;                         // first flat parameter this launch reduces (b1)
  const int P = p.p_red - rb;
  float *red0 = lds + m.tiles - rb;                  // indexed by absolute flat offsets >= rb                     // n_regions * P floats fit in the tile area (checked on the host)
  const int n_reg = p.n_regions;
  for (int round = 0; round < (n_waves + n_reg - 1) / n_reg; ++round) {
    if (wave / n_reg == round) {
      float *red = red0 + (wave % n_reg) * P;
      const bool first = (round == 0);
      // one accumulator tile: 16 old values are read, then 16 sums written (reads never wait on the writes)
      auto red_tile = [&](const f32x16 &acc, int idx0, int ld, bool valid) {
        if (!valid) return;
        float *q = red + idx0;
        if (first) {                                     // first wave of a region: plain stores, nothing to read
#pragma unroll
          for (int r = 0; r < 16; ++r) q[((r & 3) + 8 * (r >> 2)) * ld] = acc[r];
        } else {
          float old[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) old[r] = q[((r & 3) + 8 * (r >> 2)) * ld];
#pragma unroll
          for (int r = 0; r < 16; ++r) q[((r & 3) + 8 * (r >> 2)) * ld] = old[r] + acc[r];
        }
      };
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
          const int col = 32 * tj + l31, row0 = 32 * ti + 4 * half;
#pragma unroll
          for (int l = 0; l < LN; ++l) red_tile(gW2[l][ti][tj], o.w2[l] + row0 * HID + col, HID, true);
        }
      // head: rows a = ROWMAP(r, half) < A only
      if (HEAD != 3)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        float old[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) { const int a = ROWMAP(r, half); old[r] = (!first && a < A) ? red[o.wh + a * HID + 32 * tj + l31] : 0.f; }
#pragma unroll
        for (int r = 0; r < 16; ++r) { const int a = ROWMAP(r, half); if (a < A) red[o.wh + a * HID + 32 * tj + l31] = old[r] + gWh[0][tj][r]; }
      }
      {
        constexpr int NVAL = 3 * (LN + 1) + 1;
        float vals[NVAL]; int idx[NVAL]; bool ok[NVAL];
        int n = 0;
        vals[n] = gB[0]; idx[n] = o.b1 + lane; ok[n++] = true;
        vals[n] = vLnW[0]; idx[n] = o.ln1_w + lane; ok[n++] = true;
        vals[n] = vLnB[0]; idx[n] = o.ln1_b + lane; ok[n++] = true;
#pragma unroll
        for (int l = 0; l < LN; ++l) {
          vals[n] = gB[l + 1]; idx[n] = o.b2[l] + lane; ok[n++] = true;
          vals[n] = vLnW[l + 1]; idx[n] = o.ln2_w[l] + lane; ok[n++] = true;
          vals[n] = vLnB[l + 1]; idx[n] = o.ln2_b[l] + lane; ok[n++] = true;
        }
        vals[n] = gBh; idx[n] = (HEAD != 3) ? o.bh + l31 : 0; ok[n++] = (HEAD != 3 && half == 0 && l31 < A);
        float old[NVAL];
#pragma unroll
        for (int i = 0; i < NVAL; ++i) old[i] = (!first && ok[i]) ? red[idx[i]] : 0.f;
#pragma unroll
        for (int i = 0; i < NVAL; ++i) if (ok[i]) red[idx[i]] = old[i] + vals[i];
      }
    }
    __syncthreads();
  }
  STAMP(12);    // block reduction through LDS
  float *slab = p.slabs + (size_t)blockIdx.x * p.slab_stride + p.slab_col0 + rb;
  const float *redv = red0 + rb;
  if (n_reg > 1) {
    for (int e = threadIdx.x; e < P; e += blockDim.x) slab[e] = redv[e] + redv[P + e];
  } else {
    for (int e = threadIdx.x; e < P; e += blockDim.x) slab[e] = redv[e];
  }
  STAMP(13);    // slab write
  STAMP_FLUSH();
}
