// stats_core.h — the arithmetic of the statistics kernels (stats.hip, update_stats in mlp.hip) as device functions, shared with
// the fused once-per-train() launches of train_glue.hip: a kernel and its fused form run the same operations in the same order,
// so their results are bit-identical.
#pragma once
#include "common.h"

#define STAT_BLOCK 256
#define STAT_MAX_BLOCKS 1024

static inline int stat_blocks(int64_t n) {
  int64_t b = (n + STAT_BLOCK * 4 - 1) / (STAT_BLOCK * 4);
  if (b < 1) b = 1;
  if (b > STAT_MAX_BLOCKS) b = STAT_MAX_BLOCKS;
  return (int)b;
}

// v[0..NV) = sum of the per-block partials [nblk][NV]; valid in thread 0
template <int NV>
__device__ __forceinline__ void final_reduce_sum(const double *partials, int nblk, double (&v)[NV], double *smem /*[16*NV]*/) {
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
  for (int b = threadIdx.x; b < nblk; b += blockDim.x) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += partials[(size_t)b * NV + i];
  }
  block_sum<NV>(v, smem);
}

// one sample of the advantage build: adv = returns - denormalised value; {sum a, sum a^2, count} over active rows
__device__ __forceinline__ void adv_moments_term(float ret, float value_pred, float active, const VnStats &vn, float *adv_i,
                                                 double (&v)[3]) {
  const float a = ret - (value_pred * vn.sd + vn.mean);   // r_mappo.py:174-177
  *adv_i = a;
  if (active != 0.f) {                                     // :178-181 (nanmean / nanstd)
    v[0] += (double)a;
    v[1] += (double)a * (double)a;
    v[2] += 1.0;
  }
}

// one sample of the minibatch moments: {sum ret, sum ret^2, sum active}
__device__ __forceinline__ void minibatch_moments_term(float r, float active, double (&v)[3]) {
  v[0] += (double)r;
  v[1] += (double)r * (double)r;
  v[2] += (double)active;
}

// valuenorm.py:37-54, one EMA step: running <- running*w + batch*(1-w).  The batch term is rounded to fp32 once and the
// running term enters through one fused multiply-add, spelled out so that the compiler has no choice of which product to
// fuse: valuenorm_update_kernel, valuenorm_update_n_kernel and the fused prologue all take this step and agree bit for bit.
// (Left to contraction -- __fmul_rn / __fadd_rn do not stop it -- the single update fused the batch product, the loop, its
// invariant product hoisted, the running one, and the two differed in the last bit.)
struct VnBatchTerms { float b0, b1; };   // batch mean * (1-w), batch mean of squares * (1-w)

__device__ __forceinline__ VnBatchTerms valuenorm_batch_terms(double m0, double m1, double m3, float omw) {
#pragma clang fp contract(off)
  const double B = m3 > 0.0 ? m3 : 1.0;
  VnBatchTerms t;
  t.b0 = (float)(m0 / B) * omw;
  t.b1 = (float)(m1 / B) * omw;
  return t;
}

__device__ __forceinline__ void valuenorm_ema_step(float &s0, float &s1, float &s2, const VnBatchTerms &t, float w, float omw) {
  s0 = __fmaf_rn(s0, w, t.b0);
  s1 = __fmaf_rn(s1, w, t.b1);
  s2 = __fmaf_rn(s2, w, omw);
}

// n such steps with the same batch moments {m0 = sum ret, m1 = sum ret^2, m3 = B}.  One thread.
__device__ __forceinline__ void valuenorm_update_n_body(float *vn_state, double m0, double m1, double m3, float w, float omw, int n,
                                                        float *states_out) {
  const VnBatchTerms t = valuenorm_batch_terms(m0, m1, m3, omw);
  float s0 = vn_state[0], s1 = vn_state[1], s2 = vn_state[2];
  for (int e = 0; e < n; ++e) {
    valuenorm_ema_step(s0, s1, s2, t, w, omw);
    states_out[3 * e + 0] = s0; states_out[3 * e + 1] = s1; states_out[3 * e + 2] = s2;
  }
  vn_state[0] = s0; vn_state[1] = s1; vn_state[2] = s2;
}

// statistics of one fused update from the two kernels' per-workgroup partial sums (same layout as
// mappo_ppo_loss_fwd_bwd's `stats`); one workgroup of blockDim.x threads
__device__ __forceinline__ void update_stats_body(const double *__restrict__ pa, const double *__restrict__ pc, int na, int nc,
                                                  const double *__restrict__ mb_moments, int use_policy_active,
                                                  int use_value_active, double *__restrict__ stats, double *__restrict__ acc,
                                                  double *smem /*[16*4]*/) {
  double v[4] = {0.0, 0.0, 0.0, 0.0};    // sum w*min, sum w*H, sum ratio, sum w_v*l
  for (int b = threadIdx.x; b < na; b += blockDim.x) { v[0] += pa[b * 4 + 0]; v[1] += pa[b * 4 + 1]; v[2] += pa[b * 4 + 2]; }
  for (int b = threadIdx.x; b < nc; b += blockDim.x) v[3] += pc[b * 4 + 0];
  block_sum<4>(v, smem);
  if (threadIdx.x == 0) {
    const double sa = mb_moments[2] > 0.0 ? mb_moments[2] : 1.0;
    const double Bg = mb_moments[3] > 0.0 ? mb_moments[3] : 1.0;
    const double den_pi = use_policy_active ? sa : Bg, den_v = use_value_active ? sa : Bg;
    stats[0] = v[3] / den_v;
    stats[1] = -v[0] / den_pi;
    stats[2] = v[1] / den_pi;
    stats[3] = v[2] / Bg;
    stats[4] = mb_moments[2];
    stats[5] = mb_moments[3];
    if (acc) { acc[0] += stats[0]; acc[1] += stats[1]; acc[2] += stats[2]; acc[3] += stats[3]; }   // train_info sums (r_mappo.py:207-212)
  }
}
