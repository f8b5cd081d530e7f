// mlp_wide_fwd_launch.h — launchers of the streamed and resident one-launch wide forwards (mlp_wide16.h) for the activation
// MLP_WIDE_RELU; included by mlp_wide_fwd_r{0,1}.hip, which define that template parameter.  8-wave workgroups only — batches of
// up to 256 tiles take the split-K kernels (mlp_wide_sk.hip), and above that the 8-wave groups have enough tiles.
#pragma once
#include "mlp_fwd.h"
#include "mlp_upd16.h"
#include "mlp_wide16.h"
#include "mlp_launch.h"

template <bool R, int L, int MODE>
static int wide16_forward_nch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Wide16Args &w, const FwdArgs &a, const char *who) {
  constexpr int PID = (MODE == 1) ? MAPPO_PROF_ACT : MAPPO_PROF_MLP_FWD;
  return w.D <= 256 ? launch_kernel<wide_forward16_kernel<R, L, MODE, 8, 4>, WIDE_LDS_STREAM, PID>(who, grid, block, lds_bytes, st, w, a)       // row block registers for 4 chunks instead of 8
                    : launch_kernel<wide_forward16_kernel<R, L, MODE, 8, 8>, WIDE_LDS_STREAM, PID>(who, grid, block, lds_bytes, st, w, a);
}
template <bool R, int L>
static int wide16_forward_mode(int mode, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Wide16Args &w, const FwdArgs &a, const char *who) {
  if (mode == 0) return wide16_forward_nch<R, L, 0>(grid, block, lds_bytes, st, w, a, who);
  if (mode == 1) return wide16_forward_nch<R, L, 1>(grid, block, lds_bytes, st, w, a, who);
  return wide16_forward_nch<R, L, 2>(grid, block, lds_bytes, st, w, a, who);
}
template <bool R>
int wide16_launch_forward_r(int mode, int ln, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Wide16Args &w, const FwdArgs &a,
                            const char *who) {
  if (ln == 0) return wide16_forward_mode<R, 0>(mode, grid, block, lds_bytes, st, w, a, who);
  if (ln == 1) return wide16_forward_mode<R, 1>(mode, grid, block, lds_bytes, st, w, a, who);
  return wide16_forward_mode<R, 2>(mode, grid, block, lds_bytes, st, w, a, who);
}
template int wide16_launch_forward_r<MLP_WIDE_RELU>(int, int, dim3, dim3, size_t, hipStream_t, const Wide16Args &, const FwdArgs &, const char *);

template <bool R, int L>
static int wide16_features_dual_one(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const WideDualArgs &d) {
  return launch_kernel<wide_features16_dual_kernel<R, L, 8>, WIDE_LDS_STREAM, MAPPO_PROF_MLP_FWD>("mlp_features_dual", grid, block, lds_bytes, st, d);
}
template <bool R>
int wide16_launch_features_dual_r(int ln, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Wide16Args &wa, const FwdArgs &a,
                                  const Wide16Args &wc, const FwdArgs &c, int nA) {
  WideDualArgs d;
  d.wa = wa; d.wc = wc; d.a = a; d.c = c; d.nA = nA;
  if (ln == 0) return wide16_features_dual_one<R, 0>(grid, block, lds_bytes, st, d);
  if (ln == 1) return wide16_features_dual_one<R, 1>(grid, block, lds_bytes, st, d);
  return wide16_features_dual_one<R, 2>(grid, block, lds_bytes, st, d);
}
template int wide16_launch_features_dual_r<MLP_WIDE_RELU>(int, dim3, dim3, size_t, hipStream_t, const Wide16Args &, const FwdArgs &,
                                                          const Wide16Args &, const FwdArgs &, int);

template <bool R, int L, int NCH>
static int wide16_rollout_step_one(dim3 grid, size_t lds_bytes, hipStream_t st, const WideStepArgs &s) {
  return launch_kernel<wide_rollout_step_kernel<R, L, NCH>, WIDE_LDS_STREAM, MAPPO_PROF_ACT>("rollout_step", grid, dim3(512), lds_bytes, st, s);
}
template <bool R>
int wide16_launch_rollout_step_r(int ln, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &wa, const FwdArgs &a,
                                 const Wide16Args &wc, const FwdArgs &c, int nA) {
  WideStepArgs s;
  s.wa = wa; s.wc = wc; s.a = a; s.c = c; s.nA = nA;
  const bool big = wa.D > 256 || wc.D > 256;                      // row-block registers for 8 chunks instead of 4
  if (ln == 0) return big ? wide16_rollout_step_one<R, 0, 8>(grid, lds_bytes, st, s) : wide16_rollout_step_one<R, 0, 4>(grid, lds_bytes, st, s);
  if (ln == 1) return big ? wide16_rollout_step_one<R, 1, 8>(grid, lds_bytes, st, s) : wide16_rollout_step_one<R, 1, 4>(grid, lds_bytes, st, s);
  return big ? wide16_rollout_step_one<R, 2, 8>(grid, lds_bytes, st, s) : wide16_rollout_step_one<R, 2, 4>(grid, lds_bytes, st, s);
}
template int wide16_launch_rollout_step_r<MLP_WIDE_RELU>(int, dim3, size_t, hipStream_t, const Wide16Args &, const FwdArgs &, const Wide16Args &,
                                                         const FwdArgs &, int);

template <bool R, int L, int NCH>
static int wide16_features_resident_one(dim3 grid, hipStream_t st, const Wide16Args &w, const FwdArgs &a) {
  const size_t lds_bytes = sizeof(float) * ((size_t)HID * 64 * NCH + HID + a.map.tiles);
  MAPPO_REQUIRE(lds_bytes <= WIDE_LDS_WHOLE, "mlp_features: needs %zu B of LDS", lds_bytes);
  return launch_kernel<wide_features16_resident_kernel<R, L, NCH>, WIDE_LDS_WHOLE, MAPPO_PROF_MLP_FWD>("mlp_features", grid, dim3(512), lds_bytes, st, w, a);
}
template <bool R, int L>
static int wide16_features_resident_nch(dim3 grid, hipStream_t st, const Wide16Args &w, const FwdArgs &a) {
  switch ((w.D + 63) / 64) {
    case 2: return wide16_features_resident_one<R, L, 2>(grid, st, w, a);
    case 3: return wide16_features_resident_one<R, L, 3>(grid, st, w, a);
    case 4: return wide16_features_resident_one<R, L, 4>(grid, st, w, a);
    case 5: return wide16_features_resident_one<R, L, 5>(grid, st, w, a);
    case 6: return wide16_features_resident_one<R, L, 6>(grid, st, w, a);
    case 7: return wide16_features_resident_one<R, L, 7>(grid, st, w, a);
    default: return wide16_features_resident_one<R, L, 8>(grid, st, w, a);
  }
}
// layer_N <= 1 (the caller checks); grid: one workgroup per 8 tiles, at most one per CU
template <bool R>
int wide16_launch_features_resident_r(int ln, dim3 grid, hipStream_t st, const Wide16Args &w, const FwdArgs &a) {
  return ln == 0 ? wide16_features_resident_nch<R, 0>(grid, st, w, a) : wide16_features_resident_nch<R, 1>(grid, st, w, a);
}
template int wide16_launch_features_resident_r<MLP_WIDE_RELU>(int, dim3, hipStream_t, const Wide16Args &, const FwdArgs &);

template <bool R, int L, int NCH>
static int wide16_rollout_full_one(dim3 grid, size_t lds_bytes, hipStream_t st, const WideFullArgs &s) {
  return launch_kernel<wide_rollout_full_kernel<R, L, NCH>, WIDE_LDS_WHOLE, MAPPO_PROF_ACT>("rollout_step", grid, dim3(512), lds_bytes, st, s);
}
// in_dim of BOTH networks == 64 NCH, NCH 4 or 8 (the caller checks); ins: rewards / masks of the fused insert or NULL
template <bool R>
int wide16_launch_rollout_full_r(int ln, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &wa, const FwdArgs &a,
                                 const Wide16Args &wc, const FwdArgs &c, int nA, const InsertArgs *ins) {
  WideFullArgs s = {};
  s.wa = wa; s.wc = wc; s.a = a; s.c = c; s.nA = nA;
  if (ins) { s.ins = *ins; s.has_ins = 1; }
  const bool big = wa.D == 512;
  if (ln == 0) return big ? wide16_rollout_full_one<R, 0, 8>(grid, lds_bytes, st, s) : wide16_rollout_full_one<R, 0, 4>(grid, lds_bytes, st, s);
  if (ln == 1) return big ? wide16_rollout_full_one<R, 1, 8>(grid, lds_bytes, st, s) : wide16_rollout_full_one<R, 1, 4>(grid, lds_bytes, st, s);
  return big ? wide16_rollout_full_one<R, 2, 8>(grid, lds_bytes, st, s) : wide16_rollout_full_one<R, 2, 4>(grid, lds_bytes, st, s);
}
template int wide16_launch_rollout_full_r<MLP_WIDE_RELU>(int, dim3, size_t, hipStream_t, const Wide16Args &, const FwdArgs &, const Wide16Args &,
                                                         const FwdArgs &, int, const InsertArgs *);
