// mlp_wide_sliced_launch.h — launcher of the one-launch forward for in_dim 513..2048 (mlp_wide_sliced.h) for the activation
// MLP_WIDE_RELU; included by mlp_wide_sliced_r{0,1}.hip, which define that template parameter.
#pragma once
#include "mlp_fwd.h"
#include "mlp_upd16.h"
#include "mlp_wide_sliced.h"
#include "mlp_launch.h"

template <bool R, int L>
static int wide_sliced_forward_mode(int mode, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &w, const FwdArgs &a, const char *who) {
  const dim3 block(512);
  if (mode == 0) return launch_kernel<wide_forward_sliced_kernel<R, L, 0>, WIDE_LDS_STREAM, MAPPO_PROF_MLP_FWD>(who, grid, block, lds_bytes, st, w, a);
  if (mode == 1) return launch_kernel<wide_forward_sliced_kernel<R, L, 1>, WIDE_LDS_STREAM, MAPPO_PROF_ACT>(who, grid, block, lds_bytes, st, w, a);
  return launch_kernel<wide_forward_sliced_kernel<R, L, 2>, WIDE_LDS_STREAM, MAPPO_PROF_MLP_FWD>(who, grid, block, lds_bytes, st, w, a);
}
template <bool R>
int wide_sliced_launch_forward_r(int mode, int ln, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &w, const FwdArgs &a,
                                 const char *who) {
  if (ln == 0) return wide_sliced_forward_mode<R, 0>(mode, grid, lds_bytes, st, w, a, who);
  if (ln == 1) return wide_sliced_forward_mode<R, 1>(mode, grid, lds_bytes, st, w, a, who);
  return wide_sliced_forward_mode<R, 2>(mode, grid, lds_bytes, st, w, a, who);
}
template int wide_sliced_launch_forward_r<MLP_WIDE_RELU>(int, int, dim3, size_t, hipStream_t, const Wide16Args &, const FwdArgs &, const char *);
