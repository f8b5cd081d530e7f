// mlp_upd2d_launch.h — launchers of mlp_update2_dual_kernel<MLP_UPD_RELU, MLP_UPD_LN, WIDE_A 0..1, WIDE_C 0..1> (mlp_upd2.h);
// included by mlp_upd2d_r*_l*.hip, which define the two template parameters.
#pragma once
#include "mlp_upd2.h"
#include "mlp_launch.h"

template <bool R, int L, bool WA, bool WC>
static int upd2d_launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const DualArgs &d) {
  return launch_kernel<mlp_update2_dual_kernel<R, L, WA, WC>, LDS_DYN_MAX, MAPPO_PROF_MLP_BWD>("actor_critic_update", grid, block, lds_bytes, st, d);
}
template <bool R, int L>
int upd2d_inst(bool wa, bool wc, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const DualArgs &d) {
  if (wa) return wc ? upd2d_launch<R, L, true, true>(grid, block, lds_bytes, st, d) : upd2d_launch<R, L, true, false>(grid, block, lds_bytes, st, d);
  return wc ? upd2d_launch<R, L, false, true>(grid, block, lds_bytes, st, d) : upd2d_launch<R, L, false, false>(grid, block, lds_bytes, st, d);
}
template int upd2d_inst<MLP_UPD_RELU, MLP_UPD_LN>(bool, bool, dim3, dim3, size_t, hipStream_t, const DualArgs &);
