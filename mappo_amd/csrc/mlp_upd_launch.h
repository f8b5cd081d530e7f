// mlp_upd_launch.h — launchers of mlp_update_kernel<MLP_UPD_RELU, MLP_UPD_LN, HEAD 0..3> (mlp_upd.h); included by
// mlp_upd_r*_l*.hip, which define the two template parameters.
#pragma once
#include "mlp_upd.h"
#include "mlp_launch.h"

template <bool R, int L, int HEAD>
int upd_inst(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const UpdArgs &a, const char *who) {
  return launch_kernel<mlp_update_kernel<R, L, HEAD>, LDS_DYN_MAX, MAPPO_PROF_MLP_BWD>(who, grid, block, lds_bytes, st, a);
}
template int upd_inst<MLP_UPD_RELU, MLP_UPD_LN, 0>(dim3, dim3, size_t, hipStream_t, const UpdArgs &, const char *);
template int upd_inst<MLP_UPD_RELU, MLP_UPD_LN, 1>(dim3, dim3, size_t, hipStream_t, const UpdArgs &, const char *);
template int upd_inst<MLP_UPD_RELU, MLP_UPD_LN, 2>(dim3, dim3, size_t, hipStream_t, const UpdArgs &, const char *);
template int upd_inst<MLP_UPD_RELU, MLP_UPD_LN, 3>(dim3, dim3, size_t, hipStream_t, const UpdArgs &, const char *);
