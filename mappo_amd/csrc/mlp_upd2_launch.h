// mlp_upd2_launch.h — launchers of mlp_update2_kernel<MLP_UPD_RELU, MLP_UPD_LN, HEAD 0..3, WIDE 0..1> (mlp_upd2.h); included by
// mlp_upd2_r*_l*.hip, which define the two template parameters.
#pragma once
#include "mlp_upd2.h"
#include "mlp_launch.h"

template <bool R, int L, int HEAD>
int upd2_inst(bool wide, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const UpdArgs &a, const char *who) {
  return wide ? launch_kernel<mlp_update2_kernel<R, L, HEAD, true>, LDS_DYN_MAX, MAPPO_PROF_MLP_BWD>(who, grid, block, lds_bytes, st, a)
              : launch_kernel<mlp_update2_kernel<R, L, HEAD, false>, LDS_DYN_MAX, MAPPO_PROF_MLP_BWD>(who, grid, block, lds_bytes, st, a);
}
template int upd2_inst<MLP_UPD_RELU, MLP_UPD_LN, 0>(bool, dim3, dim3, size_t, hipStream_t, const UpdArgs &, const char *);
template int upd2_inst<MLP_UPD_RELU, MLP_UPD_LN, 1>(bool, dim3, dim3, size_t, hipStream_t, const UpdArgs &, const char *);
template int upd2_inst<MLP_UPD_RELU, MLP_UPD_LN, 2>(bool, dim3, dim3, size_t, hipStream_t, const UpdArgs &, const char *);
template int upd2_inst<MLP_UPD_RELU, MLP_UPD_LN, 3>(bool, dim3, dim3, size_t, hipStream_t, const UpdArgs &, const char *);
