// mlp_upd16_launch.h — launchers of the 16-sample-tile update kernels (mlp_upd16.h): mlp_update16_kernel, mlp_update16_dual_kernel
// and mlp_update16x_kernel<MLP_UPD_RELU, MLP_UPD_LN, ...>; included by mlp_upd16_r*_l*.hip, which define the two template parameters
// (mlp_upd16md_r*_l*.hip with MLP_UPD_MD: the MultiDiscrete actor's kernels; mlp_upd16g_r*_l*.hip with MLP_UPD_GROUP: the grouped launch).
#pragma once
#include "mlp_upd16.h"
#include "mlp_launch.h"

static_assert(L16<0, 1, false>::LDS_CAP * 4 == UPD16_LDS_MAX, "L16::LDS_CAP is UPD16_LDS_MAX in floats");

#if defined(MLP_UPD_GROUP)
// several agents' dual launches in one (mlp_update16_group_kernel): translation units mlp_upd16g_r*_l*.hip
template <bool R, int L>
int upd16g_inst(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Group16Args &g) {
  return launch_kernel<mlp_update16_group_kernel<R, L>, UPD16_LDS_MAX, MAPPO_PROF_MLP_BWD>("actor_critic_update_group", grid, block, lds_bytes, st, g);
}
template int upd16g_inst<MLP_UPD_RELU, MLP_UPD_LN>(dim3, dim3, size_t, hipStream_t, const Group16Args &);
#elif defined(MLP_UPD_MD)
// the MultiDiscrete actor's kernels (mlp_update16_md_kernel, mlp_update16_md_dual_kernel): translation units mlp_upd16md_r*_l*.hip
template <bool R, int L, bool W>
static int upd16md_launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Upd16Args &a, const MdHeads &md) {
  return launch_kernel<mlp_update16_md_kernel<R, L, W>, UPD16_LDS_MAX, MAPPO_PROF_MLP_BWD>("actor_update_md", grid, block, lds_bytes, st, a, md);
}
template <bool R, int L>
int upd16md_inst(bool wide, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Upd16Args &a, const MdHeads &md) {
  return wide ? upd16md_launch<R, L, true>(grid, block, lds_bytes, st, a, md) : upd16md_launch<R, L, false>(grid, block, lds_bytes, st, a, md);
}
template int upd16md_inst<MLP_UPD_RELU, MLP_UPD_LN>(bool, dim3, dim3, size_t, hipStream_t, const Upd16Args &, const MdHeads &);

template <bool R, int L, bool WA, bool WC>
static int upd16mdd_launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Dual16Args &d, const MdHeads &md) {
  return launch_kernel<mlp_update16_md_dual_kernel<R, L, WA, WC>, UPD16_LDS_MAX, MAPPO_PROF_MLP_BWD>("actor_critic_update_md", grid, block, lds_bytes, st, d, md);
}
template <bool R, int L>
int upd16mdd_inst(bool wa, bool wc, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Dual16Args &d, const MdHeads &md) {
  if (wa) return wc ? upd16mdd_launch<R, L, true, true>(grid, block, lds_bytes, st, d, md) : upd16mdd_launch<R, L, true, false>(grid, block, lds_bytes, st, d, md);
  return wc ? upd16mdd_launch<R, L, false, true>(grid, block, lds_bytes, st, d, md) : upd16mdd_launch<R, L, false, false>(grid, block, lds_bytes, st, d, md);
}
template int upd16mdd_inst<MLP_UPD_RELU, MLP_UPD_LN>(bool, bool, dim3, dim3, size_t, hipStream_t, const Dual16Args &, const MdHeads &);
#else

template <bool R, int L, int HEAD, bool W>
static int upd16_launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Upd16Args &a) {
  return launch_kernel<mlp_update16_kernel<R, L, HEAD, W>, UPD16_LDS_MAX, MAPPO_PROF_MLP_BWD>("update16", grid, block, lds_bytes, st, a);
}
template <bool R, int L>
int upd16_inst(int head, bool wide, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Upd16Args &a) {
  if (head == 1) return wide ? upd16_launch<R, L, 1, true>(grid, block, lds_bytes, st, a) : upd16_launch<R, L, 1, false>(grid, block, lds_bytes, st, a);
  if (head == 3) return wide ? upd16_launch<R, L, 3, true>(grid, block, lds_bytes, st, a) : upd16_launch<R, L, 3, false>(grid, block, lds_bytes, st, a);
  return wide ? upd16_launch<R, L, 2, true>(grid, block, lds_bytes, st, a) : upd16_launch<R, L, 2, false>(grid, block, lds_bytes, st, a);
}
template int upd16_inst<MLP_UPD_RELU, MLP_UPD_LN>(int, bool, dim3, dim3, size_t, hipStream_t, const Upd16Args &);

template <bool R, int L, bool WA, bool WC>
static int upd16d_launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Dual16Args &d) {
  return launch_kernel<mlp_update16_dual_kernel<R, L, WA, WC>, UPD16_LDS_MAX, MAPPO_PROF_MLP_BWD>("actor_critic_update", grid, block, lds_bytes, st, d);
}
template <bool R, int L>
int upd16d_inst(bool wa, bool wc, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Dual16Args &d) {
  if (wa) return wc ? upd16d_launch<R, L, true, true>(grid, block, lds_bytes, st, d) : upd16d_launch<R, L, true, false>(grid, block, lds_bytes, st, d);
  return wc ? upd16d_launch<R, L, false, true>(grid, block, lds_bytes, st, d) : upd16d_launch<R, L, false, false>(grid, block, lds_bytes, st, d);
}
template int upd16d_inst<MLP_UPD_RELU, MLP_UPD_LN>(bool, bool, dim3, dim3, size_t, hipStream_t, const Dual16Args &);

template <bool R, int L, int HEAD>
static int upd16x_launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Upd16Args &a) {
  return launch_kernel<mlp_update16x_kernel<R, L, HEAD>, UPD16_LDS_MAX, MAPPO_PROF_MLP_BWD>("update16x", grid, block, lds_bytes, st, a);
}
template <bool R, int L>
int upd16x_inst(int head, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Upd16Args &a) {
  if (head == 3) return upd16x_launch<R, L, 3>(grid, block, lds_bytes, st, a);
  return head == 1 ? upd16x_launch<R, L, 1>(grid, block, lds_bytes, st, a) : upd16x_launch<R, L, 2>(grid, block, lds_bytes, st, a);
}
template int upd16x_inst<MLP_UPD_RELU, MLP_UPD_LN>(int, dim3, dim3, size_t, hipStream_t, const Upd16Args &);
#endif  // MLP_UPD_MD
