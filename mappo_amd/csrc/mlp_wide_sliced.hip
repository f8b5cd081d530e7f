// inputs beyond 512 columns (mlp_wide_sliced.h): layer-1 forward into the wide workspace, layer-1 weight gradient, and the host
// side the entry points share (the one-launch forwards are compiled in mlp_wide_sliced_r{0,1}.hip)
#include "mlp_host.h"
#include "mlp_wide_sliced.h"

int wide_sliced_launch_l1_fwd(const Wide16Args &w, dim3 grid, hipStream_t st) {
  return launch_kernel<wide_l1_fwd_sliced_kernel<0>, WIDE_LDS_STREAM, MAPPO_PROF_WIDE_L1>("wide_l1_fwd", grid, dim3(512), 0, st, w);
}

template <bool FN>
static void wide_sliced_l1_bwd_one(const WideBwd16Args &w, dim3 grid, hipStream_t st) {
  if (w.rows) PROF_LAUNCH(MAPPO_PROF_WIDE_L1, (wide_l1_bwd_sliced_kernel<FN, true>), grid, dim3(512), 0, st, w);
  else PROF_LAUNCH(MAPPO_PROF_WIDE_L1, (wide_l1_bwd_sliced_kernel<FN, false>), grid, dim3(512), 0, st, w);
}
// grid: (slab rows, 512-column slices)
int wide_sliced_launch_l1_bwd(const WideBwd16Args &w, dim3 grid, hipStream_t st) {
  if (w.fn_w >= 0) wide_sliced_l1_bwd_one<true>(w, grid, st); else wide_sliced_l1_bwd_one<false>(w, grid, st);
  return MAPPO_OK;
}

// LDS map, layer-1 arguments and launch shape of the one-launch forward for the network in `a` (a.off set): the tail's map with
// one [16][TP] logits tile per wave behind it
int wide_sliced_forward_prepare(FwdArgs &a, Wide16Args &w, size_t &lb, dim3 &grid, const char *who) {
  a.map = lds_map_tail(a.desc);
  a.map.wave_stride = 16 * TP;
  a.map.total = a.map.tiles + 8 * a.map.wave_stride;
  lb = (size_t)a.map.total * sizeof(float);
  MAPPO_REQUIRE(lb <= WIDE_LDS_STREAM, "%s: needs %zu B of LDS", who, lb);
  w = Wide16Args{};
  w.params = a.params; w.x = a.x; w.rows = a.rows; w.B = a.B; w.D = a.desc.in_dim; w.w1 = a.off.w1; w.b1 = a.off.b1;
  w.fn_w = a.desc.use_feature_norm ? a.off.fn_w : -1; w.fn_b = a.desc.use_feature_norm ? a.off.fn_b : -1;
  w.x_M = a.x_M; w.x_sn = a.x_sn; w.x_sm = a.x_sm;
  const int64_t n_groups = ((a.B + 15) / 16 + 7) / 8;            // 8 tiles (one per wave) share the weight stream
  grid = dim3((unsigned)(n_groups < 2 * NUM_CU ? n_groups : 2 * NUM_CU));
  return MAPPO_OK;
}

// mode 0: out = head output, 1: sample / argmax + log-prob, 2: trunk features [64][B]
int wide_sliced_forward(int mode, const FwdArgs &a_in, hipStream_t st, const char *who) {
  FwdArgs a = a_in;
  a.off = net_offsets(a.desc);
  MAPPO_REQUIRE(!a.out_blocked, "%s: the blocked trunk output exists for in_dim <= %d only", who, WIDE_TUNED_MAX_D);
  Wide16Args w;
  size_t lb;
  dim3 grid;
  if (int rc = wide_sliced_forward_prepare(a, w, lb, grid, who)) return rc;
  const int rcl = a.desc.use_relu ? wide_sliced_launch_forward_r<true>(mode, a.desc.layer_N, grid, lb, st, w, a, who)
                                  : wide_sliced_launch_forward_r<false>(mode, a.desc.layer_N, grid, lb, st, w, a, who);
  if (rcl) return rcl;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}
