// mlp_host.h — host helpers shared by the entry points in mlp.hip, mlp_step.hip and rollout_spread.hip: descriptor checks, the
// waves-per-workgroup fit and the launch shape of the one-launch wide forward.  Needs mlp_fwd.h, mlp_wide16_args.h, mlp_launch.h.
#pragma once
#include "mlp_fwd.h"
#include "mlp_upd16.h"           // RS16
#include "mlp_wide16_args.h"
#include "mlp_launch.h"

// LDS map, layer-1 arguments and launch shape of the one-launch wide forward (mlp_wide16.h) for the network in `a` (a.off / a.map set)
static int wide_forward_prepare(FwdArgs &a, Wide16Args &w, size_t &lb, dim3 &grid, dim3 &block, const char *who) {
  a.map.wave_stride = 16 * TP;                                   // the tail only needs the [16][TP] logits tile of a wave
  a.map.total = a.map.tiles + 8 * a.map.wave_stride;
  lb = (size_t)a.map.total * sizeof(float);
  MAPPO_REQUIRE(lb + sizeof(float) * (2 * HID * RS16 + HID) <= LDS_DYN_MAX, "%s: needs %zu B of LDS", who, lb);
  w = Wide16Args{};
  w.params = a.params; w.x = a.x; w.rows = a.rows; w.B = a.B; w.D = a.desc.in_dim; w.w1 = a.off.w1; w.b1 = a.off.b1;
  w.fn_w = a.desc.use_feature_norm ? a.off.fn_w : -1; w.fn_b = a.desc.use_feature_norm ? a.off.fn_b : -1;
  // 8 tiles (one per wave) share the weight stream; at most one workgroup per CU
  const int64_t n_tiles16 = (a.B + 15) / 16;
  const int64_t n_groups = (n_tiles16 + 7) / 8;
  grid = dim3((unsigned)(n_groups < NUM_CU ? n_groups : NUM_CU));
  block = dim3(512);
  return MAPPO_OK;
}

static int check_desc_common(const mappo_net_desc *d, const char *who) {
  MAPPO_REQUIRE(d, "%s: null desc", who);
  MAPPO_REQUIRE(d->hidden == HID, "%s: hidden_size %d unsupported (kernels are tiled for %d)", who, d->hidden, HID);
  MAPPO_REQUIRE(d->in_dim >= 1 && d->in_dim <= MAPPO_MAX_IN_DIM, "%s: in_dim %d outside [1,%d]", who, d->in_dim, MAPPO_MAX_IN_DIM);
  MAPPO_REQUIRE(d->out_dim >= 1 && d->out_dim <= MAPPO_MAX_ACTIONS, "%s: out_dim %d outside [1,%d]", who, d->out_dim,
                MAPPO_MAX_ACTIONS);
  MAPPO_REQUIRE(d->layer_N >= 0 && d->layer_N <= MAPPO_MAX_LAYER_N, "%s: layer_N %d outside [0,%d]", who, d->layer_N,
                MAPPO_MAX_LAYER_N);
  return MAPPO_OK;
}
static int check_desc(const mappo_net_desc *d, const char *who) {
  if (int rc = check_desc_common(d, who)) return rc;
  MAPPO_REQUIRE(!d->recurrent, "%s: recurrent networks go through mlp_features / gru_* / trunk_backward", who);
  return MAPPO_OK;
}
static int check_desc_trunk(const mappo_net_desc *d, const char *who) { return check_desc_common(d, who); }

// MultiDiscrete entry points (mappo_*_md): the limits of the multi-head kernels, checked on the host before anything is launched
static int check_md(const mappo_net_desc *d, const int32_t *head_dims, int32_t n_heads, const float *avail, const char *who, MdHeads &md) {
  MAPPO_REQUIRE(d, "%s: null desc", who);
  MAPPO_REQUIRE(head_dims, "%s: null head_dims", who);
  MAPPO_REQUIRE(n_heads >= 1 && n_heads <= 4, "%s: n_heads %d outside [1,4] (lane q of a sample's quad carries head q)", who, n_heads);
  int sum = 0;
  md = MdHeads{};
  md.n = n_heads;
  for (int j = 0; j < n_heads; ++j) {
    MAPPO_REQUIRE(head_dims[j] >= 1, "%s: head_dims[%d] = %d, every head needs at least 1 action", who, j, head_dims[j]);
    md.dim[j] = head_dims[j];
    sum += head_dims[j];
  }
  MAPPO_REQUIRE(sum == d->out_dim, "%s: sum of head_dims %d != out_dim %d", who, sum, d->out_dim);
  MAPPO_REQUIRE(d->out_dim <= 16, "%s: out_dim %d > 16 (the heads' logits share one 16-wide head tile)", who, d->out_dim);
  MAPPO_REQUIRE(d->in_dim <= MAXD, "%s: in_dim %d > %d", who, d->in_dim, MAXD);
  MAPPO_REQUIRE(d->layer_N <= 1, "%s: layer_N %d > 1", who, d->layer_N);
  MAPPO_REQUIRE(!d->recurrent, "%s: recurrent policies are not built for MultiDiscrete spaces", who);
  MAPPO_REQUIRE(!avail, "%s: MultiDiscrete spaces have no available_actions (avail must be NULL)", who);
  return check_desc(d, who);
}

static int fit_waves(const mappo_net_desc &d, int want) {
  int nw = want;
  while (nw > 1 && (size_t)lds_map(d, nw).total * sizeof(float) > LDS_DYN_MAX) nw >>= 1;
  return nw;
}
