// mlp.hip — host entry points of the MLP forward, update and backward (the dispatch among the kernel families: launch_forward,
// launch_update, mappo_actor_critic_update; the family table is at the top of mlp_blocks.h) + the kernels that have no unit of
// their own: mlp_forward_kernel (mlp_fwd.h), wide_l1_bwd_kernel, update_stats_kernel.  The update kernels are instantiated in
// mlp_upd*_r*_l*.hip and the wide-input kernels in mlp_wide*.hip so that they compile in parallel; their launchers are declared
// in mlp_launch.h.
#include "mlp_host.h"
#include "mlp_upd.h"             // UPD_THREADS
#include "mlp_upd2.h"            // DualArgs
#include "mlp_upd16.h"           // Upd16Args, Dual16Args, L16
#include "stats_core.h"          // update_stats_body
#include <stdlib.h>

#ifdef MLP_STAMPS                // diagnostic build (scripts/stamps*.py): the buffers the update kernels flush their stamps to
static unsigned long long *g_stamp_host = nullptr;          // [gridDim.x][N_STAMPS]
static unsigned long long *g_stamp_waves_host = nullptr;    // [gridDim.x][8][N_STAMPS]
extern "C" int mappo_debug_set_stamps(unsigned long long *buf) { g_stamp_host = buf; return 0; }
extern "C" int mappo_debug_set_stamps_waves(unsigned long long *buf) { g_stamp_waves_host = buf; return 0; }
#endif

extern "C" int64_t mappo_net_param_count(const mappo_net_desc *desc) {
  if (!desc) return -1;
  return net_offsets(*desc).total;
}

template <int MODE>
static int launch_forward(const FwdArgs &a_in, hipStream_t st, const char *who) {
  MAPPO_CLEAR_STICKY();
  const int64_t n_tiles = (a_in.B + TS - 1) / TS;
  const int LN = a_in.desc.layer_N;
  // all waves of a workgroup stage the weights together, so 4 waves per workgroup even for rollout-sized batches
  const int nw = fit_waves(a_in.desc, n_tiles >= 4 ? 4 : (n_tiles >= 2 ? 2 : 1));
  FwdArgs a = a_in;
  a.off = net_offsets(a.desc);
  a.map = lds_map(a.desc, nw);
  const size_t lds_bytes = (size_t)a.map.total * sizeof(float);
  MAPPO_REQUIRE(lds_bytes <= LDS_DYN_MAX, "%s: needs %zu B of LDS", who, lds_bytes);
  int64_t nb = (n_tiles + nw - 1) / nw;
  if (nb > NUM_CU) nb = NUM_CU;
  dim3 grid((unsigned)nb), block(WAVE * nw);
  // beyond the tuned wide kernels: layer 1 in K slices + the register-resident tail, one launch (mlp_wide_sliced.h)
  if (a.desc.in_dim > WIDE_TUNED_MAX_D) return wide_sliced_forward(MODE, a, st, who);
  {
    if (a.desc.in_dim > MAXD && a.desc.in_dim <= 512 && a.x_M == 0) {
      // wide inputs: layer 1 from registers + double-buffered W1 chunks, the rest of the network on the same tile (mlp_wide16.h)
      Wide16Args w;
      size_t lb;
      dim3 g2, b2;
      if (int rcp = wide_forward_prepare(a, w, lb, g2, b2, who)) return rcp;
      const int64_t nt16 = (a.B + 15) / 16;
      int64_t sk_max = WIDE_SK_MAX_TILES;
      if (const char *e = getenv("MAPPO_WIDE_SK_TILES")) sk_max = atoll(e);      // diagnostic override
      if (nt16 <= sk_max && !getenv("MAPPO_WIDE_NO_SK")) {          // step-sized batch: one tile per 4-wave workgroup, split-K
        const int64_t gsk = nt16 < NUM_CU ? nt16 : NUM_CU;          // (512 registers per wave: one workgroup per CU; more tiles are walked)
        if (int rcw = wide16_launch_forward_sk(MODE, a.desc.use_relu != 0, LN, dim3((unsigned)gsk), lb, st, w, a, who)) return rcw;
        MAPPO_CHECK_LAUNCH(who);
        return MAPPO_OK;
      }
      // trunk features of a training-sized batch: W1' resident (wide_features16_resident_kernel); MAPPO_WIDE_RESIDENT=0: streamed (A/B)
      FwdArgs ar = a;
      ar.map = lds_map_tail(a.desc);
      const size_t lres = sizeof(float) * ((size_t)HID * 64 * ((a.desc.in_dim + 63) / 64) + HID + ar.map.tiles);
      if (MODE == 2 && LN <= 1 && nt16 >= 2 * 8 * NUM_CU && lres <= 159 * 1024 &&
          !(getenv("MAPPO_WIDE_RESIDENT") && atoi(getenv("MAPPO_WIDE_RESIDENT")) == 0)) {
        const int rcr = a.desc.use_relu ? wide16_launch_features_resident_r<true>(LN, g2, st, w, ar) : wide16_launch_features_resident_r<false>(LN, g2, st, w, ar);
        if (rcr) return rcr;
        MAPPO_CHECK_LAUNCH(who);
        return MAPPO_OK;
      }
      if (int rcw = wide16_launch_forward(MODE, a.desc.use_relu != 0, LN, g2, b2, lb, st, w, a, who)) return rcw;
      MAPPO_CHECK_LAUNCH(who);
      return MAPPO_OK;
    }
  }
  // XW: 0 = in_dim <= 32, 1 = in_dim <= 64 (rows prefetched into registers), 2 = in_dim > 64 (K-chunked layer 1)
  const int xw = a.desc.in_dim > MAXD ? 2 : (a.desc.in_dim > 32 ? 1 : 0);
  constexpr int prof_id = (MODE == 1) ? MAPPO_PROF_ACT : MAPPO_PROF_MLP_FWD;
  if (int rc = dispatch_relu_ln(a.desc.use_relu != 0, LN, [&](auto R, auto L) {
        if (xw == 2) return launch_kernel<mlp_forward_kernel<R.value, L.value, MODE, 2>, LDS_DYN_MAX, prof_id>(who, grid, block, lds_bytes, st, a);
        if (xw == 1) return launch_kernel<mlp_forward_kernel<R.value, L.value, MODE, 1>, LDS_DYN_MAX, prof_id>(who, grid, block, lds_bytes, st, a);
        return launch_kernel<mlp_forward_kernel<R.value, L.value, MODE, 0>, LDS_DYN_MAX, prof_id>(who, grid, block, lds_bytes, st, a);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}

extern "C" int mappo_mlp_forward(const float *params, const mappo_net_desc *desc, const float *x, const int32_t *rows,
                                 int64_t B, float *out, mappo_stream_t stream) {
  if (int rc = check_desc(desc, "mlp_forward")) return rc;
  MAPPO_REQUIRE(params && x && out && B > 0, "mlp_forward: bad arguments");
  FwdArgs a = {};
  a.params = params; a.x = x; a.rows = rows; a.out = out; a.desc = *desc; a.B = B;
  return launch_forward<0>(a, as_stream(stream), "mlp_forward");
}

extern "C" int mappo_mlp_features(const float *params, const mappo_net_desc *desc, const float *x, const int32_t *rows,
                                  int64_t B, float *featT, mappo_stream_t stream) {
  if (int rc = check_desc_trunk(desc, "mlp_features")) return rc;
  MAPPO_REQUIRE(params && x && featT && B > 0, "mlp_features: bad arguments");
  FwdArgs a = {};
  a.params = params; a.x = x; a.rows = rows; a.out = featT; a.desc = *desc; a.B = B;
  if (desc->in_dim <= MAXD) return launch_features16(a, as_stream(stream));
  return launch_forward<2>(a, as_stream(stream), "mlp_features");
}

// wide-input branch of mappo_mlp_features_seq (gru_train16.hip): the one-launch wide forward with the blocked output form
int mlp_features_blocked_wide_(const float *params, const mappo_net_desc *desc, const float *x, const int32_t *rows, int64_t B,
                               float *out_blocked, mappo_stream_t stream) {
  if (int rc = check_desc_trunk(desc, "mlp_features_seq")) return rc;
  MAPPO_REQUIRE(desc->in_dim > MAXD && desc->in_dim <= 512 && (B & 15) == 0, "mlp_features_seq: wide inputs need in_dim <= 512 and Nc %% 16 == 0");
  FwdArgs a = {};
  a.params = params; a.x = x; a.rows = rows; a.out = out_blocked; a.desc = *desc; a.B = B; a.out_blocked = 1;
  return launch_forward<2>(a, as_stream(stream), "mlp_features_seq");
}

extern "C" int mappo_actor_act(const float *params, const mappo_net_desc *desc, const float *obs, const float *avail,
                               int64_t B, int32_t deterministic, uint64_t seed, uint64_t counter,
                               const uint64_t *counter_dev, float *actions, float *logp, mappo_stream_t stream) {
  if (int rc = check_desc(desc, "actor_act")) return rc;
  MAPPO_REQUIRE(params && obs && actions && logp && B > 0, "actor_act: bad arguments");
  FwdArgs a = {};
  a.params = params; a.x = obs; a.rows = nullptr; a.avail = avail; a.actions = actions; a.logp = logp; a.desc = *desc;
  a.B = B; a.deterministic = deterministic; a.seed = seed; a.counter = counter; a.counter_dev = counter_dev;
  return launch_forward<1>(a, as_stream(stream), "actor_act");
}

// get_actions of a MultiDiscrete policy: mappo_actor_act's kernel (same logits, bit for bit) with one sample / argmax per head
extern "C" int mappo_actor_act_md(const float *params, const mappo_net_desc *desc, const float *obs, const float *avail,
                                  const int32_t *head_dims, int32_t n_heads, int64_t B, int32_t deterministic, uint64_t seed,
                                  uint64_t counter, const uint64_t *counter_dev, float *actions, float *logp, mappo_stream_t stream) {
  MdHeads md;
  if (int rc = check_md(desc, head_dims, n_heads, avail, "actor_act_md", md)) return rc;
  MAPPO_REQUIRE(params && obs && actions && logp && B > 0, "actor_act_md: bad arguments");
  MAPPO_CLEAR_STICKY();
  FwdArgs a = {};
  a.params = params; a.x = obs; a.actions = actions; a.logp = logp; a.desc = *desc;
  a.B = B; a.deterministic = deterministic; a.seed = seed; a.counter = counter; a.counter_dev = counter_dev;
  // the launch shape of launch_forward<1> for narrow inputs
  const int64_t n_tiles = (B + TS - 1) / TS;
  const int nw = fit_waves(a.desc, n_tiles >= 4 ? 4 : (n_tiles >= 2 ? 2 : 1));
  a.off = net_offsets(a.desc);
  a.map = lds_map(a.desc, nw);
  const size_t lds_bytes = (size_t)a.map.total * sizeof(float);
  MAPPO_REQUIRE(lds_bytes <= LDS_DYN_MAX, "actor_act_md: needs %zu B of LDS", lds_bytes);
  int64_t nb = (n_tiles + nw - 1) / nw;
  if (nb > NUM_CU) nb = NUM_CU;
  dim3 grid((unsigned)nb), block(WAVE * nw);
  const bool xw = a.desc.in_dim > 32;
  hipStream_t st = as_stream(stream);
  if (int rc = dispatch_relu_ln<1>(a.desc.use_relu != 0, a.desc.layer_N, [&](auto R, auto L) {
        if (xw) return launch_kernel<mlp_forward_md_kernel<R.value, L.value, 1>, LDS_DYN_MAX, MAPPO_PROF_ACT>("actor_act_md", grid, block, lds_bytes, st, a, md);
        return launch_kernel<mlp_forward_md_kernel<R.value, L.value, 0>, LDS_DYN_MAX, MAPPO_PROF_ACT>("actor_act_md", grid, block, lds_bytes, st, a, md);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH("actor_act_md");
  return MAPPO_OK;
}

// ---- one wave per 16-sample tile (mlp_upd16.h) ---------------------------------------------------------------------
#define UPD16_WAVES (UPD16_THREADS / WAVE)
static size_t upd16_lds_floats(const mappo_net_desc &d, bool actor) {
  const bool w = d.in_dim > 32;
  if (actor) {
    if (d.layer_N > 0) return w ? L16<1, 1, true>::TOTAL : L16<1, 1, false>::TOTAL;
    return w ? L16<0, 1, true>::TOTAL : L16<0, 1, false>::TOTAL;
  }
  if (d.layer_N > 0) return w ? L16<1, 2, true>::TOTAL : L16<1, 2, false>::TOTAL;
  return w ? L16<0, 2, true>::TOTAL : L16<0, 2, false>::TOTAL;
}
// The layout must also fit: L16<1, 1, true> (actor, 33..64 inputs, layer_N = 1) needs 171 072 B > UPD16_LDS_MAX, so that actor
// takes the pair kernel (mlp_upd2.h), in the single and in the dual launch.
static bool upd16_eligible(const mappo_net_desc &d, bool actor) {
  return d.in_dim <= MAXD && d.layer_N <= 1 && !d.recurrent && (actor ? d.out_dim <= 16 : d.out_dim == 1) &&
         upd16_lds_floats(d, actor) * sizeof(float) <= UPD16_LDS_MAX;
}
// MFMA instructions per 16-sample tile (+ a flat allowance for the VALU phases): the share of the chip a network gets
static int upd16_tile_cost(const mappo_net_desc &d, bool actor) {
  const int C = (d.in_dim + 3) >> 2, nbk = d.in_dim > 32 ? 4 : 2;
  int c = 4 * C + 16 * nbk + 40;
  if (d.layer_N > 0) c += 3 * 64;
  if (actor) c += 16 + 16 + 4 * ((d.out_dim + 3) >> 2);
  return c;
}
// trunk backward (gradient arriving at the trunk output; recurrent networks): same kernels, no head
static bool upd16_trunk_eligible(const mappo_net_desc &d) {
  return d.in_dim <= MAPPO_MAX_IN_DIM && d.layer_N <= 1;
}
static size_t upd16_trunk_lds_floats(const mappo_net_desc &d) {
  if (d.in_dim > MAXD) return d.layer_N > 0 ? L16<1, 3, true, true>::TOTAL : L16<0, 3, true, true>::TOTAL;
  const bool w = d.in_dim > 32;
  if (d.layer_N > 0) return w ? L16<1, 3, true>::TOTAL : L16<1, 3, false>::TOTAL;
  return w ? L16<0, 3, true>::TOTAL : L16<0, 3, false>::TOTAL;
}
// ---- wide inputs through the 16-sample-tile kernels ----
static bool upd16x_eligible(const mappo_net_desc &d, bool actor) {
  return d.in_dim > MAXD && d.in_dim <= MAPPO_MAX_IN_DIM && d.layer_N <= 1 && !d.recurrent && (actor ? d.out_dim <= 16 : d.out_dim == 1);
}
static int64_t wide_z1_offset(int64_t B) { return wide16_z1_offset(B); }     // workspace layout: mlp_wide16.h (>= the [64][B] | mean0 | rstd0 of the round-1 kernels)

// The layout a producer leaves in a wide workspace is a pure function of (network descriptor, producer): mappo_wide_layout.
// The caller passes it on to mappo_wide_l1_backward — no host-side state, nothing keyed by pointers.
static int wide_layout_of(const mappo_net_desc &d, int producer) {
  if (producer == MAPPO_PRODUCER_TRUNK_BACKWARD) return upd16_trunk_eligible(d) ? MAPPO_WIDE_LAYOUT_BLOCKED : MAPPO_WIDE_LAYOUT_FEATURE_MAJOR;
  if (producer == MAPPO_PRODUCER_ACTOR_UPDATE || producer == MAPPO_PRODUCER_CRITIC_UPDATE)
    return upd16x_eligible(d, producer == MAPPO_PRODUCER_ACTOR_UPDATE) ? MAPPO_WIDE_LAYOUT_BLOCKED : MAPPO_WIDE_LAYOUT_FEATURE_MAJOR;
  return MAPPO_WIDE_LAYOUT_FEATURE_MAJOR;                        // mappo_mlp_backward (external gradient): K-chunked kernel
}
extern "C" int32_t mappo_wide_layout(const mappo_net_desc *desc, int32_t producer) {
  if (!desc || producer < MAPPO_PRODUCER_MLP_BACKWARD || producer > MAPPO_PRODUCER_TRUNK_BACKWARD) {
    mappo_set_error("wide_layout: bad arguments");
    return MAPPO_EINVAL;
  }
  return wide_layout_of(*desc, producer);
}
static size_t upd16x_lds_floats(const mappo_net_desc &d, bool actor) {
  if (actor) return d.layer_N > 0 ? L16<1, 1, true, true>::TOTAL : L16<0, 1, true, true>::TOTAL;
  return d.layer_N > 0 ? L16<1, 2, true, true>::TOTAL : L16<0, 2, true, true>::TOTAL;
}
// offsets, slab range and LDS check of one network's 16-sample-tile launch; wide: the upd16x form (layer 1 in mlp_wide16.h)
static int prep16(Upd16Args &a, bool actor, bool wide, const char *who) {
  UpdArgs &u = a.u;
  u.off = net_offsets(u.desc);
  MAPPO_REQUIRE(u.slab_col0 >= 0 && u.slab_col0 + u.off.total <= u.slab_stride, "%s: slab column range", who);
  const size_t lds_bytes = (wide ? upd16x_lds_floats(u.desc, actor) : upd16_lds_floats(u.desc, actor)) * sizeof(float);
  MAPPO_REQUIRE(lds_bytes <= UPD16_LDS_MAX, "%s: needs %zu B of LDS", who, lds_bytes);
  a.zero_row0 = a.zero_row1 = 0; a.zero_col0 = 0; a.zero_cols = 0; a.zero_partials = nullptr;
  return MAPPO_OK;
}
// layer 1 of the 16-sample-tile update path in K slices (mlp_wide_sliced.h): beyond the tuned kernels' 512 columns, and only there.
// Experiment build -DWIDE_EXP_SLICED (scripts/exp_build.py, never the product library): MAPPO_WIDE_SLICED=1 then takes it at every
// wide width, for the A/B against the tuned kernels in DESIGN.md §5.
static bool wide_sliced_l1(int in_dim) {
#ifdef WIDE_EXP_SLICED
  static const bool forced = getenv("MAPPO_WIDE_SLICED") && atoi(getenv("MAPPO_WIDE_SLICED")) != 0;
  if (forced && in_dim > MAXD) return true;
#endif
  return in_dim > WIDE_TUNED_MAX_D;
}
// z1 = b1' + W1' xhat0 and the row statistics, one launch (mlp_wide16.h; beyond its 512 columns mlp_wide_sliced.h)
static int launch_wide_l1_fwd(const float *params, const mappo_net_desc &d, const NetOff &o, const float *x, const int32_t *rows, int64_t B,
                              float *z1, float *mean0, float *rstd0, hipStream_t st, const char *who) {
  Wide16Args w = {};
  w.params = params; w.x = x; w.rows = rows; w.z1 = z1; w.mean0 = mean0; w.rstd0 = rstd0; w.B = B; w.D = d.in_dim;
  w.w1 = o.w1; w.b1 = o.b1; w.fn_w = d.use_feature_norm ? o.fn_w : -1; w.fn_b = d.use_feature_norm ? o.fn_b : -1;
  const int64_t n_groups = ((B + 15) / 16 + 7) / 8;
  dim3 grid((unsigned)(n_groups < NUM_CU ? n_groups : NUM_CU));
  if (wide_sliced_l1(d.in_dim)) {
    const dim3 gs((unsigned)(n_groups < 2 * NUM_CU ? n_groups : 2 * NUM_CU));      // (workgroups stride over the tile groups; 200 VGPRs: one resident per CU)
    if (int rcl = wide_sliced_launch_l1_fwd(w, gs, st)) return rcl;
  } else if (int rcl = wide16_launch_l1_fwd(w, grid, st)) return rcl;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}

// workgroups of the dual launch: the chip's 256 CUs split by the networks' tile costs (few tiles: one tile per wave)
static void upd16_split(const mappo_net_desc &da, const mappo_net_desc &dc, int64_t B, int &nA, int &nC) {
  const int64_t n_tiles = (B + 15) / 16;
  const int64_t want = (n_tiles + UPD16_WAVES - 1) / UPD16_WAVES;
  const int ca = upd16_tile_cost(da, true), cc = upd16_tile_cost(dc, false);
  int a = (int)((int64_t)NUM_CU * ca / (ca + cc));
  if (const char *e = getenv("MAPPO_UPD16_NA")) a = atoi(e);   // diagnostic override of the actor's share (scripts/time_dual.py)
  a = a < 64 ? 64 : (a > NUM_CU - 64 ? NUM_CU - 64 : a);
  int c = NUM_CU - a;
  nA = (int)(want < a ? want : a);
  nC = (int)(want < c ? want : c);
}

extern "C" int32_t mappo_mlp_backward_slabs(int64_t B) {
  // number of slabs an update/backward launch writes: one per workgroup, at most one workgroup per CU
  int64_t n_tiles = (B + TS - 1) / TS;
  return (int32_t)(n_tiles < NUM_CU ? n_tiles : NUM_CU);
}

template <int HEAD>
static int launch_update(UpdArgs &a, hipStream_t st, const char *who) {
  MAPPO_CLEAR_STICKY();
  const mappo_net_desc &d = a.desc;
  a.off = net_offsets(d);
  MAPPO_REQUIRE(a.slab_col0 >= 0 && a.slab_col0 + a.off.total <= a.slab_stride, "%s: slab column range", who);
  const int LN = d.layer_N;
  const bool relu = d.use_relu != 0;
  a.p_red = (HEAD == 3 && d.recurrent) ? a.off.gru_wih : a.off.total;
  int nb = mappo_mlp_backward_slabs(a.B);          // every slab the caller sized for is written: grid == that count
  if (a.n_blocks > 0) {                            // caller-chosen grid (actor and critic side by side on disjoint CUs)
    MAPPO_REQUIRE(a.n_blocks <= NUM_CU, "%s: n_blocks %d > %d", who, a.n_blocks, NUM_CU);
    nb = a.n_blocks < nb ? a.n_blocks : nb;
  }
#ifdef MLP_STAMPS
  a.stamps = g_stamp_host;
  a.stamps_waves = g_stamp_waves_host;
#endif
  int rc;
  const bool trunk16 = HEAD == 3 && upd16_trunk_eligible(d);
  const bool loss16 = (HEAD == 1 || HEAD == 2) && (d.in_dim <= MAXD ? upd16_eligible(d, HEAD == 1) : upd16x_eligible(d, HEAD == 1));
  if (loss16 || trunk16) {
    // one wave per 16-sample tile (mlp_upd16.h), layer_N <= 1.  Wide inputs (upd16x): layer-1 forward as its own kernel
    // (mlp_wide16.h), then the update kernel from z1 on; the caller's mappo_wide_l1_backward turns dz1 + the row statistics into
    // the W1 / feature-norm gradients
    const bool x16 = d.in_dim > MAXD;
    if (x16) {
      MAPPO_REQUIRE(a.wide_ws, "%s: in_dim %d needs the wide workspace (mappo_wide_workspace_floats)", who, d.in_dim);
      if (int rcw = launch_wide_l1_fwd(a.params, d, a.off, a.x, a.rows, a.B, a.wide_ws + wide_z1_offset(a.B), a.wide_ws + 64 * wide16_bp(a.B),
                                       a.wide_ws + 65 * wide16_bp(a.B), st, who))
        return rcw;
    }
    Upd16Args a16 = {};                    // (zero_* = 0: nothing to zero-fill in a single-network launch)
    a16.u = a;
    size_t lds_floats;
    if (HEAD == 3) {
      lds_floats = upd16_trunk_lds_floats(d);
      MAPPO_REQUIRE(lds_floats * sizeof(float) <= UPD16_LDS_MAX, "%s: needs %zu B of LDS", who, lds_floats * sizeof(float));
    } else {
      if (int rc16 = prep16(a16, HEAD == 1, x16, who)) return rc16;
      lds_floats = x16 ? upd16x_lds_floats(d, HEAD == 1) : upd16_lds_floats(d, HEAD == 1);
    }
    const size_t lds_bytes = lds_floats * sizeof(float);
    dim3 grid((unsigned)nb), block(WAVE * UPD16_WAVES);
    const bool wide = d.in_dim > 32;
    rc = dispatch_relu_ln<1>(relu, LN, [&](auto R, auto L) {
      return x16 ? upd16x_inst<R.value, L.value>(HEAD, grid, block, lds_bytes, st, a16) : upd16_inst<R.value, L.value>(HEAD, wide, grid, block, lds_bytes, st, a16);
    });
  } else if (d.in_dim <= MAXD) {
    // pair kernel (mlp_upd2.h): n_pairs tiles in flight per workgroup, two waves each
    const int np = fit_waves(d, 4);
    a.map = lds_map(d, np);
    const size_t lds_bytes = (size_t)a.map.total * sizeof(float);
    MAPPO_REQUIRE(lds_bytes <= LDS_DYN_MAX, "%s: needs %zu B of LDS", who, lds_bytes);
    a.red_base = 0;
    const int tile_area = np * a.map.wave_stride, vec_floats = 2 * np * (3 * (LN + 1) + 3) * 64;
    a.n_regions = (np > 1 && 2 * a.p_red + vec_floats <= tile_area) ? 2 : 1;
    MAPPO_REQUIRE(a.n_regions * a.p_red + vec_floats <= tile_area, "%s: reduction buffer too small", who);
    dim3 grid((unsigned)nb), block(2 * WAVE * np);
    const bool wide = d.in_dim > 32;
    rc = dispatch_relu_ln(relu, LN, [&](auto R, auto L) { return upd2_inst<R.value, L.value, HEAD>(wide, grid, block, lds_bytes, st, a, who); });
  } else {
    // wide inputs, K-chunked kernel (mlp_upd.h): one wave per tile; W1 / feature-norm gradients come from wide_l1_bwd_kernel
    const int nw = fit_waves(d, UPD_THREADS / WAVE);
    a.map = lds_map(d, nw);
    const size_t lds_bytes = (size_t)a.map.total * sizeof(float);
    MAPPO_REQUIRE(lds_bytes <= LDS_DYN_MAX, "%s: needs %zu B of LDS", who, lds_bytes);
    a.red_base = a.off.b1;
    MAPPO_REQUIRE(a.wide_ws, "%s: in_dim %d needs the wide workspace (mappo_wide_workspace_floats)", who, d.in_dim);
    const int p_span = a.p_red - a.red_base;
    a.n_regions = (nw > 1 && nw * a.map.wave_stride >= 2 * p_span) ? 2 : 1;
    MAPPO_REQUIRE(nw * a.map.wave_stride >= a.n_regions * p_span, "%s: reduction buffer too small", who);
    dim3 grid((unsigned)nb), block(WAVE * nw);
    rc = dispatch_relu_ln(relu, LN, [&](auto R, auto L) { return upd_inst<R.value, L.value, HEAD>(grid, block, lds_bytes, st, a, who); });
  }
  if (rc) return rc;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}

extern "C" int mappo_mlp_backward(const float *params, const mappo_net_desc *desc, const float *x, const int32_t *rows,
                                  int64_t B, const float *dout, float *slabs, int64_t slab_stride, int64_t slab_col0,
                                  float *wide_ws, mappo_stream_t stream) {
  if (int rc = check_desc(desc, "mlp_backward")) return rc;
  MAPPO_REQUIRE(params && x && dout && slabs && B > 0, "mlp_backward: bad arguments");
  UpdArgs a = {};
  a.params = params; a.x = x; a.rows = rows; a.dout = dout; a.slabs = slabs; a.slab_stride = slab_stride;
  a.slab_col0 = slab_col0; a.desc = *desc; a.B = B; a.wide_ws = wide_ws;
  return launch_update<0>(a, as_stream(stream), "mlp_backward");
}

extern "C" int mappo_trunk_backward(const float *params, const mappo_net_desc *desc, const float *x, const int32_t *rows,
                                    int64_t B, const float *dHT, float *slabs, int64_t slab_stride, int64_t slab_col0,
                                    float *wide_ws, mappo_stream_t stream) {
  if (int rc = check_desc_trunk(desc, "trunk_backward")) return rc;
  MAPPO_REQUIRE(params && x && dHT && slabs && B > 0, "trunk_backward: bad arguments");
  UpdArgs a = {};
  a.params = params; a.x = x; a.rows = rows; a.dHT = dHT; a.slabs = slabs; a.slab_stride = slab_stride;
  a.slab_col0 = slab_col0; a.desc = *desc; a.B = B; a.wide_ws = wide_ws;
  return launch_update<3>(a, as_stream(stream), "trunk_backward");
}

// the same for the sequence-tiled minibatch of the recurrent training pass: d(trunk output) arrives BLOCKED per (t, 16 sequences)
// tile (the d x component gru16_bwd_kernel leaves in its scratch); in_dim <= 64
extern "C" int mappo_trunk_backward_seq(const float *params, const mappo_net_desc *desc, const float *x, const int32_t *rows,
                                        int32_t L, int32_t Nc, const float *dx_blocked, float *slabs, int64_t slab_stride,
                                        int64_t slab_col0, float *wide_ws, mappo_stream_t stream) {
  if (int rc = check_desc_trunk(desc, "trunk_backward_seq")) return rc;
  MAPPO_REQUIRE(params && x && dx_blocked && slabs && L > 0 && Nc > 0, "trunk_backward_seq: bad arguments");
  MAPPO_REQUIRE(desc->in_dim <= 512 && desc->layer_N <= 1, "trunk_backward_seq: in_dim %d > 512 or layer_N %d > 1 take mappo_trunk_backward", desc->in_dim, desc->layer_N);
  MAPPO_REQUIRE(desc->in_dim <= MAXD || (Nc & 15) == 0, "trunk_backward_seq: wide inputs need Nc %% 16 == 0 (Nc = %d)", Nc);
  UpdArgs a = {};
  a.params = params; a.x = x; a.rows = rows; a.dHT = dx_blocked; a.slabs = slabs; a.slab_stride = slab_stride;
  a.slab_col0 = slab_col0; a.desc = *desc; a.B = (int64_t)L * Nc; a.seq_nc = Nc; a.wide_ws = wide_ws;
  return launch_update<3>(a, as_stream(stream), "trunk_backward_seq");
}

extern "C" int64_t mappo_update_partials_bytes(void) { return (int64_t)NUM_CU * 4 * sizeof(double); }

extern "C" int mappo_actor_update(const float *params, const mappo_net_desc *desc, const float *obs, const int32_t *rows,
                                  int64_t B, const float *avail, const float *actions, const float *old_logp,
                                  const float *adv, const float *active, const double *mb_moments,
                                  const mappo_ppo_cfg *cfg, float *slabs, int64_t slab_stride, int64_t slab_col0,
                                  double *partials, float *wide_ws, int32_t n_blocks, mappo_stream_t stream) {
  if (int rc = check_desc(desc, "actor_update")) return rc;
  MAPPO_REQUIRE(params && obs && actions && old_logp && adv && active && mb_moments && cfg && slabs && partials && B > 0,
                "actor_update: bad arguments");
  UpdArgs a = {};
  a.params = params; a.x = obs; a.rows = rows; a.slabs = slabs; a.slab_stride = slab_stride; a.slab_col0 = slab_col0;
  a.desc = *desc; a.B = B; a.avail = avail; a.actions = actions; a.old_logp = old_logp; a.adv = adv; a.active = active;
  a.mb_moments = mb_moments; a.partials = partials; a.cfg = *cfg; a.wide_ws = wide_ws; a.n_blocks = n_blocks;
  return launch_update<1>(a, as_stream(stream), "actor_update");
}

extern "C" int mappo_critic_update(const float *params, const mappo_net_desc *desc, const float *share_obs,
                                   const int32_t *rows, int64_t B, const float *v_old, const float *returns,
                                   const float *active, const float *vn_state, const double *mb_moments,
                                   const mappo_ppo_cfg *cfg, float *slabs, int64_t slab_stride, int64_t slab_col0,
                                   double *partials, float *wide_ws, int32_t n_blocks, mappo_stream_t stream) {
  if (int rc = check_desc(desc, "critic_update")) return rc;
  MAPPO_REQUIRE(desc->out_dim == 1, "critic_update: out_dim must be 1");
  MAPPO_REQUIRE(params && share_obs && v_old && returns && active && mb_moments && cfg && slabs && partials && B > 0,
                "critic_update: bad arguments");
  MAPPO_REQUIRE(!cfg->use_valuenorm || vn_state, "critic_update: use_valuenorm needs vn_state");
  UpdArgs a = {};
  a.params = params; a.x = share_obs; a.rows = rows; a.slabs = slabs; a.slab_stride = slab_stride; a.slab_col0 = slab_col0;
  a.desc = *desc; a.B = B; a.v_old = v_old; a.returns = returns; a.active = active; a.vn_state = vn_state;
  a.mb_moments = mb_moments; a.partials = partials; a.cfg = *cfg; a.wide_ws = wide_ws; a.n_blocks = n_blocks;
  return launch_update<2>(a, as_stream(stream), "critic_update");
}

// ---- MultiDiscrete actor (multi-head loss) on the 16-sample-tile kernels ----
// L16 of the multi-head actor: 33..64 inputs with a hidden layer drop the transposed W2' copy (L16::NOW2T), which is what makes
// that shape fit
static size_t upd16md_lds_floats(const mappo_net_desc &d) {
  const bool w = d.in_dim > 32;
  if (d.layer_N > 0) return w ? L16<1, 1, true, false, true>::TOTAL : L16<1, 1, false>::TOTAL;
  return w ? L16<0, 1, true>::TOTAL : L16<0, 1, false>::TOTAL;
}
static_assert(L16<1, 1, true, false, true>::TOTAL * sizeof(float) <= UPD16_LDS_MAX, "the multi-head actor's widest layout must fit");

extern "C" int mappo_actor_update_md(const float *params, const mappo_net_desc *desc, const float *obs, const int32_t *rows, int64_t B,
                                     const float *avail, const int32_t *head_dims, int32_t n_heads, const float *actions,
                                     const float *old_logp, const float *adv, const float *active, const double *mb_moments,
                                     const mappo_ppo_cfg *cfg, float *slabs, int64_t slab_stride, int64_t slab_col0, double *partials,
                                     float *wide_ws /*unused: in_dim <= 64*/, int32_t n_blocks, mappo_stream_t stream) {
  (void)wide_ws;
  MdHeads md;
  if (int rc = check_md(desc, head_dims, n_heads, avail, "actor_update_md", md)) return rc;
  MAPPO_REQUIRE(params && obs && actions && old_logp && adv && active && mb_moments && cfg && slabs && partials && B > 0,
                "actor_update_md: bad arguments");
  MAPPO_REQUIRE(n_blocks >= 0 && n_blocks <= NUM_CU, "actor_update_md: n_blocks %d outside [0,%d]", n_blocks, NUM_CU);
  Upd16Args a16 = {};
  UpdArgs &a = a16.u;
  a.params = params; a.x = obs; a.rows = rows; a.slabs = slabs; a.slab_stride = slab_stride; a.slab_col0 = slab_col0;
  a.desc = *desc; a.B = B; a.actions = actions; a.old_logp = old_logp; a.adv = adv; a.active = active;
  a.mb_moments = mb_moments; a.partials = partials; a.cfg = *cfg; a.n_blocks = n_blocks;
  a.off = net_offsets(a.desc);
  MAPPO_REQUIRE(slab_col0 >= 0 && slab_col0 + a.off.total <= slab_stride, "actor_update_md: slab column range");
  MAPPO_CLEAR_STICKY();
  int nb = mappo_mlp_backward_slabs(B);
  if (n_blocks > 0) nb = n_blocks < nb ? n_blocks : nb;
  const size_t lds_bytes = upd16md_lds_floats(a.desc) * sizeof(float);
  dim3 grid((unsigned)nb), block(WAVE * UPD16_WAVES);
  const bool wide = a.desc.in_dim > 32;
  if (int rc = dispatch_relu_ln<1>(a.desc.use_relu != 0, a.desc.layer_N, [&](auto R, auto L) {
        return upd16md_inst<R.value, L.value>(wide, grid, block, lds_bytes, as_stream(stream), a16, md);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH("actor_update_md");
  return MAPPO_OK;
}

// mappo_actor_critic_update for a MultiDiscrete actor.  Slab / partial rows per network: mappo_dual_update_slabs of the two
// descriptors, as for the Discrete launch (an actor that the Discrete 16-sample-tile kernel cannot take — 33..64 inputs with a
// hidden layer — gets that count of workgroups for each network).
extern "C" int mappo_actor_critic_update_md(const float *actor_params, const mappo_net_desc *actor_desc, const float *obs,
                                            const float *critic_params, const mappo_net_desc *critic_desc, const float *share_obs,
                                            const int32_t *rows, int64_t B, const float *avail, const int32_t *head_dims,
                                            int32_t n_heads, const float *actions, const float *old_logp, const float *adv,
                                            const float *active, const float *v_old, const float *returns, const float *vn_state,
                                            const double *mb_moments, const mappo_ppo_cfg *cfg, float *slabs, int64_t slab_stride,
                                            int64_t actor_col0, int64_t critic_col0, double *actor_partials, double *critic_partials,
                                            mappo_stream_t stream) {
  MdHeads md;
  if (int rc = check_md(actor_desc, head_dims, n_heads, avail, "actor_critic_update_md", md)) return rc;
  if (int rc = check_desc(critic_desc, "actor_critic_update_md")) return rc;
  MAPPO_REQUIRE(critic_desc->in_dim <= MAXD && critic_desc->layer_N <= 1, "actor_critic_update_md: critic in_dim %d > %d or layer_N %d > 1",
                critic_desc->in_dim, MAXD, critic_desc->layer_N);
  MAPPO_REQUIRE(actor_desc->layer_N == critic_desc->layer_N && actor_desc->use_relu == critic_desc->use_relu,
                "actor_critic_update_md: actor and critic must share layer_N and the activation");
  MAPPO_REQUIRE(critic_desc->out_dim == 1, "actor_critic_update_md: critic out_dim must be 1");
  MAPPO_REQUIRE(actor_params && critic_params && obs && share_obs && actions && old_logp && adv && active && v_old && returns && mb_moments &&
                    cfg && slabs && actor_partials && critic_partials && B > 0, "actor_critic_update_md: bad arguments");
  MAPPO_REQUIRE(!cfg->use_valuenorm || vn_state, "actor_critic_update_md: use_valuenorm needs vn_state");
  Dual16Args d = {};
  UpdArgs &a = d.a.u, &c = d.c.u;
  a.params = actor_params; a.x = obs; a.rows = rows; a.slabs = slabs; a.slab_stride = slab_stride; a.slab_col0 = actor_col0;
  a.desc = *actor_desc; a.B = B; a.actions = actions; a.old_logp = old_logp; a.adv = adv; a.active = active;
  a.mb_moments = mb_moments; a.partials = actor_partials; a.cfg = *cfg;
  c.params = critic_params; c.x = share_obs; c.rows = rows; c.slabs = slabs; c.slab_stride = slab_stride; c.slab_col0 = critic_col0;
  c.desc = *critic_desc; c.B = B; c.v_old = v_old; c.returns = returns; c.active = active; c.vn_state = vn_state;
  c.mb_moments = mb_moments; c.partials = critic_partials; c.cfg = *cfg;
  a.off = net_offsets(a.desc);
  MAPPO_REQUIRE(actor_col0 >= 0 && actor_col0 + a.off.total <= slab_stride, "actor_critic_update_md: slab column range");
  if (int rc = prep16(d.c, false, false, "actor_critic_update_md")) return rc;
  MAPPO_CLEAR_STICKY();
  if (upd16_eligible(*actor_desc, true)) upd16_split(a.desc, c.desc, B, d.nA, d.nC);
  else d.nA = d.nC = mappo_dual_update_slabs(actor_desc, critic_desc, B);
  if (d.nA < d.nC) { d.c.zero_row0 = d.nA; d.c.zero_row1 = d.nC; d.c.zero_col0 = actor_col0; d.c.zero_cols = a.off.total; d.c.zero_partials = actor_partials; }
  if (d.nC < d.nA) { d.a.zero_row0 = d.nC; d.a.zero_row1 = d.nA; d.a.zero_col0 = critic_col0; d.a.zero_cols = c.off.total; d.a.zero_partials = critic_partials; }
  const size_t la = upd16md_lds_floats(a.desc), lc = upd16_lds_floats(c.desc, false);
  const size_t lds_bytes = (la > lc ? la : lc) * sizeof(float);
  dim3 grid((unsigned)(d.nA + d.nC)), block(WAVE * UPD16_WAVES);
  const bool wa = a.desc.in_dim > 32, wc = c.desc.in_dim > 32, relu = a.desc.use_relu != 0;
  if (int rc = dispatch_relu_ln<1>(relu, a.desc.layer_N, [&](auto R, auto L) { return upd16mdd_inst<R.value, L.value>(wa, wc, grid, block, lds_bytes, as_stream(stream), d, md); }))
    return rc;
  MAPPO_CHECK_LAUNCH("actor_critic_update_md");
  return MAPPO_OK;
}

// ---- actor + critic update in one launch --------------------------------------------------------------------------
static int prep_pair(UpdArgs &a, int np, const char *who) {
  a.off = net_offsets(a.desc);
  MAPPO_REQUIRE(a.slab_col0 >= 0 && a.slab_col0 + a.off.total <= a.slab_stride, "%s: slab column range", who);
  a.map = lds_map(a.desc, np);
  a.p_red = a.off.total;
  a.red_base = 0;
  const int LN = a.desc.layer_N;
  const int tile_area = np * a.map.wave_stride, vec_floats = 2 * np * (3 * (LN + 1) + 3) * 64;
  a.n_regions = (np > 1 && 2 * a.p_red + vec_floats <= tile_area) ? 2 : 1;
  MAPPO_REQUIRE(a.n_regions * a.p_red + vec_floats <= tile_area, "%s: reduction buffer too small", who);
  return MAPPO_OK;
}

extern "C" int32_t mappo_dual_update_slabs(const mappo_net_desc *actor_desc, const mappo_net_desc *critic_desc, int64_t B) {
  // slab rows (= loss-partial rows) the caller provides PER NETWORK for mappo_actor_critic_update; every one of them is written
  if (actor_desc && critic_desc && upd16_eligible(*actor_desc, true) && upd16_eligible(*critic_desc, false)) {
    int nA, nC;
    upd16_split(*actor_desc, *critic_desc, B, nA, nC);
    return nA > nC ? nA : nC;
  }
  int64_t n_tiles = (B + TS - 1) / TS;              // pair kernel: half the CUs each
  return (int32_t)(n_tiles < NUM_CU / 2 ? n_tiles : NUM_CU / 2);
}

extern "C" int mappo_actor_critic_update(const float *actor_params, const mappo_net_desc *actor_desc, const float *obs,
                                         const float *critic_params, const mappo_net_desc *critic_desc, const float *share_obs,
                                         const int32_t *rows, int64_t B, const float *avail, const float *actions,
                                         const float *old_logp, const float *adv, const float *active, const float *v_old,
                                         const float *returns, const float *vn_state, const double *mb_moments,
                                         const mappo_ppo_cfg *cfg, float *slabs, int64_t slab_stride, int64_t actor_col0,
                                         int64_t critic_col0, double *actor_partials, double *critic_partials,
                                         mappo_stream_t stream) {
  if (int rc = check_desc(actor_desc, "actor_critic_update")) return rc;
  if (int rc = check_desc(critic_desc, "actor_critic_update")) return rc;
  MAPPO_REQUIRE(actor_desc->in_dim <= MAXD && critic_desc->in_dim <= MAXD, "actor_critic_update: in_dim > %d takes the separate launches", MAXD);
  MAPPO_REQUIRE(actor_desc->layer_N == critic_desc->layer_N && actor_desc->use_relu == critic_desc->use_relu,
                "actor_critic_update: actor and critic must share layer_N and the activation");
  MAPPO_REQUIRE(critic_desc->out_dim == 1, "actor_critic_update: critic out_dim must be 1");
  MAPPO_REQUIRE(actor_params && critic_params && obs && share_obs && actions && old_logp && adv && active && v_old && returns && mb_moments &&
                    cfg && slabs && actor_partials && critic_partials && B > 0, "actor_critic_update: bad arguments");
  MAPPO_REQUIRE(!cfg->use_valuenorm || vn_state, "actor_critic_update: use_valuenorm needs vn_state");
  MAPPO_CLEAR_STICKY();
  UpdArgs ua = {}, uc = {};
  {
    UpdArgs &a = ua, &c = uc;
    a.params = actor_params; a.x = obs; a.rows = rows; a.slabs = slabs; a.slab_stride = slab_stride; a.slab_col0 = actor_col0;
    a.desc = *actor_desc; a.B = B; a.avail = avail; a.actions = actions; a.old_logp = old_logp; a.adv = adv; a.active = active;
    a.mb_moments = mb_moments; a.partials = actor_partials; a.cfg = *cfg;
    c.params = critic_params; c.x = share_obs; c.rows = rows; c.slabs = slabs; c.slab_stride = slab_stride; c.slab_col0 = critic_col0;
    c.desc = *critic_desc; c.B = B; c.v_old = v_old; c.returns = returns; c.active = active; c.vn_state = vn_state;
    c.mb_moments = mb_moments; c.partials = critic_partials; c.cfg = *cfg;
  }
  if (upd16_eligible(*actor_desc, true) && upd16_eligible(*critic_desc, false)) {
    Dual16Args d = {};
    d.a.u = ua; d.c.u = uc;
    UpdArgs &a = d.a.u, &c = d.c.u;
    if (int rc = prep16(d.a, true, false, "actor_critic_update")) return rc;
    if (int rc = prep16(d.c, false, false, "actor_critic_update")) return rc;
    upd16_split(a.desc, c.desc, B, d.nA, d.nC);
#ifdef MLP_STAMPS
    a.stamps = c.stamps = g_stamp_host;                          // indexed by blockIdx.x: the actor's rows first
    a.stamps_waves = c.stamps_waves = g_stamp_waves_host;
#endif
    // the network with fewer workgroups: its missing slab / partial rows are zero-filled by the other one's workgroups
    if (d.nA < d.nC) { d.c.zero_row0 = d.nA; d.c.zero_row1 = d.nC; d.c.zero_col0 = actor_col0; d.c.zero_cols = a.off.total; d.c.zero_partials = actor_partials; }
    if (d.nC < d.nA) { d.a.zero_row0 = d.nC; d.a.zero_row1 = d.nA; d.a.zero_col0 = critic_col0; d.a.zero_cols = c.off.total; d.a.zero_partials = critic_partials; }
    const size_t la = upd16_lds_floats(a.desc, true), lc = upd16_lds_floats(c.desc, false);
    const size_t lds_bytes = (la > lc ? la : lc) * sizeof(float);
    dim3 grid((unsigned)(d.nA + d.nC)), block(WAVE * UPD16_WAVES);
    const bool wa = a.desc.in_dim > 32, wc = c.desc.in_dim > 32, relu = a.desc.use_relu != 0;
    // layer_N <= 1 (upd16_eligible)
    if (int rc = dispatch_relu_ln<1>(relu, a.desc.layer_N, [&](auto R, auto L) { return upd16d_inst<R.value, L.value>(wa, wc, grid, block, lds_bytes, as_stream(stream), d); }))
      return rc;
    MAPPO_CHECK_LAUNCH("actor_critic_update");
    return MAPPO_OK;
  }
  DualArgs d = {};
  d.a = ua; d.c = uc;
  UpdArgs &a = d.a, &c = d.c;
  int np = fit_waves(a.desc, 4);
  const int npc = fit_waves(c.desc, 4);
  np = np < npc ? np : npc;
  if (int rc = prep_pair(a, np, "actor_critic_update")) return rc;
  if (int rc = prep_pair(c, np, "actor_critic_update")) return rc;
  const int ta = a.map.total, tc = c.map.total;
  const size_t lds_bytes = (size_t)(ta > tc ? ta : tc) * sizeof(float);
  MAPPO_REQUIRE(lds_bytes <= LDS_DYN_MAX, "actor_critic_update: needs %zu B of LDS", lds_bytes);
  d.nA = d.nC = mappo_dual_update_slabs(nullptr, nullptr, B);
#ifdef MLP_STAMPS
  a.stamps = c.stamps = nullptr;
#endif
  dim3 grid((unsigned)(d.nA + d.nC)), block(2 * WAVE * np);
  const bool wa = a.desc.in_dim > 32, wc = c.desc.in_dim > 32, relu = a.desc.use_relu != 0;
  if (int rc = dispatch_relu_ln(relu, a.desc.layer_N, [&](auto R, auto L) { return upd2d_inst<R.value, L.value>(wa, wc, grid, block, lds_bytes, as_stream(stream), d); }))
    return rc;
  MAPPO_CHECK_LAUNCH("actor_critic_update");
  return MAPPO_OK;
}

// ---- the dual launches of several agents in one (mlp_update16_group_kernel) -----------------------------------------------------
// Every check comes before the launch and names the job; a job passes exactly when mappo_actor_critic_update would serve it with
// the 16-sample-tile dual kernel, and its workgroup counts are that call's (upd16_split).
extern "C" int32_t mappo_update_group_accepts(const mappo_net_desc *actor_desc, const mappo_net_desc *critic_desc) {
  if (!actor_desc || !critic_desc) return 0;
  const mappo_net_desc &a = *actor_desc, &c = *critic_desc;
  return a.hidden == HID && c.hidden == HID && a.in_dim >= 1 && c.in_dim >= 1 && a.out_dim >= 1 && a.layer_N >= 0 && a.layer_N == c.layer_N &&
         a.use_relu == c.use_relu && (a.use_feature_norm != 0) == (c.use_feature_norm != 0) && upd16_eligible(a, true) && upd16_eligible(c, false);
}

extern "C" int mappo_actor_critic_update_group(const mappo_update_job *jobs, int32_t n_jobs, mappo_stream_t stream) {
  const char *who = "actor_critic_update_group";
  MAPPO_REQUIRE(n_jobs >= 1 && n_jobs <= MAPPO_MAX_GROUP, "%s: n_jobs=%d outside [1,%d] (job count)", who, n_jobs, MAPPO_MAX_GROUP);
  MAPPO_REQUIRE(jobs, "%s: null job array (job 0)", who);
  Group16Args g = {};
  g.n_jobs = n_jobs;
  const mappo_net_desc &a0 = jobs[0].actor_desc;
  g.use_feature_norm = a0.use_feature_norm != 0;
  size_t lds_floats = 0;
  int blocks = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const mappo_update_job &J = jobs[j];
    const mappo_net_desc &da = J.actor_desc, &dc = J.critic_desc;
    MAPPO_REQUIRE(da.hidden == HID && dc.hidden == HID, "%s: job %d: hidden_size %d / %d unsupported (kernels are tiled for %d)", who, j,
                  da.hidden, dc.hidden, HID);
    MAPPO_REQUIRE(da.in_dim >= 1 && dc.in_dim >= 1 && da.out_dim >= 1, "%s: job %d: in_dim %d / %d, out_dim %d must be positive", who, j,
                  da.in_dim, dc.in_dim, da.out_dim);
    MAPPO_REQUIRE(da.in_dim <= MAXD && dc.in_dim <= MAXD, "%s: job %d: in_dim %d > %d (wide inputs take the single calls)", who, j,
                  da.in_dim > MAXD ? da.in_dim : dc.in_dim, MAXD);
    MAPPO_REQUIRE(!da.recurrent && !dc.recurrent, "%s: job %d: recurrent networks are not grouped", who, j);
    MAPPO_REQUIRE(da.layer_N >= 0 && da.layer_N <= 1 && dc.layer_N == da.layer_N, "%s: job %d: layer_N %d / %d (grouped: 0 or 1, shared by both networks)",
                  who, j, da.layer_N, dc.layer_N);
    MAPPO_REQUIRE(da.out_dim <= 16, "%s: job %d: out_dim %d > 16 (a Discrete head of at most 16 actions; MultiDiscrete is not grouped)", who, j, da.out_dim);
    MAPPO_REQUIRE(dc.out_dim == 1, "%s: job %d: critic out_dim must be 1", who, j);
    MAPPO_REQUIRE(da.use_relu == dc.use_relu && (da.use_feature_norm != 0) == (dc.use_feature_norm != 0),
                  "%s: job %d: actor and critic must share the activation and feature normalisation", who, j);
    MAPPO_REQUIRE(upd16_eligible(da, true) && upd16_eligible(dc, false),
                  "%s: job %d: an actor with %d inputs and layer_N %d takes the pair kernel (single call only)", who, j, da.in_dim, da.layer_N);
    MAPPO_REQUIRE(da.layer_N == a0.layer_N, "%s: job %d: layer_N %d differs from job 0's %d (one launch is one kernel instance)", who, j, da.layer_N,
                  a0.layer_N);
    MAPPO_REQUIRE((da.use_relu != 0) == (a0.use_relu != 0), "%s: job %d: use_relu %d differs from job 0's %d (one launch is one kernel instance)", who,
                  j, da.use_relu, a0.use_relu);
    MAPPO_REQUIRE((da.use_feature_norm != 0) == (a0.use_feature_norm != 0),
                  "%s: job %d: use_feature_norm %d differs from job 0's %d (one launch is one kernel instance)", who, j, da.use_feature_norm,
                  a0.use_feature_norm);
    MAPPO_REQUIRE(J.actor_params && J.critic_params && J.obs && J.share_obs && J.actions && J.old_logp && J.adv && J.active && J.v_old && J.returns &&
                      J.mb_moments && J.slabs && J.actor_partials && J.critic_partials, "%s: job %d: null pointer", who, j);
    MAPPO_REQUIRE(J.B > 0, "%s: job %d: B=%lld", who, j, (long long)J.B);
    MAPPO_REQUIRE(!J.cfg.use_valuenorm || J.vn_state, "%s: job %d: use_valuenorm needs vn_state", who, j);
    const NetOff oa = net_offsets(da), oc = net_offsets(dc);
    MAPPO_REQUIRE(J.actor_col0 >= 0 && J.actor_col0 + oa.total <= J.slab_stride && J.critic_col0 >= 0 && J.critic_col0 + oc.total <= J.slab_stride,
                  "%s: job %d: slab column range", who, j);
    Group16Job &G = g.job[j];
    G.actor_params = J.actor_params; G.critic_params = J.critic_params; G.obs = J.obs; G.share_obs = J.share_obs; G.rows = J.rows;
    G.avail = J.avail; G.actions = J.actions; G.old_logp = J.old_logp; G.adv = J.adv; G.active = J.active; G.v_old = J.v_old;
    G.returns = J.returns; G.vn_state = J.vn_state; G.mb_moments = J.mb_moments; G.slabs = J.slabs;
    G.actor_partials = J.actor_partials; G.critic_partials = J.critic_partials;
    G.B = J.B; G.slab_stride = J.slab_stride; G.actor_col0 = J.actor_col0; G.critic_col0 = J.critic_col0; G.cfg = J.cfg;
    G.in_a = da.in_dim; G.in_c = dc.in_dim; G.out_a = da.out_dim; G.tot_a = oa.total; G.tot_c = oc.total;
    G.block0 = blocks;
    upd16_split(da, dc, J.B, G.nA, G.nC);
    blocks += G.nA + G.nC;
    const size_t la = upd16_lds_floats(da, true), lc = upd16_lds_floats(dc, false);
    lds_floats = la > lds_floats ? la : lds_floats;
    lds_floats = lc > lds_floats ? lc : lds_floats;
  }
  MAPPO_CLEAR_STICKY();
  const size_t lds_bytes = lds_floats * sizeof(float);      // (<= UPD16_LDS_MAX: upd16_eligible)
  dim3 grid((unsigned)blocks), block(WAVE * UPD16_WAVES);
  if (int rc = dispatch_relu_ln<1>(a0.use_relu != 0, a0.layer_N, [&](auto R, auto L) { return upd16g_inst<R.value, L.value>(grid, block, lds_bytes, as_stream(stream), g); }))
    return rc;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}

// ------------------------------------------------------------------------------------------------
// wide_l1_bwd_kernel: layer-1 weight gradient and feature-norm gradients for in_dim > 64.
//   dW1[f][k]  = sum_s dz1[f][s] * xn[k][s],   xn = xhat0 * gamma0 + beta0
//   dxn[k][s]  = sum_f W1[f][k] * dz1[f][s] ;  dgamma0[k] = sum_s dxn * xhat0 ;  dbeta0[k] = sum_s dxn
// A workgroup owns ONE 64-column chunk of W1 (blockIdx.y) and one share of the row tiles (blockIdx.x); its 4 waves
// walk row tiles, keep the chunk's 64x64 dW1 block in registers, and the per-sample-lane partial sums of the
// feature-norm gradients are reduced across lanes once at the end.  One slab row per blockIdx.x.
// ------------------------------------------------------------------------------------------------
struct WideArgs {
  const float *params, *x;
  const int32_t *rows;
  const float *wide_ws;
  float *slabs;
  int64_t slab_stride, slab_col0;
  NetOff off;
  int64_t B;
  int D, use_feature_norm;
};

__global__ __launch_bounds__(256, 1) void wide_l1_bwd_kernel(WideArgs p) {
  extern __shared__ __align__(16) float lds[];
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), l31 = lane & 31, half = lane >> 5;
  const int D = p.D, c0 = blockIdx.y * MAXD, kc = min(MAXD, D - c0);
  float *sW = lds;                                   // [64 kk][WP]  W1 chunk, k-major
  float *sG = sW + MAXD * WP, *sBt = sG + MAXD;      // gamma0 / beta0 of the chunk
  float *tD = sBt + MAXD + wave * (2 * HID * TP);    // [64 f][TP]   dz1 tile
  float *tXc = tD + HID * TP;                        // [64 kk][TP]  xhat0 tile of the chunk
  stage_w1_chunk(sW, p.params + p.off.w1, D, c0, kc);
  for (int e = threadIdx.x; e < MAXD; e += blockDim.x) {
    const bool in = e < kc;
    sG[e] = in ? (p.use_feature_norm ? p.params[p.off.fn_w + c0 + e] : 1.f) : 0.f;
    sBt[e] = (in && p.use_feature_norm) ? p.params[p.off.fn_b + c0 + e] : 0.f;
  }
  __syncthreads();
  const float *dz1T = p.wide_ws, *stats = p.wide_ws + (int64_t)HID * p.B;
  f32x16 gW[2][2], accB[2], accG[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { accB[i][r] = 0.f; accG[i][r] = 0.f; }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) gW[i][j][r] = 0.f;
  }
  const int64_t n_tiles = (p.B + TS - 1) / TS;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t base = tile * TS;
    const int n_valid = (int)min((int64_t)TS, p.B - base);
    const bool ok = l31 < n_valid;
    // dz1 tile [f][s] (feature-major source: 128-B segments)
    {
      float v[HID / 2];                                // lane (s = l31, half) takes features 2 i + half: all 32 loads in flight
      const int64_t col = base + min(l31, n_valid - 1);
#pragma unroll
      for (int i = 0; i < HID / 2; ++i) v[i] = dz1T[(int64_t)(2 * i + half) * p.B + col];
#pragma unroll
      for (int i = 0; i < HID / 2; ++i) tD[(2 * i + half) * TP + l31] = ok ? v[i] : 0.f;
    }
    const int64_t row = ok ? (p.rows ? (int64_t)p.rows[base + l31] : base + l31) : 0;
    const float mean0 = ok ? stats[base + l31] : 0.f, rstd0 = ok ? stats[p.B + base + l31] : 1.f;
    wide_commit_chunk(tXc, p.x + row * D, D, c0, ok, mean0, rstd0, l31, half);
    wave_lds_sync();
    // dW1 chunk
    {
      const float g0 = sG[l31], b0 = sBt[l31], g1 = sG[32 + l31], b1 = sBt[32 + l31];
#pragma unroll 2
      for (int ss = 0; ss < TS / 2; ++ss) {
        const int s = 2 * ss + half;
        const float a0 = tD[l31 * TP + s], a1 = tD[(32 + l31) * TP + s];
        // padding samples carry dz1 = 0, padding columns carry gamma = beta = 0
        const float x0 = tXc[l31 * TP + s] * g0 + b0, x1 = tXc[(32 + l31) * TP + s] * g1 + b1;
        gW[0][0] = mfma(a0, x0, gW[0][0]);
        gW[0][1] = mfma(a0, x1, gW[0][1]);
        gW[1][0] = mfma(a1, x0, gW[1][0]);
        gW[1][1] = mfma(a1, x1, gW[1][1]);
      }
    }
    if (p.use_feature_norm) {
      f32x16 dX[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dX[t][r] = 0.f;
#pragma unroll 4
      for (int ff = 0; ff < HID / 2; ++ff) {
        const int f = 2 * ff + half;
        const float b = tD[f * TP + l31];
        dX[0] = mfma(sW[l31 * WP + f], b, dX[0]);
        dX[1] = mfma(sW[(32 + l31) * WP + f], b, dX[1]);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          accB[t][r] += dX[t][r];
          accG[t][r] += dX[t][r] * tXc[(32 * t + ROWMAP(r, half)) * TP + l31];
        }
    }
    wave_lds_sync();
  }
  // ---- cross-lane (sample) reduction of the feature-norm partial sums, through this wave's tiles ----
  float gFnB = 0.f, gFnW = 0.f;
  if (p.use_feature_norm) {
    wave_lds_sync();
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        tD[(32 * t + ROWMAP(r, half)) * TP + l31] = accB[t][r];
        tXc[(32 * t + ROWMAP(r, half)) * TP + l31] = accG[t][r];
      }
    wave_lds_sync();
    for (int j = 0; j < TS; ++j) { gFnB += tD[lane * TP + j]; gFnW += tXc[lane * TP + j]; }
  }
  // ---- reduce the 4 waves through LDS (reusing wave 0's tiles), write this workgroup's slab columns ----
  __syncthreads();
  float *red = sBt + MAXD;                           // >= 64*64 + 128 floats available (4 waves x 2 tiles)
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
          float old[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) old[r] = (w == 0) ? 0.f : red[(32 * ti + ROWMAP(r, half)) * MAXD + 32 * tj + l31];
#pragma unroll
          for (int r = 0; r < 16; ++r) red[(32 * ti + ROWMAP(r, half)) * MAXD + 32 * tj + l31] = old[r] + gW[ti][tj][r];
        }
      const float ob = (w == 0) ? 0.f : red[HID * MAXD + lane], og = (w == 0) ? 0.f : red[HID * MAXD + MAXD + lane];
      red[HID * MAXD + lane] = ob + gFnB;
      red[HID * MAXD + MAXD + lane] = og + gFnW;
    }
    __syncthreads();
  }
  float *slab = p.slabs + (size_t)blockIdx.x * p.slab_stride + p.slab_col0;
  for (int e = threadIdx.x; e < HID * kc; e += blockDim.x) {
    const int f = e / kc, kk = e - f * kc;
    slab[p.off.w1 + f * D + c0 + kk] = red[f * MAXD + kk];
  }
  if (p.use_feature_norm)
    for (int e = threadIdx.x; e < kc; e += blockDim.x) {
      slab[p.off.fn_b + c0 + e] = red[HID * MAXD + e];
      slab[p.off.fn_w + c0 + e] = red[HID * MAXD + MAXD + e];
    }
}

extern "C" int64_t mappo_wide_workspace_floats(int64_t B) { return wide_z1_offset(B) + (int64_t)HID * B; }     // + z1 [B][64] (mlp_wide16.h)

extern "C" int32_t mappo_wide_l1_slabs(int64_t B) {
  // slab rows mappo_wide_l1_backward may write (never more than the update launch's own mappo_mlp_backward_slabs(B))
  return mappo_mlp_backward_slabs(B);
}

extern "C" int mappo_wide_l1_backward(const float *params, const mappo_net_desc *desc, const float *x, const int32_t *rows,
                                      int64_t B, const float *wide_ws, float *slabs, int64_t slab_stride, int64_t slab_col0,
                                      int32_t layout, mappo_stream_t stream) {
  if (int rc = check_desc_trunk(desc, "wide_l1_backward")) return rc;
  MAPPO_REQUIRE(desc->in_dim > MAXD, "wide_l1_backward: in_dim %d is handled inside the update kernels", desc->in_dim);
  MAPPO_REQUIRE(params && x && wide_ws && slabs && B > 0, "wide_l1_backward: bad arguments");
  MAPPO_REQUIRE(layout == MAPPO_WIDE_LAYOUT_BLOCKED || layout == MAPPO_WIDE_LAYOUT_FEATURE_MAJOR,
                "wide_l1_backward: layout %d (pass mappo_wide_layout(desc, producer) of the launch that filled the workspace)", (int)layout);
  {
    if (layout == MAPPO_WIDE_LAYOUT_BLOCKED) {
      // 16x16x4 kernel (mlp_wide16.h): raw products, every input element read once
      const NetOff o = net_offsets(*desc);
      MAPPO_REQUIRE(slab_col0 >= 0 && slab_col0 + o.total <= slab_stride, "wide_l1_backward: slab column range");
      WideBwd16Args w = {};
      w.params = params; w.x = x; w.rows = rows; w.wide_ws = wide_ws; w.slabs = slabs; w.slab_stride = slab_stride; w.slab_col0 = slab_col0;
      w.B = B; w.D = desc->in_dim; w.w1 = o.w1; w.fn_w = desc->use_feature_norm ? o.fn_w : -1; w.fn_b = desc->use_feature_norm ? o.fn_b : -1;
      const int nch = (desc->in_dim + 63) / 64;
      w.nca = nch <= 2 ? 2 : (nch <= 4 ? 4 : 8);
      const int rows_max = mappo_mlp_backward_slabs(B);
      if (wide_sliced_l1(desc->in_dim)) {
        // 512-column slices side by side (mlp_wide_sliced.h): one workgroup per (slab row, slice), every slab row written
        w.nca = 8; w.groups = 1;
        if (int rcl = wide_sliced_launch_l1_bwd(w, dim3((unsigned)rows_max, (unsigned)((nch + 7) / 8)), as_stream(stream))) return rcl;
        MAPPO_CHECK_LAUNCH("wide_l1_backward");
        return MAPPO_OK;
      }
      w.groups = 8 / w.nca;
      if (rows_max < w.groups) w.groups = 1;
      const int gx = rows_max / w.groups;
      (void)wide16_launch_l1_bwd(w, dim3((unsigned)gx), as_stream(stream));
      MAPPO_CHECK_LAUNCH("wide_l1_backward");
      return MAPPO_OK;
    }
  }
  MAPPO_CLEAR_STICKY();
  WideArgs a = {};
  a.params = params; a.x = x; a.rows = rows; a.wide_ws = wide_ws; a.slabs = slabs; a.slab_stride = slab_stride; a.slab_col0 = slab_col0;
  a.off = net_offsets(*desc); a.B = B; a.D = desc->in_dim; a.use_feature_norm = desc->use_feature_norm;
  MAPPO_REQUIRE(slab_col0 >= 0 && slab_col0 + a.off.total <= slab_stride, "wide_l1_backward: slab column range");
  const size_t lds_bytes = (size_t)(MAXD * WP + 2 * MAXD + 4 * 2 * HID * TP) * sizeof(float);
  dim3 grid((unsigned)mappo_wide_l1_slabs(B), (unsigned)((desc->in_dim + MAXD - 1) / MAXD));
  if (int rc = launch_kernel<wide_l1_bwd_kernel, LDS_DYN_MAX>("wide_l1_backward", grid, dim3(256), lds_bytes, as_stream(stream), a)) return rc;
  MAPPO_CHECK_LAUNCH("wide_l1_backward");
  return MAPPO_OK;
}

// statistics of one fused update from the two kernels' per-workgroup partial sums (same layout as
// mappo_ppo_loss_fwd_bwd's `stats`)
__global__ __launch_bounds__(256) void update_stats_kernel(const double *__restrict__ pa, const double *__restrict__ pc, int na,
                                                          int nc, const double *__restrict__ mb_moments, int use_policy_active,
                                                          int use_value_active, double *__restrict__ stats,
                                                          double *__restrict__ acc) {
  __shared__ double smem[16 * 4];
  update_stats_body(pa, pc, na, nc, mb_moments, use_policy_active, use_value_active, stats, acc, smem);
}

extern "C" int mappo_update_stats(const double *actor_partials, int32_t n_actor, const double *critic_partials,
                                  int32_t n_critic, const double *mb_moments, const mappo_ppo_cfg *cfg, double *stats,
                                  double *acc, mappo_stream_t stream) {
  MAPPO_REQUIRE(critic_partials && mb_moments && cfg && stats && n_critic > 0 && n_actor >= 0, "update_stats: bad arguments");
  hipLaunchKernelGGL(update_stats_kernel, dim3(1), dim3(256), 0, as_stream(stream), actor_partials, critic_partials,
                     actor_partials ? (int)n_actor : 0, (int)n_critic, mb_moments, cfg->use_policy_active_masks,
                     cfg->use_value_active_masks, stats, acc);
  MAPPO_CHECK_LAUNCH("update_stats");
  return MAPPO_OK;
}

// ------------------------------------------------------------------------------------------------
// self test of the documented v_mfma_f32_32x32x2_f32 lane maps (tests/test_gpu_kernels.py)
// ------------------------------------------------------------------------------------------------
__global__ void selftest_mfma_kernel(const float *A, const float *Bm, float *Dm) {
  const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  acc = mfma(A[l31 * 2 + half], Bm[half * 32 + l31], acc);     // A[i=l31][k=half], B[k=half][j=l31]
#pragma unroll
  for (int r = 0; r < 16; ++r) Dm[ROWMAP(r, half) * 32 + l31] = acc[r];
}

extern "C" int mappo_selftest_mfma(const float *A, const float *Bm, float *D, mappo_stream_t stream) {
  MAPPO_REQUIRE(A && Bm && D, "selftest_mfma: null pointer");
  hipLaunchKernelGGL(selftest_mfma_kernel, dim3(1), dim3(WAVE), 0, as_stream(stream), A, Bm, D);
  MAPPO_CHECK_LAUNCH("selftest_mfma");
  return MAPPO_OK;
}

