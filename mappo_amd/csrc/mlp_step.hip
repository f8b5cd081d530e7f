// mlp_step.hip — host entry points of the rollout side: the fused rollout step (actor get_actions + critic get_values + MPE insert
// in one launch), the one-launch rollout episode, the trunk features of recurrent networks and the wide recurrent step.  The
// kernels are in mlp_fwd.h; the wide-input launches go through the launchers declared in mlp_launch.h.
#include "mlp_host.h"
#include <stdlib.h>

int launch_features16(const FwdArgs &a_in, hipStream_t st) {
  MAPPO_CLEAR_STICKY();
  FwdArgs a = a_in;
  const int64_t n_tiles = (a.B + 15) / 16;
  const int nw = fit_waves(a.desc, n_tiles >= 4 ? 4 : (n_tiles >= 2 ? 2 : 1));
  a.off = net_offsets(a.desc); a.map = lds_map(a.desc, nw);
  const size_t lds_bytes = (size_t)a.map.total * sizeof(float);
  MAPPO_REQUIRE(lds_bytes <= LDS_DYN_MAX, "mlp_features: needs %zu B of LDS", lds_bytes);
  int64_t nb = (n_tiles + nw - 1) / nw;
  if (nb > 2 * NUM_CU) nb = 2 * NUM_CU;                      // every workgroup stages the weights once, then walks its tiles
  dim3 grid((unsigned)nb), block(WAVE * nw);
  if (int rc = dispatch_relu_ln(a.desc.use_relu != 0, a.desc.layer_N, [&](auto R, auto L) {
        return launch_kernel<features16_kernel<R.value, L.value>, LDS_DYN_MAX>("mlp_features", grid, block, lds_bytes, st, a);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH("mlp_features");
  return MAPPO_OK;
}

extern "C" int mappo_mlp_features_dual(const float *params_a, const mappo_net_desc *desc_a, const float *x_a, float *featT_a,
                                       const float *params_c, const mappo_net_desc *desc_c, const float *x_c, float *featT_c,
                                       int64_t B, mappo_stream_t stream) {
  if (int rc = check_desc_trunk(desc_a, "mlp_features_dual")) return rc;
  if (int rc = check_desc_trunk(desc_c, "mlp_features_dual")) return rc;
  const bool sliced = desc_a->in_dim > WIDE_TUNED_MAX_D && desc_c->in_dim > WIDE_TUNED_MAX_D;
  MAPPO_REQUIRE(sliced || ((desc_a->in_dim <= MAXD) == (desc_c->in_dim <= MAXD) && desc_a->in_dim <= 512 && desc_c->in_dim <= 512),
                "mlp_features_dual: both networks narrow (in_dim <= %d), both wide (65..512) or both beyond 512 (in_dim %d / %d: run "
                "mappo_mlp_features per network)", MAXD, desc_a->in_dim, desc_c->in_dim);
  MAPPO_REQUIRE(desc_a->layer_N == desc_c->layer_N && desc_a->use_relu == desc_c->use_relu,
                "mlp_features_dual: the networks must share layer_N and the activation");
  MAPPO_REQUIRE(params_a && x_a && featT_a && params_c && x_c && featT_c && B > 0, "mlp_features_dual: bad arguments");
  MAPPO_CLEAR_STICKY();
  if (sliced) {
    // beyond the tuned wide kernels: each network's one-launch sliced forward (mlp_wide_sliced.h), one after the other
    FwdArgs a = {}, c = {};
    a.params = params_a; a.x = x_a; a.out = featT_a; a.desc = *desc_a; a.B = B;
    c.params = params_c; c.x = x_c; c.out = featT_c; c.desc = *desc_c; c.B = B;
    if (int rc = wide_sliced_forward(2, a, as_stream(stream), "mlp_features_dual")) return rc;
    return wide_sliced_forward(2, c, as_stream(stream), "mlp_features_dual");
  }
  if (desc_a->in_dim > MAXD) {
    // wide inputs: the one-launch wide forward (mlp_wide16.h) of both networks by workgroup role
    FwdArgs a = {}, c = {};
    a.params = params_a; a.x = x_a; a.out = featT_a; a.desc = *desc_a; a.B = B; a.off = net_offsets(a.desc); a.map = lds_map(a.desc, 8);
    c.params = params_c; c.x = x_c; c.out = featT_c; c.desc = *desc_c; c.B = B; c.off = net_offsets(c.desc); c.map = lds_map(c.desc, 8);
    Wide16Args wa, wc;
    size_t lba, lbc;
    dim3 ga, gc, ba, bc;
    if (int rcp = wide_forward_prepare(a, wa, lba, ga, ba, "mlp_features_dual")) return rcp;
    if (int rcp = wide_forward_prepare(c, wc, lbc, gc, bc, "mlp_features_dual")) return rcp;
    const int64_t nt16 = (B + 15) / 16;
    if (nt16 <= WIDE_SK_MAX_TILES && !getenv("MAPPO_WIDE_NO_SK")) {
      if (int rcw = wide16_launch_features_sk_dual(desc_a->use_relu != 0, desc_a->layer_N, dim3((unsigned)(2 * nt16)), lba > lbc ? lba : lbc,
                                                   as_stream(stream), wa, a, wc, c, (int)nt16))
        return rcw;
    } else if (int rcw = wide16_launch_features_dual(desc_a->use_relu != 0, desc_a->layer_N, dim3(ga.x + gc.x), ba, lba > lbc ? lba : lbc,
                                                     as_stream(stream), wa, a, wc, c, (int)ga.x))
      return rcw;
    MAPPO_CHECK_LAUNCH("mlp_features_dual");
    return MAPPO_OK;
  }
  const int64_t n_tiles = (B + 15) / 16;
  const int want = n_tiles >= 4 ? 4 : (n_tiles >= 2 ? 2 : 1);
  int nw = fit_waves(*desc_a, want);
  const int nwc = fit_waves(*desc_c, want);
  nw = nw < nwc ? nw : nwc;
  FwdArgs a = {}, c = {};
  a.params = params_a; a.x = x_a; a.out = featT_a; a.desc = *desc_a; a.B = B; a.off = net_offsets(a.desc); a.map = lds_map(a.desc, nw);
  c.params = params_c; c.x = x_c; c.out = featT_c; c.desc = *desc_c; c.B = B; c.off = net_offsets(c.desc); c.map = lds_map(c.desc, nw);
  const int totA = a.map.total, totC = c.map.total;
  const size_t lds_bytes = (size_t)(totA > totC ? totA : totC) * sizeof(float);
  MAPPO_REQUIRE(lds_bytes <= LDS_DYN_MAX, "mlp_features_dual: needs %zu B of LDS", lds_bytes);
  int64_t nb = (n_tiles + nw - 1) / nw;
  if (nb > NUM_CU) nb = NUM_CU;
  dim3 grid((unsigned)(2 * nb)), block(WAVE * nw);
  if (int rc = dispatch_relu_ln(desc_a->use_relu != 0, desc_a->layer_N, [&](auto R, auto L) {
        return launch_kernel<features16_dual_kernel<R.value, L.value>, LDS_DYN_MAX>("mlp_features_dual", grid, block, lds_bytes, as_stream(stream), a, c, (int)nb);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH("mlp_features_dual");
  return MAPPO_OK;
}

// wide-input branch of mappo_recurrent_step_dual (gru.hip): both trunks (split-K), GRU steps and heads in one launch
#define WIDE_REC_STEP_MAX_TILES 1024
int mappo_recurrent_step_dual_wide_(const float *actor_params, const mappo_net_desc *actor_desc, const float *obs, const float *actor_h0,
                                    float *actor_h_last, const float *critic_params, const mappo_net_desc *critic_desc, const float *share_obs,
                                    const float *critic_h0, float *critic_h_last, const float *masks, int32_t Nc, const float *avail,
                                    int32_t deterministic, uint64_t seed, uint64_t counter, const uint64_t *counter_dev, float *actions,
                                    float *logp, float *values, const SmacInsert *ins, mappo_stream_t stream) {
  if (int rc = check_desc_trunk(actor_desc, "recurrent_step_dual")) return rc;
  if (int rc = check_desc_trunk(critic_desc, "recurrent_step_dual")) return rc;
  MAPPO_REQUIRE(actor_desc->in_dim > MAXD && critic_desc->in_dim > MAXD && actor_desc->in_dim <= 512 && critic_desc->in_dim <= 512,
                "recurrent_step_dual: both networks wide (in_dim %d..512)", MAXD + 1);
  const int64_t nt16 = ((int64_t)Nc + 15) / 16;
  MAPPO_REQUIRE(nt16 <= WIDE_REC_STEP_MAX_TILES, "recurrent_step_dual: %d rows exceed the one-launch step (mlp_features_dual + gru_step_dual)", Nc);
  MAPPO_CLEAR_STICKY();
  FwdArgs a = {}, c = {};
  a.params = actor_params; a.x = obs; a.desc = *actor_desc; a.B = Nc; a.off = net_offsets(a.desc); a.map = lds_map(a.desc, 8);
  c.params = critic_params; c.x = share_obs; c.desc = *critic_desc; c.B = Nc; c.off = net_offsets(c.desc); c.map = lds_map(c.desc, 8);
  Wide16Args wa, wc;
  size_t lba, lbc;
  dim3 ga, gc, ba, bc;
  if (int rcp = wide_forward_prepare(a, wa, lba, ga, ba, "recurrent_step_dual")) return rcp;
  if (int rcp = wide_forward_prepare(c, wc, lbc, gc, bc, "recurrent_step_dual")) return rcp;
  WideStepIO io = {};
  io.ins = ins;
  io.actor_h0 = actor_h0; io.critic_h0 = critic_h0; io.masks = masks; io.avail = avail; io.actor_h_last = actor_h_last;
  io.critic_h_last = critic_h_last; io.actions = actions; io.logp = logp; io.values = values; io.Nc = Nc; io.deterministic = deterministic;
  io.seed = seed; io.counter = counter; io.counter_dev = counter_dev;
  if (int rcw = wide16_launch_recurrent_step_dual(actor_desc->use_relu != 0, actor_desc->layer_N, lba > lbc ? lba : lbc, as_stream(stream), wa, a,
                                                  wc, c, (int)nt16, io))
    return rcw;
  MAPPO_CHECK_LAUNCH("recurrent_step_dual");
  return MAPPO_OK;
}

// ---- fused rollout step (rollout_step_kernel): translation unit mlp_step.hip --------------------------------------
// md != NULL: the MultiDiscrete step (mappo_rollout_step_md, narrow networks with layer_N <= 1: check_md): actions / logp [B][md->n]
static int rollout_step_impl(const float *actor_params, const mappo_net_desc *actor_desc, const float *critic_params,
                             const mappo_net_desc *critic_desc, const float *obs, int64_t obs_stride_n, int64_t obs_stride_m,
                             const float *share_obs, int64_t share_stride_n, int64_t share_stride_m, int32_t M, int64_t B,
                             const float *avail, int32_t deterministic, uint64_t seed, uint64_t counter,
                             const uint64_t *counter_dev, float *actions, float *logp, float *values, float *obs_dst,
                             float *share_dst, const float *rewards, int64_t rew_stride_n, int64_t rew_stride_m,
                             const uint8_t *dones, int64_t done_stride_n, int64_t done_stride_m, float *rew_dst,
                             float *mask_dst, int32_t centralized, mappo_stream_t stream, const MdHeads *md) {
  if (int rc = check_desc(actor_desc, "rollout_step")) return rc;
  if (int rc = check_desc(critic_desc, "rollout_step")) return rc;
  const bool sliced = actor_desc->in_dim > WIDE_TUNED_MAX_D && critic_desc->in_dim > WIDE_TUNED_MAX_D;
  MAPPO_REQUIRE(sliced || ((actor_desc->in_dim <= MAXD) == (critic_desc->in_dim <= MAXD) && actor_desc->in_dim <= 512 && critic_desc->in_dim <= 512),
                "rollout_step: both networks narrow (in_dim <= %d), both wide (65..512) or both beyond 512 (in_dim %d / %d: run "
                "mappo_actor_act and mappo_mlp_forward per network)", MAXD, actor_desc->in_dim, critic_desc->in_dim);
  MAPPO_REQUIRE(actor_desc->layer_N == critic_desc->layer_N && actor_desc->use_relu == critic_desc->use_relu,
                "rollout_step: actor and critic must share layer_N and the activation");
  MAPPO_REQUIRE(critic_desc->out_dim == 1, "rollout_step: critic out_dim must be 1");
  MAPPO_REQUIRE(actor_params && critic_params && obs && share_obs && values && B > 0 && M >= 0 && (!actions == !logp),
                "rollout_step: bad arguments");                  // actions == logp == NULL: critic (+ insert) only
  MAPPO_REQUIRE(M > 0 || !obs_dst, "rollout_step: the fused insert needs the (thread, agent) row layout (M > 0)");
  MAPPO_REQUIRE(!obs_dst || (share_dst && rewards && dones && rew_dst && mask_dst && B % M == 0), "rollout_step: incomplete insert arguments");
  MAPPO_CLEAR_STICKY();
  if (sliced) {
    // beyond the tuned wide kernels: the insert as its own launch, then each network's one-launch sliced forward (mlp_wide_sliced.h)
    // reading the env's rows in place
    if (obs_dst)
      if (int rci = mappo_insert_mpe(obs, obs_stride_n, obs_stride_m, rewards, rew_stride_n, rew_stride_m, dones, done_stride_n, done_stride_m,
                                     obs_dst, share_dst, rew_dst, mask_dst, (int32_t)(B / M), M, actor_desc->in_dim, centralized, stream))
        return rci;
    if (actions) {
      FwdArgs a = {};
      a.params = actor_params; a.x = obs; a.avail = avail; a.actions = actions; a.logp = logp; a.desc = *actor_desc; a.B = B;
      a.deterministic = deterministic; a.seed = seed; a.counter = counter; a.counter_dev = counter_dev;
      a.x_M = M; a.x_sn = obs_stride_n; a.x_sm = obs_stride_m;
      if (int rc = wide_sliced_forward(1, a, as_stream(stream), "rollout_step")) return rc;
    }
    FwdArgs c = {};
    c.params = critic_params; c.x = share_obs; c.out = values; c.desc = *critic_desc; c.B = B;
    c.x_M = M; c.x_sn = share_stride_n; c.x_sm = share_stride_m;
    return wide_sliced_forward(0, c, as_stream(stream), "rollout_step");
  }
  if (actor_desc->in_dim > MAXD) {
    // Wide inputs: the insert is its own (HBM-bound: it moves the rows it copies once in, twice out) launch, the two networks share
    // one (wide_rollout_step_kernel: every CU busy for one chunk-latency chain instead of half the chip for two).
    // in_dim 256 / 512 on both networks and at most two tiles per wave: W1' staged whole, and the insert's row copies ride on the
    // forward's loads (wide_rollout_full_kernel); MAPPO_WIDE_FULL_STEP=0: the streamed form (A/B)
    const int64_t nt16_ = (B + 15) / 16;
    const bool full_step = actor_desc->in_dim == critic_desc->in_dim && (actor_desc->in_dim == 256 || actor_desc->in_dim == 512) &&
                           nt16_ <= 2 * 8 * (NUM_CU / 2) && !(getenv("MAPPO_WIDE_FULL_STEP") && atoi(getenv("MAPPO_WIDE_FULL_STEP")) == 0);
    const bool fuse_ins = full_step && obs_dst && actions && !centralized && obs_stride_m == actor_desc->in_dim &&
                          share_stride_m == critic_desc->in_dim;
    if (obs_dst && !fuse_ins)
      if (int rci = mappo_insert_mpe(obs, obs_stride_n, obs_stride_m, rewards, rew_stride_n, rew_stride_m, dones, done_stride_n, done_stride_m,
                                     obs_dst, share_dst, rew_dst, mask_dst, (int32_t)(B / M), M, actor_desc->in_dim, centralized, stream))
        return rci;
    FwdArgs a = {}, c = {};
    a.params = actor_params; a.x = obs; a.avail = avail; a.actions = actions; a.logp = logp; a.desc = *actor_desc; a.B = B;
    a.deterministic = deterministic; a.seed = seed; a.counter = counter; a.counter_dev = counter_dev;
    a.off = net_offsets(a.desc); a.map = lds_map(a.desc, 8);
    c.params = critic_params; c.x = share_obs; c.out = values; c.desc = *critic_desc; c.B = B; c.off = net_offsets(c.desc); c.map = lds_map(c.desc, 8);
    Wide16Args wa, wc;
    size_t lba, lbc;
    dim3 ga, gc, ba, bc;
    if (int rcp = wide_forward_prepare(a, wa, lba, ga, ba, "rollout_step")) return rcp;
    if (int rcp = wide_forward_prepare(c, wc, lbc, gc, bc, "rollout_step")) return rcp;
    wa.x_M = M; wa.x_sn = obs_stride_n; wa.x_sm = obs_stride_m;
    wc.x_M = M; wc.x_sn = share_stride_n; wc.x_sm = share_stride_m;
    // each network: one workgroup per 8 tiles, at most half of the chip's CUs
    const int64_t n_groups = ((B + 15) / 16 + 7) / 8;
    const int nb = (int)(n_groups < NUM_CU / 2 ? n_groups : NUM_CU / 2);
    const int nA = actions ? nb : 0;
    const dim3 grid((unsigned)(nA + nb));
    const size_t lb = lba > lbc ? lba : lbc;
    if (full_step) {
      const size_t lw = sizeof(float) * ((size_t)HID * actor_desc->in_dim + HID);      // W1' whole + folded bias; the tail's map reuses the space
      const size_t lf = lw > lb ? lw : lb;
      MAPPO_REQUIRE(lf <= 159 * 1024, "rollout_step: needs %zu B of LDS", lf);
      InsertArgs ins = {};
      if (fuse_ins) {
        wa.copy_dst = obs_dst; wc.copy_dst = share_dst;
        ins.rew = rewards; ins.rew_sn = rew_stride_n; ins.rew_sm = rew_stride_m; ins.done = dones; ins.done_sn = done_stride_n;
        ins.done_sm = done_stride_m; ins.rew_dst = rew_dst; ins.mask_dst = mask_dst; ins.N = (int)(B / M); ins.M = M;
      }
      const int rcf = actor_desc->use_relu
          ? wide16_launch_rollout_full_r<true>(actor_desc->layer_N, grid, lf, as_stream(stream), wa, a, wc, c, nA, fuse_ins ? &ins : nullptr)
          : wide16_launch_rollout_full_r<false>(actor_desc->layer_N, grid, lf, as_stream(stream), wa, a, wc, c, nA, fuse_ins ? &ins : nullptr);
      if (rcf) return rcf;
      MAPPO_CHECK_LAUNCH("rollout_step");
      return MAPPO_OK;
    }
    const int rcw = actor_desc->use_relu ? wide16_launch_rollout_step_r<true>(actor_desc->layer_N, grid, lb, as_stream(stream), wa, a, wc, c, nA)
                                         : wide16_launch_rollout_step_r<false>(actor_desc->layer_N, grid, lb, as_stream(stream), wa, a, wc, c, nA);
    if (rcw) return rcw;
    MAPPO_CHECK_LAUNCH("rollout_step");
    return MAPPO_OK;
  }
  const int64_t n_tiles = (B + 15) / 16;                 // forward16_body: 16 samples per wave
  const int want = n_tiles >= 4 ? 4 : (n_tiles >= 2 ? 2 : 1);
  int nw = fit_waves(*actor_desc, want);
  const int nwc = fit_waves(*critic_desc, want);
  nw = nw < nwc ? nw : nwc;
  StepArgs s = {};
  s.a.params = actor_params; s.a.x = obs; s.a.avail = avail; s.a.actions = actions; s.a.logp = logp; s.a.desc = *actor_desc; s.a.B = B;
  s.a.deterministic = deterministic; s.a.seed = seed; s.a.counter = counter; s.a.counter_dev = counter_dev;
  s.a.x_sn = obs_stride_n; s.a.x_sm = obs_stride_m; s.a.x_M = M;
  s.a.off = net_offsets(s.a.desc); s.a.map = lds_map(s.a.desc, nw);
  s.c.params = critic_params; s.c.x = share_obs; s.c.out = values; s.c.desc = *critic_desc; s.c.B = B;
  s.c.x_sn = share_stride_n; s.c.x_sm = share_stride_m; s.c.x_M = M;
  s.c.off = net_offsets(s.c.desc); s.c.map = lds_map(s.c.desc, nw);
  const int totA = s.a.map.total, totC = s.c.map.total;
  const size_t lds_bytes = (size_t)(totA > totC ? totA : totC) * sizeof(float);
  MAPPO_REQUIRE(lds_bytes <= LDS_DYN_MAX, "rollout_step: needs %zu B of LDS", lds_bytes);
  int64_t nb = (n_tiles + nw - 1) / nw;
  if (nb > NUM_CU / 2) nb = NUM_CU / 2;
  s.nA = actions ? (int)nb : 0; s.nC = (int)nb; s.nI = 0;
  if (obs_dst) {
    InsertArgs &i = s.ins;
    i.obs = obs; i.obs_sn = obs_stride_n; i.obs_sm = obs_stride_m; i.rew = rewards; i.rew_sn = rew_stride_n; i.rew_sm = rew_stride_m;
    i.done = dones; i.done_sn = done_stride_n; i.done_sm = done_stride_m; i.obs_dst = obs_dst; i.share_dst = share_dst;
    i.rew_dst = rew_dst; i.mask_dst = mask_dst; i.N = (int)(B / M); i.M = M; i.D = actor_desc->in_dim; i.centralized = centralized;
    const int64_t total = B * (centralized ? (int64_t)M * i.D : i.D);
    int64_t ni = (total + 2047) / 2048;                  // ~8 elements per thread
    s.nI = (int)(ni > NUM_CU ? NUM_CU : ni);              // (64 insert workgroups became the long pole of the launch beyond ~2 000 threads)
  }
  dim3 grid((unsigned)(s.nA + s.nC + s.nI)), block(WAVE * nw);
  if (md) {
    if (int rc = dispatch_relu_ln<1>(actor_desc->use_relu != 0, actor_desc->layer_N, [&](auto R, auto L) {
          return launch_kernel<rollout_step_md_kernel<R.value, L.value>, LDS_DYN_MAX, MAPPO_PROF_ACT>("rollout_step_md", grid, block, lds_bytes, as_stream(stream), s, *md);
        }))
      return rc;
    MAPPO_CHECK_LAUNCH("rollout_step_md");
    return MAPPO_OK;
  }
  if (int rc = dispatch_relu_ln(actor_desc->use_relu != 0, actor_desc->layer_N, [&](auto R, auto L) {
        return launch_kernel<rollout_step_kernel<R.value, L.value>, LDS_DYN_MAX, MAPPO_PROF_ACT>("rollout_step", grid, block, lds_bytes, as_stream(stream), s);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH("rollout_step");
  return MAPPO_OK;
}

extern "C" int mappo_rollout_step(const float *actor_params, const mappo_net_desc *actor_desc, const float *critic_params,
                                  const mappo_net_desc *critic_desc, const float *obs, int64_t obs_stride_n, int64_t obs_stride_m,
                                  const float *share_obs, int64_t share_stride_n, int64_t share_stride_m, int32_t M, int64_t B,
                                  const float *avail, int32_t deterministic, uint64_t seed, uint64_t counter,
                                  const uint64_t *counter_dev, float *actions, float *logp, float *values, float *obs_dst,
                                  float *share_dst, const float *rewards, int64_t rew_stride_n, int64_t rew_stride_m,
                                  const uint8_t *dones, int64_t done_stride_n, int64_t done_stride_m, float *rew_dst,
                                  float *mask_dst, int32_t centralized, mappo_stream_t stream) {
  return rollout_step_impl(actor_params, actor_desc, critic_params, critic_desc, obs, obs_stride_n, obs_stride_m, share_obs, share_stride_n,
                           share_stride_m, M, B, avail, deterministic, seed, counter, counter_dev, actions, logp, values, obs_dst, share_dst,
                           rewards, rew_stride_n, rew_stride_m, dones, done_stride_n, done_stride_m, rew_dst, mask_dst, centralized, stream,
                           nullptr);
}

extern "C" int mappo_rollout_step_md(const float *actor_params, const mappo_net_desc *actor_desc, const float *critic_params,
                                     const mappo_net_desc *critic_desc, const float *obs, int64_t obs_stride_n, int64_t obs_stride_m,
                                     const float *share_obs, int64_t share_stride_n, int64_t share_stride_m, int32_t M, int64_t B,
                                     const float *avail, const int32_t *head_dims, int32_t n_heads, int32_t deterministic, uint64_t seed,
                                     uint64_t counter, const uint64_t *counter_dev, float *actions, float *logp, float *values,
                                     float *obs_dst, float *share_dst, const float *rewards, int64_t rew_stride_n, int64_t rew_stride_m,
                                     const uint8_t *dones, int64_t done_stride_n, int64_t done_stride_m, float *rew_dst, float *mask_dst,
                                     int32_t centralized, mappo_stream_t stream) {
  MdHeads md;
  if (int rc = check_md(actor_desc, head_dims, n_heads, avail, "rollout_step_md", md)) return rc;
  if (int rc = check_desc(critic_desc, "rollout_step_md")) return rc;
  MAPPO_REQUIRE(critic_desc->in_dim <= MAXD, "rollout_step_md: critic in_dim %d > %d", critic_desc->in_dim, MAXD);
  return rollout_step_impl(actor_params, actor_desc, critic_params, critic_desc, obs, obs_stride_n, obs_stride_m, share_obs, share_stride_n,
                           share_stride_m, M, B, nullptr, deterministic, seed, counter, counter_dev, actions, logp, values, obs_dst, share_dst,
                           rewards, rew_stride_n, rew_stride_m, dones, done_stride_n, done_stride_m, rew_dst, mask_dst, centralized, stream,
                           &md);
}

// ---- one rollout episode in one launch (rollout_episode_kernel) ---------------------------------------------------------------
// Geometry (measured: DESIGN.md, launch structure).  The kernel holds its weights in registers: one wave per SIMD, so the waves
// of one launch are at most 4 x NUM_CU and the network items are dealt over all of them; the insert follows every wave's items.
// Diagnostic overrides for A/B on one build: MAPPO_EPISODE_WAVES (waves per workgroup: 1 / 2 / 4), MAPPO_EPISODE_NET_WAVES
// (network waves), MAPPO_EPISODE_INS_WAVES (> 0: that many waves of their own for the insert), MAPPO_EPISODE_COST_A (an actor
// item's cost against a critic item's EPISODE_COST_C, which splits the network waves).
#define EPISODE_WAVES 1
#define EPISODE_COST_A 150                                 // per-item costs: the actor samples after its head (measured: DESIGN.md)
#define EPISODE_COST_C 134
static int env_int(const char *name, int dflt, int lo, int hi) {
  const char *ev = getenv(name);
  if (!ev) return dflt;
  const int v = atoi(ev);
  return v < lo ? lo : (v > hi ? hi : v);
}

// The LDS body (mlp_ep16l.h), layer_N 0 / 1: one workgroup of EPISODE_LDS_WAVES waves per CU, each serving one network from an LDS
// image of its weights; the workgroups are split between actor and critic by item cost per SIMD.  It is the default where the
// register body above would run, unless one of that body's geometry overrides is set (they keep their meaning and their kernel);
// MAPPO_EPISODE_LDS=0 / 1 forces the choice.  Overrides of its own: MAPPO_EPISODE_LDS_WAVES (waves per workgroup, 1 .. 16) and
// MAPPO_EPISODE_LDS_ACTOR_WGS (the actor's workgroups, 1 .. workgroups - 1; 0: by cost).  Measured: DESIGN.md, round 8.
#define EPISODE_LDS_DEFAULT 1
#define EPISODE_LDS_WAVES 16
#define EPISODE_LDS_COST_A 150                             // per-item costs, as for the register body (134 of 256 workgroups for the actor at the
#define EPISODE_LDS_COST_C 134                             // bench shape; the sweep in DESIGN.md, round 8: 120 .. 130 are ~1 us shorter, 2 % of the launch)
// which body a launch with this layer_N takes under the current environment (1: LDS, 0: registers)
extern "C" int mappo_rollout_episode_uses_lds(int32_t layer_N) {
  if (layer_N < 0 || layer_N > 1) return 0;
  if (const char *ev = getenv("MAPPO_EPISODE_LDS")) return atoi(ev) != 0;
  if (getenv("MAPPO_EPISODE_WAVES") || getenv("MAPPO_EPISODE_NET_WAVES") || getenv("MAPPO_EPISODE_INS_WAVES") || getenv("MAPPO_EPISODE_COST_A")) return 0;
  return EPISODE_LDS_DEFAULT;
}

extern "C" int mappo_rollout_episode(const float *actor_params, const mappo_net_desc *actor_desc, const float *critic_params,
                                     const mappo_net_desc *critic_desc, int32_t T, int32_t N, int32_t M, const float *env_obs,
                                     int64_t obs_stride_t, int64_t obs_stride_n, int64_t obs_stride_m, const float *rewards,
                                     int64_t rew_stride_t, int64_t rew_stride_n, int64_t rew_stride_m, const uint8_t *dones,
                                     int64_t done_stride_t, int64_t done_stride_n, int64_t done_stride_m, int32_t deterministic,
                                     uint64_t seed, uint64_t counter, const uint64_t *counter_dev, float *obs_buf, float *share_buf,
                                     float *rew_buf, float *mask_buf, float *actions, float *logp, float *values, float *next_values,
                                     int32_t centralized, mappo_stream_t stream) {
  if (int rc = check_desc(actor_desc, "rollout_episode")) return rc;
  if (int rc = check_desc(critic_desc, "rollout_episode")) return rc;
  MAPPO_REQUIRE(actor_desc->in_dim <= MAXD && critic_desc->in_dim <= MAXD, "rollout_episode: in_dim %d / %d: both networks must be narrow (<= %d)",
                actor_desc->in_dim, critic_desc->in_dim, MAXD);
  MAPPO_REQUIRE(actor_desc->layer_N == critic_desc->layer_N && actor_desc->use_relu == critic_desc->use_relu,
                "rollout_episode: actor and critic must share layer_N and the activation");
  MAPPO_REQUIRE(critic_desc->out_dim == 1, "rollout_episode: critic out_dim must be 1");
  MAPPO_REQUIRE(T >= 1 && N >= 1 && M >= 1, "rollout_episode: bad shape T=%d N=%d M=%d", T, N, M);
  MAPPO_REQUIRE(obs_stride_t >= 0 && obs_stride_n >= 0 && obs_stride_m >= 0 && rew_stride_t >= 0 && rew_stride_n >= 0 && rew_stride_m >= 0 &&
                done_stride_t >= 0 && done_stride_n >= 0 && done_stride_m >= 0, "rollout_episode: negative stride");
  const int D = actor_desc->in_dim;
  if (centralized)      // share row of (n, m) = the thread's agents side by side, read in place: the agents must be contiguous
    MAPPO_REQUIRE(critic_desc->in_dim == M * D && obs_stride_m == D, "rollout_episode: centralized critic needs in_dim M*D = %d (got %d) and "
                  "agent rows D apart in the env output (stride %lld)", M * D, critic_desc->in_dim, (long long)obs_stride_m);
  else
    MAPPO_REQUIRE(critic_desc->in_dim == D, "rollout_episode: critic in_dim %d != actor in_dim %d", critic_desc->in_dim, D);
  MAPPO_REQUIRE(actor_params && critic_params && env_obs && rewards && dones && obs_buf && share_buf && rew_buf && mask_buf && actions && logp &&
                values && next_values, "rollout_episode: bad arguments (null pointer)");
  MAPPO_CLEAR_STICKY();
  const int64_t B = (int64_t)N * M, S = critic_desc->in_dim;
  const int64_t n_tiles = (B + 15) / 16;
  const bool use_lds = mappo_rollout_episode_uses_lds(actor_desc->layer_N) != 0;
  int nw = env_int("MAPPO_EPISODE_WAVES", EPISODE_WAVES, 1, 4);
  if (nw != 1 && nw != 2) nw = 4;
  const int n_ins = env_int("MAPPO_EPISODE_INS_WAVES", 0, 0, 4 * NUM_CU - 2);
  const int n_net = env_int("MAPPO_EPISODE_NET_WAVES", 4 * NUM_CU - n_ins, 2, 4 * NUM_CU);
  const int64_t cost_a = env_int("MAPPO_EPISODE_COST_A", EPISODE_COST_A, 1, 1000), cost_c = EPISODE_COST_C;
  // the split of the network waves with the shortest longest wave (items per wave x item cost); no network gets more waves than items
  const int64_t items_a = (int64_t)T * n_tiles, items_c = (int64_t)(T + 1) * n_tiles;
  int64_t wa = 1, best = -1;
  for (int64_t a = 1; a < n_net; ++a) {
    const int64_t la = (items_a + a - 1) / a * cost_a, lc = (items_c + (n_net - a) - 1) / (n_net - a) * cost_c;
    const int64_t l = la > lc ? la : lc;
    if (best < 0 || l < best) { best = l; wa = a; }
  }
  const int64_t wc = n_net - wa > items_c ? items_c : n_net - wa;
  if (wa > items_a) wa = items_a;
  EpisodeArgs e = {};
  e.a.params = actor_params; e.a.actions = actions; e.a.logp = logp; e.a.desc = *actor_desc; e.a.B = B; e.a.deterministic = deterministic;
  e.a.seed = seed; e.a.counter = counter; e.a.counter_dev = counter_dev; e.a.off = net_offsets(e.a.desc);
  e.c.params = critic_params; e.c.out = values; e.c.desc = *critic_desc; e.c.B = B; e.c.off = net_offsets(e.c.desc);
  e.sa = EpisodeSrc{obs_buf, (int64_t)M * D, D, env_obs, obs_stride_t, obs_stride_n, obs_stride_m};
  e.sc = EpisodeSrc{share_buf, (int64_t)M * S, S, env_obs, obs_stride_t, obs_stride_n, centralized ? 0 : obs_stride_m};
  e.next_values = next_values;
  InsertArgs &i = e.ins;
  i.obs = env_obs; i.obs_sn = obs_stride_n; i.obs_sm = obs_stride_m; i.rew = rewards; i.rew_sn = rew_stride_n; i.rew_sm = rew_stride_m;
  i.done = dones; i.done_sn = done_stride_n; i.done_sm = done_stride_m;
  i.obs_dst = obs_buf + B * D; i.share_dst = share_buf + B * S; i.rew_dst = rew_buf; i.mask_dst = mask_buf + B;    // slots 1, 1, 0, 1
  i.N = N; i.M = M; i.D = D; i.centralized = centralized;
  e.ins_obs_st = obs_stride_t; e.ins_rew_st = rew_stride_t; e.ins_done_st = done_stride_t;
  e.T = T; e.M = M; e.wA = (int)wa; e.wC = (int)wc;
  e.wI0 = n_ins > 0 ? e.wA + e.wC : 0;
  e.wAll = e.wA + e.wC + n_ins;
  const bool relu = actor_desc->use_relu != 0;
  if (use_lds) {
    const int W = env_int("MAPPO_EPISODE_LDS_WAVES", EPISODE_LDS_WAVES, 1, EPL_MAX_WAVES);
    // no more workgroups than have an item for every wave (at least one per network), at most one per CU
    int64_t G = (items_a + W - 1) / W + (items_c + W - 1) / W;
    G = G > NUM_CU ? NUM_CU : G;
    // the actor's share: the shortest longest SIMD (a workgroup's waves sit on min(W, 4) SIMDs; items per SIMD x item cost)
    const int simds = W < 4 ? W : 4;
    int64_t ga = 1, lbest = -1;
    for (int64_t a = 1; a < G; ++a) {
      const int64_t la = (items_a + a * simds - 1) / (a * simds) * EPISODE_LDS_COST_A, lc = (items_c + (G - a) * simds - 1) / ((G - a) * simds) * EPISODE_LDS_COST_C;
      const int64_t l = la > lc ? la : lc;
      if (lbest < 0 || l < lbest) { lbest = l; ga = a; }
    }
    ga = env_int("MAPPO_EPISODE_LDS_ACTOR_WGS", 0, 0, (int)G - 1) > 0 ? env_int("MAPPO_EPISODE_LDS_ACTOR_WGS", 0, 0, (int)G - 1) : ga;
    e.wA = (int)ga; e.wC = (int)(G - ga); e.wI0 = 0; e.wAll = (int)G * W;
    const dim3 lgrid((unsigned)G), lblock(WAVE * W);
    const int img = actor_desc->layer_N == 0 ? EplMap<0>::total : EplMap<1>::total;
    const size_t lbytes = sizeof(float) * (img + W * 16 * TP);      // the network image + a [16][TP] logits tile per wave
    // layer_N 0 / 1 only (mappo_rollout_episode_uses_lds)
    if (int rc = dispatch_relu_ln<1>(relu, actor_desc->layer_N, [&](auto R, auto L) {
          constexpr int lds_max = (int)(sizeof(float) * (EplMap<L.value>::total + EPL_MAX_WAVES * 16 * TP));
          return launch_kernel<rollout_episode_lds_kernel<R.value, L.value>, lds_max>("rollout_episode", lgrid, lblock, lbytes, as_stream(stream), e);
        }))
      return rc;
    MAPPO_CHECK_LAUNCH("rollout_episode");
    return MAPPO_OK;
  }
  const dim3 grid((unsigned)((e.wAll + nw - 1) / nw)), block(WAVE * nw);
  const size_t lds_bytes = sizeof(float) * 16 * TP * nw;   // the actor's [16][TP] logits tile per wave
  dispatch_relu_ln(relu, actor_desc->layer_N, [&](auto R, auto L) {       // (the logits tiles fit the default dynamic-LDS limit)
    hipLaunchKernelGGL((rollout_episode_kernel<R.value, L.value>), grid, block, lds_bytes, as_stream(stream), e);
    return MAPPO_OK;
  });
  MAPPO_CHECK_LAUNCH("rollout_episode");
  return MAPPO_OK;
}
