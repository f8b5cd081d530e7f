// wide-input kernels (mlp_wide16.h): the split-K forward for step-sized batches, its dual form, and the one-launch recurrent
// step built on it (mlp_wide_rec16.h)
#include "mlp_fwd.h"
#include "mlp_upd16.h"
#include "mlp_wide16.h"
#include "mlp_wide_rec16.h"
#include "mlp_launch.h"

template <bool R, int L>
static int wide16_forward_sk_mode(int mode, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &w, const FwdArgs &a, const char *who) {
  const dim3 block(256);
  if (mode == 0) return launch_kernel<wide_forward16_sk_kernel<R, L, 0>, WIDE_LDS_STREAM, MAPPO_PROF_MLP_FWD>(who, grid, block, lds_bytes, st, w, a);
  if (mode == 1) return launch_kernel<wide_forward16_sk_kernel<R, L, 1>, WIDE_LDS_STREAM, MAPPO_PROF_ACT>(who, grid, block, lds_bytes, st, w, a);
  return launch_kernel<wide_forward16_sk_kernel<R, L, 2>, WIDE_LDS_STREAM, MAPPO_PROF_MLP_FWD>(who, grid, block, lds_bytes, st, w, a);
}
int wide16_launch_forward_sk(int mode, bool relu, int ln, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &w, const FwdArgs &a,
                             const char *who) {
  return dispatch_relu_ln(relu, ln, [&](auto R, auto L) { return wide16_forward_sk_mode<R.value, L.value>(mode, grid, lds_bytes, st, w, a, who); });
}
int wide16_launch_features_sk_dual(bool relu, int ln, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &wa, const FwdArgs &a,
                                   const Wide16Args &wc, const FwdArgs &c, int nA) {
  WideDualArgs d;
  d.wa = wa; d.wc = wc; d.a = a; d.c = c; d.nA = nA;
  return dispatch_relu_ln(relu, ln, [&](auto R, auto L) {
    return launch_kernel<wide_features16_sk_dual_kernel<R.value, L.value>, WIDE_LDS_STREAM, MAPPO_PROF_MLP_FWD>("mlp_features_dual", grid, dim3(256), lds_bytes, st, d);
  });
}
int wide16_launch_recurrent_step_dual(bool relu, int ln, size_t lds_bytes, hipStream_t st, const Wide16Args &wa, const FwdArgs &a,
                                      const Wide16Args &wc, const FwdArgs &c, int nt16, const WideStepIO &io) {
  WideRecDualArgs r = {};
  r.d.wa = wa; r.d.wc = wc; r.d.a = a; r.d.c = c; r.d.nA = nt16;
  GruFwdArgs &ga = r.ga, &gc = r.gc;
  ga.params = a.params; ga.off = a.off; ga.desc = a.desc; ga.h0 = io.actor_h0; ga.masks = io.masks; ga.L = 1; ga.Nc = io.Nc; ga.A = a.desc.out_dim;
  ga.head_mode = 2; ga.h_last = io.actor_h_last; ga.avail = io.avail; ga.actions = io.actions; ga.logp = io.logp;
  ga.deterministic = io.deterministic; ga.seed = io.seed; ga.counter = io.counter; ga.counter_dev = io.counter_dev;
  gc.params = c.params; gc.off = c.off; gc.desc = c.desc; gc.h0 = io.critic_h0; gc.masks = io.masks; gc.L = 1; gc.Nc = io.Nc; gc.A = 1;
  gc.head_mode = 1; gc.h_last = io.critic_h_last; gc.out = io.values;
  r.nI = 0;
  if (io.ins) {
    r.ins = *io.ins;
    ga.dones = gc.dones = io.ins->done; ga.done_M = gc.done_M = io.ins->M; ga.done_sn = gc.done_sn = io.ins->done_sn; ga.done_sm = gc.done_sm = io.ins->done_sm;
    const int64_t most = (int64_t)io.Nc * (io.ins->D > io.ins->S ? io.ins->D : io.ins->S);
    const int64_t ni = (most + 2047) / 2048;                     // ~8 elements per thread
    r.nI = (int)(ni < 1 ? 1 : (ni > 64 ? 64 : ni));
  }
  const dim3 grid((unsigned)(2 * nt16 + r.nI));
  return dispatch_relu_ln(relu, ln, [&](auto R, auto L) {
    return launch_kernel<wide_recurrent_step_dual_kernel<R.value, L.value>, WIDE_LDS_STREAM, MAPPO_PROF_ACT>("recurrent_step_dual", grid, dim3(256), lds_bytes, st, r);
  });
}
