// mlp_wide_rec16.h — wide_recurrent_step_dual_kernel: the split-K wide trunk (mlp_wide16.h) followed by the GRU step and the heads
// (gru_step3.h) of a recurrent actor and critic in one launch.  Compiled by mlp_wide_sk.hip alone.  Needs mlp_wide16.h.
#pragma once
#include "mlp_wide16.h"
// ---- one rollout step of a recurrent actor AND critic with wide inputs in ONE launch (r_actor_critic.py:43-70,146-165;
// smac_runner.py:110-127) ----
// Round 2 ran such a step as two launches (mappo_mlp_features_dual: split-K trunks -> featT in HBM; mappo_gru_step_dual: GRU cell +
// rnn.norm + heads), 21 + 14 us at BASELINE configs[3] where the arithmetic is a few microseconds: two launch latencies, two
// weight-fetch latencies and a feature round trip through HBM.  Here the 4-wave workgroup that runs a tile's split-K trunk goes
// straight on to the tile's GRU step: the GRU / head operands of every wave are requested BEFORE the trunk starts (they land
// under it), wave 0's trunk output crosses to the other waves through 4 KB of LDS, and gru_step3_tiles finishes the row.
#include "gru_step3.h"
struct WideRecDualArgs {
  WideDualArgs d;
  GruFwdArgs ga, gc;
  SmacInsert ins;             // nI > 0: workgroups [2 nA, 2 nA + nI) perform the SMAC insert of the env output the rows are read from
  int nI;
};
template <bool RELU, int LN>
__global__ __launch_bounds__(256, 1) void wide_recurrent_step_dual_kernel(WideRecDualArgs r) {
  extern __shared__ __align__(16) float lds[];
  __shared__ SkShared sh;
  __shared__ Step3Shared s3;
  __shared__ float4 sX[4 * 64];
  const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool actor = (int)blockIdx.x < r.d.nA;                    // one tile per workgroup: grid = 2 x tiles (+ insert workgroups)
  const int bid = actor ? (int)blockIdx.x : (int)blockIdx.x - r.d.nA, nb = r.d.nA;
  if ((int)blockIdx.x >= 2 * r.d.nA) { insert_smac_body(r.ins, (int)blockIdx.x - 2 * r.d.nA, r.nI); return; }
  Step3W<0> W;
  // (the GRU step's 96 weight registers are requested BEHIND the trunk's own weights and rows: asked for first, they were what the
  // trunk's first MFMA waited for)
  if (actor) {
    wide_forward16_sk_body<RELU, LN, 4>(r.d.wa, r.d.a, lds, sh, bid, nb, reinterpret_cast<float *>(sX),
                                        [&]() __attribute__((always_inline)) { gru_step3_load<Step3Src::Lds, 0>(W, r.ga, wv, n, q); });
    gru_step3_tiles<2, Step3Src::Lds, false, 0>(W, r.ga, s3, bid, nb, sX);
  } else {
    wide_forward16_sk_body<RELU, LN, 4>(r.d.wc, r.d.c, lds, sh, bid, nb, reinterpret_cast<float *>(sX),
                                        [&]() __attribute__((always_inline)) { gru_step3_load<Step3Src::Lds, 0>(W, r.gc, wv, n, q); });
    gru_step3_tiles<1, Step3Src::Lds, false, 0>(W, r.gc, s3, bid, nb, sX);
  }
}
#undef GS
#undef NG
