// mlp_upd_args.h — the argument block every update kernel family takes (mlp_upd.h, mlp_upd2.h, mlp_upd16.h) and the prefetch of
// the in-kernel loss heads' per-sample inputs.  Needs mlp_blocks.h (LdsMap, NetOff).
#pragma once
#include "mlp_blocks.h"

// ------------------------------------------------------------------------------------------------
// update kernel: forward + head gradient (external | PPO actor loss | value loss) + backward
// ------------------------------------------------------------------------------------------------
struct UpdArgs {
  const float *params, *x;
  const int32_t *rows;
  float *slabs;
  int64_t slab_stride, slab_col0;
  mappo_net_desc desc;
  NetOff off;
  LdsMap map;
  int64_t B;
  int n_blocks;              // grid size = slab rows written (0: one workgroup per CU, capped by the tile count)
  int n_regions;             // LDS regions of P floats used for the end-of-kernel reduction (2 when they fit)
  int p_red;                 // end of the flat parameter range this launch reduces (trunk only for HEAD 3)
  int red_base;              // start of that range (b1 for wide inputs: W1 / feature-norm grads come from wide_l1_bwd_kernel)
  float *wide_ws;            // wide inputs: [64][B] dz1 (feature-major) | mean0[B] | rstd0[B]
  const float *dHT;          // HEAD 3: gradient w.r.t. the trunk output, feature-major [64][B]
  int seq_nc;                // HEAD 3 (wide inputs: seq_nc a multiple of 16, so the tiles of the flat order ARE the sequence tiles): > 0 = the B rows are a time-major [L][seq_nc] minibatch tiled per (t, 16 sequences) and dHT is BLOCKED per tile (gru_train16.hip)
  // HEAD 0
  const float *dout;
  // HEAD 1 / 2 (buffer-order arrays, indexed by rows)
  const float *avail, *actions, *old_logp, *adv, *active, *v_old, *returns, *vn_state;
  const double *mb_moments;
  double *partials;          // [gridDim.x][4]
  mappo_ppo_cfg cfg;
  unsigned long long *stamps;   // diagnostic build (-DMLP_STAMPS) only
  unsigned long long *stamps_waves;   // the same, one row per wave (update16_body)
};

// per-sample inputs of the in-kernel loss heads, prefetched one tile ahead (lanes 0..31 hold one sample each)
struct LossPrefetch {
  float f0, f1, f2, f3;     // actor: action, old_logp, adv, active   | critic: v_old, ret, active, -
  uint32_t dead;            // actor: bit a set <=> available_actions[a] == 0
};

template <int HEAD>
__device__ __forceinline__ void prefetch_loss(LossPrefetch &lp, const UpdArgs &p, int64_t row, int n_valid, int lane, int A) {
  lp.f0 = lp.f1 = lp.f2 = lp.f3 = 0.f;
  lp.dead = 0u;
  if (HEAD == 0 || HEAD == 3 || lane >= n_valid) return;        // lanes 0..31 carry the per-sample loss inputs
  if (HEAD == 1) {
    lp.f0 = p.actions[row]; lp.f1 = p.old_logp[row]; lp.f2 = p.adv[row]; lp.f3 = p.active[row];
    if (p.avail) {
      const float *av = p.avail + row * A;
      for (int a = 0; a < A; ++a) lp.dead |= (av[a] == 0.f ? 1u : 0u) << a;
    }
  } else {
    lp.f0 = p.v_old[row]; lp.f1 = p.returns[row]; lp.f2 = p.active[row];
  }
}
