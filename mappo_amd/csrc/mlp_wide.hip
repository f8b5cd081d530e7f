// wide-input kernels (in_dim 65..512, mlp_wide16.h): layer-1 forward with LDS-resident weights, layer-1 weight gradient
// (the rollout forwards are compiled in mlp_wide_fwd_r{0,1}.hip / mlp_wide_sk.hip: one translation unit took ten minutes)
#include "mlp_fwd.h"
#include "mlp_upd16.h"
#include "mlp_wide16.h"
#include "mlp_launch.h"

int wide16_launch_l1_fwd(const Wide16Args &w, dim3 grid, hipStream_t st) {
  const int nch = (w.D + 63) / 64;                                                    // exact: the row-end chunk is static in the kernel
  const size_t lds_bytes = sizeof(float) * ((size_t)HID * 64 * nch + HID);            // W1' whole (fragment order) + folded bias
  const dim3 block(512);
  switch (nch) {
    case 2: return launch_kernel<wide_l1_fwd16_kernel<2>, WIDE_LDS_WHOLE, MAPPO_PROF_WIDE_L1>("wide_l1_fwd", grid, block, lds_bytes, st, w);
    case 3: return launch_kernel<wide_l1_fwd16_kernel<3>, WIDE_LDS_WHOLE, MAPPO_PROF_WIDE_L1>("wide_l1_fwd", grid, block, lds_bytes, st, w);
    case 4: return launch_kernel<wide_l1_fwd16_kernel<4>, WIDE_LDS_WHOLE, MAPPO_PROF_WIDE_L1>("wide_l1_fwd", grid, block, lds_bytes, st, w);
    case 5: return launch_kernel<wide_l1_fwd16_kernel<5>, WIDE_LDS_WHOLE, MAPPO_PROF_WIDE_L1>("wide_l1_fwd", grid, block, lds_bytes, st, w);
    case 6: return launch_kernel<wide_l1_fwd16_kernel<6>, WIDE_LDS_WHOLE, MAPPO_PROF_WIDE_L1>("wide_l1_fwd", grid, block, lds_bytes, st, w);
    case 7: return launch_kernel<wide_l1_fwd16_kernel<7>, WIDE_LDS_WHOLE, MAPPO_PROF_WIDE_L1>("wide_l1_fwd", grid, block, lds_bytes, st, w);
    default: return launch_kernel<wide_l1_fwd16_kernel<8>, WIDE_LDS_WHOLE, MAPPO_PROF_WIDE_L1>("wide_l1_fwd", grid, block, lds_bytes, st, w);
  }
}

int wide16_launch_forward(int mode, bool relu, int ln, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Wide16Args &w,
                          const FwdArgs &a, const char *who) {
  return relu ? wide16_launch_forward_r<true>(mode, ln, grid, block, lds_bytes, st, w, a, who)
              : wide16_launch_forward_r<false>(mode, ln, grid, block, lds_bytes, st, w, a, who);
}
int wide16_launch_features_dual(bool relu, int ln, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Wide16Args &wa,
                                const FwdArgs &a, const Wide16Args &wc, const FwdArgs &c, int nA) {
  return relu ? wide16_launch_features_dual_r<true>(ln, grid, block, lds_bytes, st, wa, a, wc, c, nA)
              : wide16_launch_features_dual_r<false>(ln, grid, block, lds_bytes, st, wa, a, wc, c, nA);
}

template <bool FN, bool GATHER>
static void wide16_l1_bwd_one(const WideBwd16Args &w, dim3 grid, hipStream_t st) {
  if ((w.D & 63) == 0) PROF_LAUNCH(MAPPO_PROF_WIDE_L1, (wide_l1_bwd16_kernel<FN, GATHER, true>), grid, dim3(512), 0, st, w);      // whole chunks: branch-free tile loop
  else PROF_LAUNCH(MAPPO_PROF_WIDE_L1, (wide_l1_bwd16_kernel<FN, GATHER, false>), grid, dim3(512), 0, st, w);
}
int wide16_launch_l1_bwd(const WideBwd16Args &w, dim3 grid, hipStream_t st) {
  const bool fn = w.fn_w >= 0;
  if (w.rows) { if (fn) wide16_l1_bwd_one<true, true>(w, grid, st); else wide16_l1_bwd_one<false, true>(w, grid, st); }
  else { if (fn) wide16_l1_bwd_one<true, false>(w, grid, st); else wide16_l1_bwd_one<false, false>(w, grid, st); }
  return MAPPO_OK;
}
