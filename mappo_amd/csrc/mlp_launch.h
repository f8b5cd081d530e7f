// mlp_launch.h — what the MLP translation units share on the host side: the LDS / chip limits, the one kernel launcher
// (launch_kernel), the (use_relu, layer_N) -> template-argument dispatcher (dispatch_relu_ln) and the declarations of the
// launchers that are defined in another translation unit.  Needs common.h only: the argument blocks are named, not used.
#pragma once
#include "common.h"
#include <type_traits>

struct FwdArgs;
struct UpdArgs;
struct DualArgs;
struct Upd16Args;
struct Dual16Args;
struct Group16Args;
struct MdHeads;
struct Wide16Args;
struct WideBwd16Args;
struct InsertArgs;
struct SmacInsert;

#define LDS_LIMIT (160 * 1024)
#define LDS_STATIC 1024                      // static __shared__ of the kernels (reduction scratch), rounded up
#define LDS_DYN_MAX (LDS_LIMIT - LDS_STATIC) // what hipFuncAttributeMaxDynamicSharedMemorySize may be raised to
#define NUM_CU 256
#define UPD16_LDS_MAX (LDS_LIMIT - 256)          // the 16-sample-tile update kernels have no static __shared__
#define WIDE_LDS_STREAM (96 * 1024)           // dynamic LDS limit of the streamed / split-K wide kernels (mlp_wide16.h)
#define WIDE_LDS_WHOLE (159 * 1024)           // ... of the wide kernels that stage W1' whole
#define WIDE_SK_MAX_TILES 256          // per network: above, the streamed kernels fill the chip

// Launch Kernel with up to LDS_MAX bytes of dynamic LDS: the limit is raised once per kernel (the static is per instantiation),
// a failure to raise it is reported through mappo_set_error under the caller's name.  PROF: the profiling hook (MAPPO_PROF_*) the
// launch is bracketed by when armed, or -1 for a plain launch.
template <auto Kernel, int LDS_MAX, int PROF = -1, typename... Args>
static int launch_kernel(const char *who, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Args &...args) {
  static const hipError_t e_ = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
  if (e_ != hipSuccess) { mappo_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(e_)); (void)hipGetLastError(); return MAPPO_ELAUNCH; }
  if constexpr (PROF >= 0) PROF_LAUNCH(PROF, Kernel, grid, block, lds_bytes, st, args...);
  else hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, st, args...);
  return MAPPO_OK;
}

// f(R, L) with R = std::bool_constant<relu>, L = std::integral_constant<int, layer_N>: inside a generic lambda R.value and
// L.value are template arguments.  layer_N above MAX_LN takes MAX_LN (the callers have checked the range).
template <int MAX_LN = 2, typename F>
static int dispatch_relu_ln(bool relu, int ln, F &&f) {
  using T = std::true_type; using N = std::false_type;
  if (ln <= 0) return relu ? f(T{}, std::integral_constant<int, 0>{}) : f(N{}, std::integral_constant<int, 0>{});
  if (ln == 1 || MAX_LN == 1) return relu ? f(T{}, std::integral_constant<int, 1>{}) : f(N{}, std::integral_constant<int, 1>{});
  return relu ? f(T{}, std::integral_constant<int, MAX_LN>{}) : f(N{}, std::integral_constant<int, MAX_LN>{});
}

// ---- update kernel families: one translation unit per (RELU, LN) pair, compiled in parallel ----
// K-chunked wide kernel (mlp_upd.h), in_dim 65..512: translation units mlp_upd_r{0,1}_l{0,1,2}.hip
template <bool R, int L, int HEAD>
int upd_inst(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const UpdArgs &a, const char *who);
// pair kernel (mlp_upd2.h), in_dim <= 64: translation units mlp_upd2_r{0,1}_l{0,1,2}.hip
template <bool R, int L, int HEAD>
int upd2_inst(bool wide, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const UpdArgs &a, const char *who);
// actor + critic in one launch (mlp_update2_dual_kernel): translation units mlp_upd2d_r{0,1}_l{0,1,2}.hip
template <bool R, int L>
int upd2d_inst(bool wide_a, bool wide_c, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const DualArgs &d);
// one wave per 16-sample tile (mlp_upd16.h), in_dim <= 64, layer_N <= 1: translation units mlp_upd16_r{0,1}_l{0,1}.hip
template <bool R, int L>
int upd16_inst(int head, bool wide, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Upd16Args &a);
template <bool R, int L>
int upd16d_inst(bool wide_a, bool wide_c, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Dual16Args &d);
// the MultiDiscrete actor on the same kernels (multi-head loss): translation units mlp_upd16md_r{0,1}_l{0,1}.hip
template <bool R, int L>
int upd16md_inst(bool wide, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Upd16Args &a, const MdHeads &md);
template <bool R, int L>
int upd16mdd_inst(bool wide_a, bool wide_c, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Dual16Args &d, const MdHeads &md);
// up to MAPPO_MAX_GROUP dual launches in one (mlp_update16_group_kernel): translation units mlp_upd16g_r{0,1}_l{0,1}.hip
template <bool R, int L>
int upd16g_inst(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Group16Args &g);
// the same network from the layer-1 pre-activations on (in_dim 65..512; layer 1 in mlp_wide16.h / wide_l1_bwd_kernel)
template <bool R, int L>
int upd16x_inst(int head, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Upd16Args &a);

// ---- launchers of the wide-input kernels (mlp_wide16.h), defined in mlp_wide.hip, mlp_wide_fwd_r{0,1}.hip (the *_r forms) and mlp_wide_sk.hip ----
int wide16_launch_l1_fwd(const Wide16Args &w, dim3 grid, hipStream_t st);
int wide16_launch_forward(int mode, bool relu, int ln, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st,
                          const Wide16Args &w, const FwdArgs &a, const char *who);
int wide16_launch_l1_bwd(const WideBwd16Args &w, dim3 grid, hipStream_t st);
int wide16_launch_features_dual(bool relu, int ln, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Wide16Args &wa,
                                const FwdArgs &a, const Wide16Args &wc, const FwdArgs &c, int nA);
template <bool R>
int wide16_launch_forward_r(int mode, int ln, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Wide16Args &w, const FwdArgs &a,
                            const char *who);
template <bool R>
int wide16_launch_features_dual_r(int ln, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const Wide16Args &wa, const FwdArgs &a,
                                  const Wide16Args &wc, const FwdArgs &c, int nA);
template <bool R>
int wide16_launch_rollout_step_r(int ln, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &wa, const FwdArgs &a,
                                 const Wide16Args &wc, const FwdArgs &c, int nA);
template <bool R>
int wide16_launch_features_resident_r(int ln, dim3 grid, hipStream_t st, const Wide16Args &w, const FwdArgs &a);
template <bool R>
int wide16_launch_rollout_full_r(int ln, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &wa, const FwdArgs &a,
                                 const Wide16Args &wc, const FwdArgs &c, int nA, const InsertArgs *ins);
// split-K variants (one tile per 4-wave workgroup): step-sized batches
int wide16_launch_forward_sk(int mode, bool relu, int ln, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &w, const FwdArgs &a,
                             const char *who);
int wide16_launch_features_sk_dual(bool relu, int ln, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &wa, const FwdArgs &a,
                                   const Wide16Args &wc, const FwdArgs &c, int nA);
// trunks + GRU step + heads of both networks in one launch (wide_recurrent_step_dual_kernel); one tile per workgroup
struct WideStepIO {
  const SmacInsert *ins;        // or NULL: no fused insert (then `masks` is read; with it the row mask comes from ins->done)
  const float *actor_h0, *critic_h0, *masks, *avail;
  float *actor_h_last, *critic_h_last, *actions, *logp, *values;
  int Nc, deterministic;
  uint64_t seed, counter;
  const uint64_t *counter_dev;
};
int wide16_launch_recurrent_step_dual(bool relu, int ln, size_t lds_bytes, hipStream_t st, const Wide16Args &wa, const FwdArgs &a,
                                      const Wide16Args &wc, const FwdArgs &c, int nt16, const WideStepIO &io);

// ---- inputs beyond the tuned wide kernels' 512 columns (mlp_wide_sliced.h), defined in mlp_wide_sliced.hip / mlp_wide_sliced_r{0,1}.hip ----
#define WIDE_TUNED_MAX_D 512           // widest input of the kernels in mlp_wide16.h; above it (up to MAPPO_MAX_IN_DIM) the sliced kernels
int wide_sliced_launch_l1_fwd(const Wide16Args &w, dim3 grid, hipStream_t st);
int wide_sliced_launch_l1_bwd(const WideBwd16Args &w, dim3 grid, hipStream_t st);      // grid: (slab rows, 512-column slices)
template <bool R>
int wide_sliced_launch_forward_r(int mode, int ln, dim3 grid, size_t lds_bytes, hipStream_t st, const Wide16Args &w, const FwdArgs &a,
                                 const char *who);
// the whole forward of one network (a.x_M / x_sn / x_sm: strided rows); mode 0: head output, 1: get_actions, 2: trunk features [64][B]
int wide_sliced_forward(int mode, const FwdArgs &a, hipStream_t st, const char *who);

int launch_features16(const FwdArgs &a_in, hipStream_t st);      // mlp_step.hip
