// train_glue.hip — the once-per-train() work around the PPO epochs of a whole-buffer update, in two launches instead of
// eight (stats.hip, update_stats in mlp.hip, copy_batch in insert.hip are the separate forms; stats_core.h / insert_core.h hold
// the arithmetic both forms run, so every result is bit-identical to the separate launches):
//
//   mappo_train_prologue = adv_moments + final_reduce<3> + minibatch_moments + final_reduce<3> + valuenorm_update_n + a fill
//   mappo_train_epilogue = update_stats + copy_batch
//
// The prologue's one-workgroup jobs (the two final reductions, the ValueNorm recurrence, the fill) depend only on the
// per-workgroup partials, so the workgroup that finishes LAST does them: every workgroup takes a ticket once its partials are
// published, nobody waits.  mappo_adv_normalize stays a launch of its own: every element needs the final moments, i.e. a
// grid-wide wait, and no launch of this library spins on another workgroup.
#include "stats_core.h"
#include "insert_core.h"

struct PrologueArgs {
  const float *returns, *value_preds, *active;
  float *vn_state;            // [3] in/out or nullptr: read by every workgroup first, written by the last one
  float *adv;
  double *partials;           // [2][STAT_MAX_BLOCKS][3]: advantage partials, then minibatch partials
  int *ticket;
  double *adv_moments, *mb_moments;
  float w, omw;
  int n_epochs;
  float *states_out;
  double *zero;
  int64_t n_zero, n;
};

__global__ __launch_bounds__(STAT_BLOCK) void train_prologue_kernel(PrologueArgs p) {
  __shared__ double smem[16 * 3];
  __shared__ int s_last;
  const VnStats vn = vn_stats(p.vn_state);
  double va[3] = {0.0, 0.0, 0.0}, vm[3] = {0.0, 0.0, 0.0};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += stride) {
    const float r = p.returns[i], act = p.active[i];
    adv_moments_term(r, p.value_preds[i], act, vn, p.adv + i, va);
    minibatch_moments_term(r, act, vm);
  }
  block_sum<3>(va, smem);
  block_sum<3>(vm, smem);
  double *pa = p.partials, *pm = p.partials + (size_t)STAT_MAX_BLOCKS * 3;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      pa[(size_t)blockIdx.x * 3 + i] = va[i];
      pm[(size_t)blockIdx.x * 3 + i] = vm[i];
    }
  }
  // publish the partials, then take a ticket.  The L2 of each XCD is private: the stores are drained, ONE lane makes them
  // visible at agent scope (release) before its relaxed add, and the workgroup that draws the last ticket acquires at agent
  // scope before any of its lanes loads a partial.  (Every lane's load of vn_state has completed by here, its value fed the
  // loop above, so the last workgroup may overwrite the state.)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int t = __hip_atomic_fetch_add(p.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = t == (int)gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_last = last;
  }
  __syncthreads();
  if (!s_last) return;

  // ---- last workgroup: final_reduce_kernel<3> twice, valuenorm_update_n_kernel, the fill ----
  const int nblk = (int)gridDim.x;
  double ra[3], rm[3];
  final_reduce_sum<3>(pa, nblk, ra, smem);
  final_reduce_sum<3>(pm, nblk, rm, smem);
  for (int64_t i = threadIdx.x; i < p.n_zero; i += blockDim.x) p.zero[i] = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      p.adv_moments[i] = ra[i];
      p.mb_moments[i] = rm[i];
    }
    const double B = (double)p.n;
    p.mb_moments[3] = B;
    if (p.vn_state) valuenorm_update_n_body(p.vn_state, rm[0], rm[1], B, p.w, p.omw, p.n_epochs, p.states_out);
    __hip_atomic_store(p.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next call / graph replay starts clean
  }
}

extern "C" int64_t mappo_train_prologue_workspace_bytes(int64_t n) { return (int64_t)STAT_MAX_BLOCKS * 6 * sizeof(double); }

extern "C" int mappo_train_prologue(const float *returns, const float *value_preds, const float *active_masks, float *vn_state,
                                    float *adv, double *adv_moments, double *mb_moments, double beta, int32_t n_epochs,
                                    float *states_out, double *zero, int64_t n_zero, void *workspace, int32_t *ticket, int64_t n,
                                    mappo_stream_t stream) {
  MAPPO_REQUIRE(n > 0 && returns && value_preds && active_masks && adv && adv_moments && mb_moments && workspace && ticket,
                "train_prologue: bad arguments (n=%lld)", (long long)n);
  MAPPO_REQUIRE(!vn_state || (states_out && n_epochs >= 1), "train_prologue: a ValueNorm state needs states_out and n_epochs >= 1");
  MAPPO_REQUIRE(n_zero >= 0 && (n_zero == 0 || zero), "train_prologue: bad fill range (n_zero=%lld)", (long long)n_zero);
  PrologueArgs p;
  p.returns = returns; p.value_preds = value_preds; p.active = active_masks; p.vn_state = vn_state; p.adv = adv;
  p.partials = (double *)workspace; p.ticket = (int *)ticket; p.adv_moments = adv_moments; p.mb_moments = mb_moments;
  // (1 - beta) in double, then fp32: see mappo_valuenorm_update
  p.w = (float)beta; p.omw = (float)(1.0 - beta); p.n_epochs = (int)n_epochs; p.states_out = states_out;
  p.zero = zero; p.n_zero = n_zero; p.n = n;
  hipLaunchKernelGGL(train_prologue_kernel, dim3(stat_blocks(n)), dim3(STAT_BLOCK), 0, as_stream(stream), p);
  MAPPO_CHECK_LAUNCH("train_prologue");
  return MAPPO_OK;
}

// workgroup 0: update_stats_kernel; workgroups 1..nb: copy_batch_kernel's grid of nb
__global__ __launch_bounds__(256) void train_epilogue_kernel(const double *__restrict__ pa, const double *__restrict__ pc, int na, int nc,
                                                            const double *__restrict__ mb_moments, int use_policy_active,
                                                            int use_value_active, double *__restrict__ stats,
                                                            double *__restrict__ acc, CopyBatch c) {
  __shared__ double smem[16 * 4];
  if (blockIdx.x == 0) {
    update_stats_body(pa, pc, na, nc, mb_moments, use_policy_active, use_value_active, stats, acc, smem);
    return;
  }
  copy_batch_body(c, (int)blockIdx.x - 1, (int)gridDim.x - 1);
}

extern "C" int mappo_train_epilogue(const double *actor_partials, int32_t n_actor, const double *critic_partials, int32_t n_critic,
                                    const double *mb_moments, const mappo_ppo_cfg *cfg, double *stats, double *acc, int32_t count,
                                    float *const *dst, const float *const *src, const int64_t *n_floats, mappo_stream_t stream) {
  MAPPO_REQUIRE(critic_partials && mb_moments && cfg && stats && n_critic > 0 && n_actor >= 0, "train_epilogue: bad arguments");
  MAPPO_REQUIRE(count >= 1 && count <= COPY_MAX && dst && src && n_floats, "train_epilogue: bad copy list (count=%d)", count);
  CopyBatch c;
  c.count = count;
  int64_t total = 0;
  for (int j = 0; j < count; ++j) {
    MAPPO_REQUIRE(dst[j] && src[j] && n_floats[j] >= 0, "train_epilogue: copy entry %d", j);
    c.dst[j] = dst[j]; c.src[j] = src[j]; c.n[j] = n_floats[j];
    total += n_floats[j];
  }
  hipLaunchKernelGGL(train_epilogue_kernel, dim3((unsigned)copy_batch_blocks(total) + 1u), dim3(256), 0, as_stream(stream),
                     actor_partials, critic_partials, actor_partials ? (int)n_actor : 0, (int)n_critic, mb_moments,
                     cfg->use_policy_active_masks, cfg->use_value_active_masks, stats, acc, c);
  MAPPO_CHECK_LAUNCH("train_epilogue");
  return MAPPO_OK;
}
