// optim.hip — K10 + K11: gradient slab reduction, global-norm clipping and Adam on ONE flat buffer.
//   clip : torch.nn.utils.clip_grad_norm_ (r_mappo.py:143-146,157-160): norm = ||g||_2 over the segment,
//          coef = min(1, max_norm / (norm + 1e-6)), the PRE-clip norm is what train_info logs.
//   Adam : torch.optim.Adam defaults + eps=opti_eps (rMAPPOPolicy.py:31-37):
//          m += (g-m)(1-b1); v = v*b2 + g*g*(1-b2); p -= (lr/(1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps).
// The flat buffer holds `n_seg` segments (actor | critic), each a multiple of 256 floats so that a
// 256-thread block never straddles two segments.  Step counters and hyper-parameters are device resident
// (lr_decay just rewrites one float), so the whole update is capturable in a hipGraph.
#include "common.h"

#define OPT_BLOCK 256
#define OPT_MAX_SEG 4

struct SegBounds {
  int64_t b[OPT_MAX_SEG + 1];
  int n;
};

__device__ __forceinline__ int seg_of(const SegBounds &sb, int64_t i) {
  int s = 0;
#pragma unroll
  for (int k = 1; k < OPT_MAX_SEG; ++k)
    if (k < sb.n && i >= sb.b[k]) s = k;
  return s;
}

// grad[p] = sum over slabs (per-workgroup partial gradients written by the update kernels); coalesced in p.  A workgroup owns
// 128 parameters and splits the slab rows in four: quarter q (two waves) sums rows [q n / 4, (q + 1) n / 4), the quarters meet
// in LDS in a fixed order (deterministic).  The rows were written a moment ago on other XCDs, so every load is a long one: a
// thread issues ALL loads of its quarter (up to SLAB_INFLIGHT batches of 16 and the tail of up to 15, 79 registers) before the
// first add and pays that latency once; the adds then run in the order of the batch-by-batch walk this replaces (three to four
// latencies in a row at 134 slabs): rows of a full batch into acc[j & 3], the tail into acc[0].  Longer quarters repeat the block.
#define SLAB_BLOCK 128
#define SLAB_Q 4
#define SLAB_BATCH 16
#define SLAB_INFLIGHT 4
__device__ __forceinline__ float slab_quarter_sum(const float *__restrict__ slabs, int n_slabs, int64_t stride, int64_t p, int quarter) {
  const int s_hi = (int)(((int64_t)(quarter + 1) * n_slabs) / SLAB_Q);
  int s = (int)(((int64_t)quarter * n_slabs) / SLAB_Q);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (;;) {
    const int left = (s_hi - s) / SLAB_BATCH;                              // full batches still to add (wave-uniform)
    const int nb = left < SLAB_INFLIGHT ? left : SLAB_INFLIGHT;
    const int nt = left <= SLAB_INFLIGHT ? (s_hi - s) - nb * SLAB_BATCH : 0;   // the tail rides with the last block
    float v[SLAB_INFLIGHT][SLAB_BATCH], t[SLAB_BATCH - 1];
#pragma unroll
    for (int b = 0; b < SLAB_INFLIGHT; ++b)
      if (b < nb) {
#pragma unroll
        for (int j = 0; j < SLAB_BATCH; ++j) v[b][j] = slabs[(size_t)(s + b * SLAB_BATCH + j) * stride + p];
      }
#pragma unroll
    for (int j = 0; j < SLAB_BATCH - 1; ++j)
      if (j < nt) t[j] = slabs[(size_t)(s + nb * SLAB_BATCH + j) * stride + p];
#pragma unroll
    for (int b = 0; b < SLAB_INFLIGHT; ++b)
      if (b < nb) {
#pragma unroll
        for (int j = 0; j < SLAB_BATCH; ++j) acc[j & 3] += v[b][j];        // fixed association: deterministic
      }
#pragma unroll
    for (int j = 0; j < SLAB_BATCH - 1; ++j)
      if (j < nt) acc[0] += t[j];
    if (left <= SLAB_INFLIGHT) break;
    s += SLAB_INFLIGHT * SLAB_BATCH;
  }
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}
// the workgroup's 128 sums: valid in the threads of quarter 0 (threadIdx.x < 128), 0 elsewhere
__device__ __forceinline__ float slab_block_sum(const float *__restrict__ slabs, int n_slabs, int64_t stride, int64_t P, int64_t &p_out,
                                                const unsigned bid) {
  __shared__ float sq[SLAB_Q][SLAB_BLOCK];
  const int pi = threadIdx.x & (SLAB_BLOCK - 1), quarter = threadIdx.x / SLAB_BLOCK;
  const int64_t p = (int64_t)bid * SLAB_BLOCK + pi;
  p_out = p;
  sq[quarter][pi] = p < P ? slab_quarter_sum(slabs, n_slabs, stride, p, quarter) : 0.f;
  __syncthreads();
  return quarter == 0 ? (sq[0][pi] + sq[1][pi]) + (sq[2][pi] + sq[3][pi]) : 0.f;
}

__global__ __launch_bounds__(SLAB_BLOCK * SLAB_Q) void slab_reduce_kernel(const float *__restrict__ slabs, int n_slabs,
                                                                         int64_t stride, int64_t P, float *__restrict__ grad) {
  int64_t p;
  const float g = slab_block_sum(slabs, n_slabs, stride, P, p, blockIdx.x);
  if (threadIdx.x < SLAB_BLOCK && p < P) grad[p] = g;
}

// ---- two-launch variant of slab_reduce + clip_adam (the per-update tail of the PPO loop is launch-bound: every
// kernel here runs a few microseconds, so the launches themselves are what it costs) --------------------------------
// (1) slab_reduce that also leaves the squared-norm partial of its 128 gradient entries;
// (2) norm finalisation + Adam in one kernel (see norm_adam_kernel).
// (bid: the workgroup's index among those of ITS flat buffer — blockIdx.x, or the job-local index of the grouped launch)
//
// The launch has ONE workgroup more than the gradient needs (bid == P / 128).  It advances the Adam step of the enabled segments
// and leaves what Adam needs of (beta1, beta2, t) — nothing of it depends on the gradient — in the workspace behind the
// partials, OPT_SCAL floats per segment: lr / (1 - beta1^t), sqrt(1 - beta2^t), enabled.  Its two double-precision pow()s per
// segment run beside the reduction on a CU of their own, not between the barriers of every norm_adam workgroup; the kernel
// boundary orders them before norm_adam.
#define OPT_SCAL 4
__device__ __forceinline__ float *adam_scalars(double *partials, int64_t P) { return (float *)(partials + P / SLAB_BLOCK); }
__device__ __forceinline__ const float *adam_scalars(const double *partials, int64_t P) { return (const float *)(partials + P / SLAB_BLOCK); }
__device__ __forceinline__ void adam_step_scalars(const float *__restrict__ hyper, int32_t *step, int n_seg, float *__restrict__ scal) {
  if ((int)threadIdx.x >= n_seg) return;
  const float *h = hyper + threadIdx.x * 8;
  const bool on = h[7] != 0.f;
  int t = step[threadIdx.x];
  if (on) step[threadIdx.x] = ++t;                                       // Adam step of enabled segments
  const double bc1 = 1.0 - pow((double)h[1], (double)t);
  const double bc2 = 1.0 - pow((double)h[2], (double)t);
  scal[threadIdx.x * OPT_SCAL + 0] = (float)((double)h[0] / (bc1 > 0.0 ? bc1 : 1.0));
  scal[threadIdx.x * OPT_SCAL + 1] = (float)sqrt(bc2 > 0.0 ? bc2 : 1.0);
  scal[threadIdx.x * OPT_SCAL + 2] = on ? 1.f : 0.f;
}
__device__ __forceinline__ void slab_reduce_sq_body(const float *__restrict__ slabs, int n_slabs, int64_t stride, int64_t P, float *__restrict__ grad,
                                                    double *__restrict__ partials, const float *__restrict__ hyper, int32_t *step, int n_seg,
                                                    const unsigned bid) {
  __shared__ double smem[16];
  if ((int64_t)bid * SLAB_BLOCK >= P) {                                  // the extra workgroup (uniform: no barrier is skipped by a part)
    adam_step_scalars(hyper, step, n_seg, adam_scalars(partials, P));
    return;
  }
  int64_t p;
  const float g = slab_block_sum(slabs, n_slabs, stride, P, p, bid);    // (0 in the threads of quarters 1..3)
  if (threadIdx.x < SLAB_BLOCK && p < P) grad[p] = g;
  double v[1] = {(double)g * (double)g};
  block_sum<1>(v, smem);
  if (threadIdx.x == 0) partials[bid] = v[0];
}
__global__ __launch_bounds__(SLAB_BLOCK * SLAB_Q) void slab_reduce_sq_kernel(const float *__restrict__ slabs, int n_slabs, int64_t stride,
                                                                            int64_t P, float *__restrict__ grad, double *__restrict__ partials,
                                                                            const float *__restrict__ hyper, int32_t *step, int n_seg) {
  slab_reduce_sq_body(slabs, n_slabs, stride, P, grad, partials, hyper, step, n_seg, blockIdx.x);
}

// squared-norm partials per 128 gradient entries (+ the extra workgroup's Adam step increment and scalars): the first launch of
// mappo_clip_adam when the gradient was reduced elsewhere (data-parallel all-reduce, recurrent path)
__global__ __launch_bounds__(SLAB_BLOCK) void sqnorm128_kernel(const float *__restrict__ grad, int64_t P, double *__restrict__ partials,
                                                              const float *__restrict__ hyper, int32_t *step, int n_seg) {
  __shared__ double smem[16];
  if ((int64_t)blockIdx.x * SLAB_BLOCK >= P) {                           // the extra workgroup, as in slab_reduce_sq_body
    adam_step_scalars(hyper, step, n_seg, adam_scalars(partials, P));
    return;
  }
  const int64_t p = (int64_t)blockIdx.x * SLAB_BLOCK + threadIdx.x;
  double v[1] = {0.0};
  if (p < P) { const double g = (double)grad[p]; v[0] = g * g; }
  block_sum<1>(v, smem);
  if (threadIdx.x == 0) partials[blockIdx.x] = v[0];
}

// One 256-thread workgroup per 256 parameters (never straddles a segment).  Every workgroup finalises the norm of ITS
// segment itself (a few dozen partials: redundant across workgroups, but in parallel and without a separate launch), then
// applies Adam to its slice with the step scalars the launch before left behind the partials (adam_step_scalars; a kernel
// boundary orders them before every read here).  Between the two barriers thread 0 has a sqrt and the clip coefficient to do,
// no load and no pow().  Workgroup 0 also publishes the norms.
__device__ __forceinline__ void norm_adam_body(const double *__restrict__ partials, const SegBounds &sb, const float *__restrict__ hyper,
                                               float *__restrict__ grad_norms, double *__restrict__ norm_acc,
                                               float *__restrict__ params, const float *__restrict__ grad, float *__restrict__ m,
                                               float *__restrict__ v, const unsigned bid) {
  __shared__ double smem[16];
  __shared__ float ws_coef;
  const int64_t i = (int64_t)bid * OPT_BLOCK + threadIdx.x;
  const int s = seg_of(sb, (int64_t)bid * OPT_BLOCK);
  // everything the workgroup reads is requested here, so that it waits for memory once: the partials of its segment, its slice,
  // the hyper-parameters and the step scalars of the launch before (adam_step_scalars)
  const float gi = grad[i], pi = params[i], mi0 = m[i], vi0 = v[i];
  double acc[1] = {0.0};
  for (int b = (int)(sb.b[s] / SLAB_BLOCK) + threadIdx.x; b < (int)(sb.b[s + 1] / SLAB_BLOCK); b += OPT_BLOCK) acc[0] += partials[b];
  const float *h = hyper + s * 8, *sc = adam_scalars(partials, sb.b[sb.n]) + s * OPT_SCAL;
  const float b1 = h[1], b2 = h[2], eps = h[3], wd = h[4], max_norm = h[5], use_clip = h[6];
  const float lr_bc1 = sc[0], sqrt_bc2 = sc[1], enabled = sc[2];
  block_sum<1>(acc, smem);
  float norm = 0.f;
  if (threadIdx.x == 0) {
    norm = (float)sqrt(acc[0]);
    float coef = 1.f;
    if (use_clip != 0.f) coef = fminf(max_norm / (norm + 1e-6f), 1.f);
    ws_coef = coef;
  }
  __syncthreads();
  if (enabled != 0.f) {
    float g = gi * ws_coef;
    float pp = pi;
    if (wd != 0.f) g = g + wd * pp;
    float mi = mi0, vi = vi0;
    mi = mi + (g - mi) * (1.f - b1);
    vi = vi * b2 + g * g * (1.f - b2);
    const float denom = sqrtf(vi) / sqrt_bc2 + eps;
    pp = pp - lr_bc1 * (mi / denom);
    params[i] = pp; m[i] = mi; v[i] = vi;
  }
  if (bid != 0) return;
  // workgroup 0 publishes the norms of all segments, behind its own slice: its segment's from the sum above, the others' here
  for (int sk = 0; sk < sb.n; ++sk) {
    float norm_k = norm;
    if (sk != s) {
      acc[0] = 0.0;
      for (int b = (int)(sb.b[sk] / SLAB_BLOCK) + threadIdx.x; b < (int)(sb.b[sk + 1] / SLAB_BLOCK); b += OPT_BLOCK) acc[0] += partials[b];
      block_sum<1>(acc, smem);
      if (threadIdx.x == 0) norm_k = (float)sqrt(acc[0]);
    }
    if (threadIdx.x == 0) {
      grad_norms[sk] = norm_k;
      if (norm_acc) norm_acc[sk] += (double)norm_k;
    }
  }
}
__global__ __launch_bounds__(OPT_BLOCK) void norm_adam_kernel(const double *__restrict__ partials, SegBounds sb,
                                                             const float *__restrict__ hyper, float *__restrict__ grad_norms, double *__restrict__ norm_acc,
                                                             float *__restrict__ params, const float *__restrict__ grad,
                                                             float *__restrict__ m, float *__restrict__ v) {
  norm_adam_body(partials, sb, hyper, grad_norms, norm_acc, params, grad, m, v, blockIdx.x);
}

// ---- the same two launches for up to MAPPO_MAX_GROUP flat buffers (mappo_reduce_clip_adam_group: the agents of a separated run).
// The job table travels in the kernel argument; a workgroup finds its job with wave-uniform compares and runs the single launch's
// body with its job-local index, so every job's arithmetic and order are the single call's.
struct OptJob {
  const float *slabs, *hyper;
  float *params, *grad, *m, *v, *grad_norms;
  double *partials, *norm_acc;
  int32_t *step;
  int64_t stride;
  SegBounds sb;
  int n_slabs;
  int rblock0, ablock0;      // first workgroup of the job in the reduce launch (P / 128 + 1 each) / in the Adam launch (P / 256 each)
};
struct OptGroup {
  OptJob job[MAPPO_MAX_GROUP];
  int n_jobs;
};
static_assert(sizeof(OptGroup) <= 4096, "the job table must fit the kernel argument segment");

__global__ __launch_bounds__(SLAB_BLOCK * SLAB_Q) void slab_reduce_sq_group_kernel(OptGroup g) {
  int j = 0;
#pragma unroll
  for (int k = 1; k < MAPPO_MAX_GROUP; ++k)
    if (k < g.n_jobs && (int)blockIdx.x >= g.job[k].rblock0) j = k;
  const OptJob &J = g.job[j];
  slab_reduce_sq_body(J.slabs, J.n_slabs, J.stride, J.sb.b[J.sb.n], J.grad, J.partials, J.hyper, J.step, J.sb.n, blockIdx.x - (unsigned)J.rblock0);
}
__global__ __launch_bounds__(OPT_BLOCK) void norm_adam_group_kernel(OptGroup g) {
  int j = 0;
#pragma unroll
  for (int k = 1; k < MAPPO_MAX_GROUP; ++k)
    if (k < g.n_jobs && (int)blockIdx.x >= g.job[k].ablock0) j = k;
  const OptJob &J = g.job[j];
  norm_adam_body(J.partials, J.sb, J.hyper, J.grad_norms, J.norm_acc, J.params, J.grad, J.m, J.v, blockIdx.x - (unsigned)J.ablock0);
}

extern "C" int64_t mappo_optim_workspace_bytes(int64_t P) {
  const int64_t nblk = (P + SLAB_BLOCK - 1) / SLAB_BLOCK;       // mappo_reduce_clip_adam keeps one partial per 128 entries
  return nblk * (int64_t)sizeof(double) + OPT_MAX_SEG * OPT_SCAL * (int64_t)sizeof(float) + 64;   // partials | step scalars
}

extern "C" int mappo_slab_reduce(const float *slabs, int32_t n_slabs, int64_t slab_stride, int64_t P, float *grad,
                                 mappo_stream_t stream) {
  MAPPO_REQUIRE(slabs && grad && n_slabs > 0 && P > 0 && slab_stride >= P, "slab_reduce: bad arguments");
  const int nblk = (int)((P + SLAB_BLOCK - 1) / SLAB_BLOCK);
  PROF_LAUNCH(MAPPO_PROF_SLAB_REDUCE, slab_reduce_kernel, dim3(nblk), dim3(SLAB_BLOCK * SLAB_Q), 0, as_stream(stream), slabs,
              (int)n_slabs, slab_stride, P, grad);
  MAPPO_CHECK_LAUNCH("slab_reduce");
  return MAPPO_OK;
}

extern "C" int mappo_clip_adam(float *params, const float *grad, float *exp_avg, float *exp_avg_sq,
                               const int64_t *seg_bounds, int32_t n_seg, const float *opt_hyper, int32_t *opt_step,
                               float *grad_norms, double *norm_acc, void *workspace, mappo_stream_t stream) {
  MAPPO_REQUIRE(params && grad && exp_avg && exp_avg_sq && seg_bounds && opt_hyper && opt_step && grad_norms && workspace,
                "clip_adam: null pointer");
  MAPPO_REQUIRE(n_seg >= 1 && n_seg <= OPT_MAX_SEG, "clip_adam: n_seg=%d", n_seg);
  SegBounds sb;
  sb.n = n_seg;
  for (int s = 0; s <= n_seg; ++s) {
    MAPPO_REQUIRE(seg_bounds[s] % OPT_BLOCK == 0 && (s == 0 || seg_bounds[s] > seg_bounds[s - 1]),
                  "clip_adam: segment bounds must be increasing multiples of %d", OPT_BLOCK);
    sb.b[s] = seg_bounds[s];
  }
  MAPPO_REQUIRE(seg_bounds[0] == 0, "clip_adam: seg_bounds[0] must be 0");
  const int64_t P = seg_bounds[n_seg];
  double *partials = (double *)workspace;
  hipStream_t st = as_stream(stream);
  // two launches: squared-norm partials (+ step increment), then norm finalisation + Adam in one kernel
  PROF_BEGIN(MAPPO_PROF_ADAM, st);
  hipLaunchKernelGGL(sqnorm128_kernel, dim3((unsigned)(P / SLAB_BLOCK) + 1), dim3(SLAB_BLOCK), 0, st, grad, P, partials, opt_hyper, opt_step,
                     (int)n_seg);
  hipLaunchKernelGGL(norm_adam_kernel, dim3((unsigned)(P / OPT_BLOCK)), dim3(OPT_BLOCK), 0, st, (const double *)partials, sb, opt_hyper,
                     grad_norms, norm_acc, params, grad, exp_avg, exp_avg_sq);
  PROF_END(MAPPO_PROF_ADAM, st);
  MAPPO_CHECK_LAUNCH("clip_adam");
  return MAPPO_OK;
}

extern "C" int mappo_reduce_clip_adam(const float *slabs, int32_t n_slabs, int64_t slab_stride, float *params, float *grad,
                                      float *exp_avg, float *exp_avg_sq, const int64_t *seg_bounds, int32_t n_seg,
                                      const float *opt_hyper, int32_t *opt_step, float *grad_norms, double *norm_acc,
                                      void *workspace, mappo_stream_t stream) {
  MAPPO_REQUIRE(slabs && params && grad && exp_avg && exp_avg_sq && seg_bounds && opt_hyper && opt_step && grad_norms && workspace,
                "reduce_clip_adam: null pointer");
  MAPPO_REQUIRE(n_seg >= 1 && n_seg <= OPT_MAX_SEG && n_slabs > 0, "reduce_clip_adam: n_seg=%d n_slabs=%d", n_seg, n_slabs);
  SegBounds sb;
  sb.n = n_seg;
  for (int s = 0; s <= n_seg; ++s) {
    MAPPO_REQUIRE(seg_bounds[s] % OPT_BLOCK == 0 && (s == 0 || seg_bounds[s] > seg_bounds[s - 1]),
                  "reduce_clip_adam: segment bounds must be increasing multiples of %d", OPT_BLOCK);
    sb.b[s] = seg_bounds[s];
  }
  MAPPO_REQUIRE(seg_bounds[0] == 0, "reduce_clip_adam: seg_bounds[0] must be 0");
  const int64_t P = seg_bounds[n_seg];
  MAPPO_REQUIRE(slab_stride >= P, "reduce_clip_adam: slab_stride < P");
  const int nblk = (int)(P / SLAB_BLOCK);             // P is a multiple of 256: mappo_optim_workspace_bytes(P) covers P/128 doubles
  double *partials = (double *)workspace;
  hipStream_t st = as_stream(stream);
  PROF_LAUNCH(MAPPO_PROF_SLAB_REDUCE, slab_reduce_sq_kernel, dim3(nblk + 1), dim3(SLAB_BLOCK * SLAB_Q), 0, st, slabs, (int)n_slabs, slab_stride, P,
              grad, partials, opt_hyper, opt_step, (int)n_seg);
  PROF_LAUNCH(MAPPO_PROF_ADAM, norm_adam_kernel, dim3((unsigned)(P / OPT_BLOCK)), dim3(OPT_BLOCK), 0, st, (const double *)partials, sb,
              opt_hyper, grad_norms, norm_acc, params, (const float *)grad, exp_avg, exp_avg_sq);
  MAPPO_CHECK_LAUNCH("reduce_clip_adam");
  return MAPPO_OK;
}

extern "C" int mappo_reduce_clip_adam_group(const mappo_optim_job *jobs, int32_t n_jobs, mappo_stream_t stream) {
  const char *who = "reduce_clip_adam_group";
  MAPPO_REQUIRE(n_jobs >= 1 && n_jobs <= MAPPO_MAX_GROUP, "%s: n_jobs=%d outside [1,%d] (job count)", who, n_jobs, MAPPO_MAX_GROUP);
  MAPPO_REQUIRE(jobs, "%s: null job array (job 0)", who);
  OptGroup g = {};
  g.n_jobs = n_jobs;
  int rblocks = 0, ablocks = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const mappo_optim_job &J = jobs[j];
    MAPPO_REQUIRE(J.slabs && J.params && J.grad && J.exp_avg && J.exp_avg_sq && J.opt_hyper && J.opt_step && J.grad_norms && J.workspace,
                  "%s: job %d: null pointer", who, j);
    MAPPO_REQUIRE(J.n_seg >= 1 && J.n_seg <= OPT_MAX_SEG && J.n_slabs > 0, "%s: job %d: n_seg=%d n_slabs=%d", who, j, J.n_seg, J.n_slabs);
    OptJob &G = g.job[j];
    G.sb.n = J.n_seg;
    for (int s = 0; s <= J.n_seg; ++s) {
      MAPPO_REQUIRE(J.seg_bounds[s] % OPT_BLOCK == 0 && (s == 0 || J.seg_bounds[s] > J.seg_bounds[s - 1]),
                    "%s: job %d: segment bounds must be increasing multiples of %d", who, j, OPT_BLOCK);
      G.sb.b[s] = J.seg_bounds[s];
    }
    MAPPO_REQUIRE(J.seg_bounds[0] == 0, "%s: job %d: seg_bounds[0] must be 0", who, j);
    const int64_t P = J.seg_bounds[J.n_seg];
    MAPPO_REQUIRE(J.slab_stride >= P, "%s: job %d: slab_stride < P", who, j);
    G.slabs = J.slabs; G.hyper = J.opt_hyper; G.params = J.params; G.grad = J.grad; G.m = J.exp_avg; G.v = J.exp_avg_sq;
    G.grad_norms = J.grad_norms; G.partials = (double *)J.workspace; G.norm_acc = J.norm_acc; G.step = J.opt_step;
    G.stride = J.slab_stride; G.n_slabs = J.n_slabs;
    G.rblock0 = rblocks; G.ablock0 = ablocks;
    rblocks += (int)(P / SLAB_BLOCK) + 1;               // P is a multiple of 256: mappo_optim_workspace_bytes(P) covers P/128 doubles; + the step workgroup
    ablocks += (int)(P / OPT_BLOCK);
  }
  hipStream_t st = as_stream(stream);
  PROF_LAUNCH(MAPPO_PROF_SLAB_REDUCE, slab_reduce_sq_group_kernel, dim3((unsigned)rblocks), dim3(SLAB_BLOCK * SLAB_Q), 0, st, g);
  PROF_LAUNCH(MAPPO_PROF_ADAM, norm_adam_group_kernel, dim3((unsigned)ablocks), dim3(OPT_BLOCK), 0, st, g);
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}
