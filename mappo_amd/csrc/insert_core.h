// insert_core.h — the MPE rollout insert (see insert.hip) as a device function, shared with the fused rollout-step kernel.
#pragma once
#include "common.h"

struct InsertArgs {
  const float *obs;  int64_t obs_sn, obs_sm;       // element (n, m, d) at obs[n*obs_sn + m*obs_sm + d]
  const float *rew;  int64_t rew_sn, rew_sm;       // element (n, m)    at rew[n*rew_sn + m*rew_sm]   (0 strides broadcast)
  const uint8_t *done; int64_t done_sn, done_sm;   // bool bytes
  float *obs_dst, *share_dst, *rew_dst, *mask_dst; // contiguous slots
  int N, M, D, centralized;
};

// workgroup `bid` of `nb` cooperating 256-thread workgroups
__device__ __forceinline__ void insert_mpe_body(const InsertArgs &p, int bid, int nb) {
  const int S = p.centralized ? p.M * p.D : p.D;
  const int64_t total = (int64_t)p.N * p.M * S;
  for (int64_t e = (int64_t)bid * blockDim.x + threadIdx.x; e < total; e += (int64_t)nb * blockDim.x) {
    const int64_t nm = e / S;
    const int j = (int)(e - nm * S);
    const int n = (int)(nm / p.M), m = (int)(nm - (int64_t)n * p.M);
    const int ms = p.centralized ? j / p.D : m, d = p.centralized ? j - ms * p.D : j;      // source agent / feature
    const float v = p.obs[n * p.obs_sn + ms * p.obs_sm + d];
    p.share_dst[e] = v;
    if (!p.centralized || ms == m) p.obs_dst[nm * p.D + d] = v;                            // each obs element exactly once
    if (j == 0) {
      p.rew_dst[nm] = p.rew[n * p.rew_sn + m * p.rew_sm];
      p.mask_dst[nm] = p.done[n * p.done_sn + m * p.done_sm] ? 0.f : 1.f;
    }
  }
}

// The MPE insert of a whole episode (rollout_episode_kernel): p describes step 0 (sources: the env output of step 0, destinations:
// the buffer slots it goes to); step t reads the sources t * *_st further and writes t slots further.  Flattened over (step,
// element), U elements per lane per pass with every load of a pass issued before its stores: one dependent round trip per
// element (insert_mpe_body's loop) made this role the long pole of the launch.  Wave w of the nw waves that share the copy.
// I: the type of the (step, row, element) split of an element index — three divisions per element, which in 64 bits are
// software sequences that made the copy instruction-bound; 32 bits whenever the episode's element count fits.
template <int U, typename I>
__device__ __forceinline__ void insert_mpe_episode_run(const InsertArgs &p, int64_t obs_st, int64_t rew_st, int64_t done_st, int T,
                                                       int w, int nw) {
  const int S = p.centralized ? p.M * p.D : p.D;
  const int64_t R = (int64_t)p.N * p.M, RS = R * S, total = (int64_t)T * RS, nthr = (int64_t)nw * WAVE;
  for (int64_t e0 = (int64_t)w * WAVE + (threadIdx.x & (WAVE - 1)); e0 < total; e0 += U * nthr) {
    float v[U], rw[U];
    uint8_t dn[U];                                   // raw: a compare here would wait for the load (and every load before it)
    int64_t tn[U];                                   // t * R + nm: the row's index in the [T][R] slots
    int dd[U], jj[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t e = e0 + u * nthr;
      jj[u] = -1;
      if (e < total) {
        const I t = (I)e / (I)RS, rem = (I)e - t * (I)RS, nm = rem / (I)S;
        const int j = (int)(rem - nm * (I)S);
        const int n = (int)(nm / (I)p.M), m = (int)(nm - (I)n * (I)p.M);
        const int ms = p.centralized ? j / p.D : m, d = p.centralized ? j - ms * p.D : j;      // source agent / feature
        v[u] = p.obs[(int64_t)t * obs_st + n * p.obs_sn + ms * p.obs_sm + d];
        tn[u] = (int64_t)t * R + (int64_t)nm;
        dd[u] = (!p.centralized || ms == m) ? d : -1;                                        // each obs element exactly once
        jj[u] = j;
        if (j == 0) {
          rw[u] = p.rew[(int64_t)t * rew_st + n * p.rew_sn + m * p.rew_sm];
          dn[u] = p.done[(int64_t)t * done_st + n * p.done_sn + m * p.done_sm];
        }
      }
    }
    // one wait for the whole pass: the stores sit in divergent branches, where the counter's bookkeeping otherwise falls back to
    // a full wait (loads AND the stores before) in front of every group of stores
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (jj[u] < 0) continue;
      p.share_dst[e0 + u * nthr] = v[u];                                                     // share slots t + 1 are contiguous
      if (dd[u] >= 0) p.obs_dst[tn[u] * p.D + dd[u]] = v[u];
      if (jj[u] == 0) {
        p.rew_dst[tn[u]] = rw[u];
        p.mask_dst[tn[u]] = dn[u] != 0 ? 0.f : 1.f;
      }
    }
  }
}
template <int U>
__device__ __forceinline__ void insert_mpe_episode_body(const InsertArgs &p, int64_t obs_st, int64_t rew_st, int64_t done_st, int T,
                                                        int w, int nw) {
  const int64_t total = (int64_t)T * p.N * p.M * (p.centralized ? p.M * p.D : p.D);
  if (total <= (int64_t)UINT32_MAX) insert_mpe_episode_run<U, uint32_t>(p, obs_st, rew_st, done_st, T, w, nw);
  else insert_mpe_episode_run<U, int64_t>(p, obs_st, rew_st, done_st, T, w, nw);
}

// ---- the SMAC rollout insert (insert.hip: mappo_insert_smac) as a device function, shared with the fused recurrent rollout step ----
struct SmacInsert {
  const float *obs, *share, *avail;              // contiguous [N*M][D | S | A]
  const float *rew; int64_t rew_sn, rew_sm;
  const uint8_t *done; int64_t done_sn, done_sm;
  const uint8_t *bad;                            // contiguous [N*M] bool bytes or NULL (no bad transitions)
  const float *h_a, *h_c;                        // contiguous [N*M][H] or NULL
  float *obs_dst, *share_dst, *avail_dst, *rew_dst, *mask_dst, *bad_dst, *active_dst, *ha_dst, *hc_dst;
  int N, M, D, S, A, H;
};
__device__ __forceinline__ bool env_done(const SmacInsert &p, int n) {
  bool all = true;
  for (int m = 0; m < p.M; ++m) all = all && p.done[n * p.done_sn + m * p.done_sm] != 0;
  return all;
}
// workgroup `bid` of `nb` cooperating workgroups
__device__ __forceinline__ void insert_smac_body(const SmacInsert &p, int bid, int nb) {
  const int64_t tid = (int64_t)bid * blockDim.x + threadIdx.x, nthr = (int64_t)nb * blockDim.x;
  const int64_t R = (int64_t)p.N * p.M;
  for (int64_t e = tid; e < R * p.D; e += nthr) p.obs_dst[e] = p.obs[e];
  for (int64_t e = tid; e < R * p.S; e += nthr) p.share_dst[e] = p.share[e];
  if (p.avail)
    for (int64_t e = tid; e < R * p.A; e += nthr) p.avail_dst[e] = p.avail[e];
  for (int64_t e = tid; e < R; e += nthr) {
    const int n = (int)(e / p.M), m = (int)(e - (int64_t)n * p.M);
    const bool de = env_done(p, n), d = p.done[n * p.done_sn + m * p.done_sm] != 0;
    p.rew_dst[e] = p.rew[n * p.rew_sn + m * p.rew_sm];
    p.mask_dst[e] = de ? 0.f : 1.f;
    p.active_dst[e] = de ? 1.f : (d ? 0.f : 1.f);
    p.bad_dst[e] = (p.bad && p.bad[e]) ? 0.f : 1.f;
  }
  if (p.h_a) {
    const int h4 = p.H >> 2;
    for (int64_t e = tid; e < R * h4; e += nthr) {
      const int n = (int)((e / h4) / p.M);
      const float keep = env_done(p, n) ? 0.f : 1.f;
      float4 a = reinterpret_cast<const float4 *>(p.h_a)[e], c = reinterpret_cast<const float4 *>(p.h_c)[e];
      a.x *= keep; a.y *= keep; a.z *= keep; a.w *= keep;
      c.x *= keep; c.y *= keep; c.z *= keep; c.w *= keep;
      reinterpret_cast<float4 *>(p.ha_dst)[e] = a;
      reinterpret_cast<float4 *>(p.hc_dst)[e] = c;
    }
  }
}


// after_update (see mappo_copy_batch): up to 16 independent device copies by `nb` cooperating 256-thread workgroups, this one `bid`
#define COPY_MAX 16
struct CopyBatch {
  float *dst[COPY_MAX];
  const float *src[COPY_MAX];
  int64_t n[COPY_MAX];          // floats
  int count;
};
static inline int copy_batch_blocks(int64_t total_floats) {
  int64_t nb = (total_floats / 4 + 255) / 256;
  if (nb < 1) nb = 1;
  if (nb > 1024) nb = 1024;
  return (int)nb;
}
__device__ __forceinline__ void copy_batch_body(const CopyBatch &c, int bid, int nb) {
  for (int j = 0; j < c.count; ++j) {
    const float *__restrict__ s = c.src[j];
    float *__restrict__ d = c.dst[j];
    const int64_t n = c.n[j];
    if (((((uintptr_t)s) | ((uintptr_t)d)) & 15) == 0) {
      const int64_t n4 = n >> 2;
      for (int64_t i = (int64_t)bid * blockDim.x + threadIdx.x; i < n4; i += (int64_t)nb * blockDim.x)
        reinterpret_cast<float4 *>(d)[i] = reinterpret_cast<const float4 *>(s)[i];
      for (int64_t i = (n4 << 2) + (int64_t)bid * blockDim.x + threadIdx.x; i < n; i += (int64_t)nb * blockDim.x) d[i] = s[i];
    } else {
      for (int64_t i = (int64_t)bid * blockDim.x + threadIdx.x; i < n; i += (int64_t)nb * blockDim.x) d[i] = s[i];
    }
  }
}
