// mlp_fwd.h — the forward family on 32-sample tiles (mlp_forward_kernel: evaluate_actions / get_values / get_actions / trunk
// features) and the kernels built on the register-resident 16-sample-tile forward (mlp_fwd16.h): the fused rollout step, the
// one-launch rollout episode and the trunk features of a recurrent network.  Needs mlp_blocks.h.
#pragma once
#include "mlp_blocks.h"

// ------------------------------------------------------------------------------------------------
// forward kernel.  MODE 0: out[B][A] = head output.   MODE 1: sample/argmax + log-prob (get_actions).
// ------------------------------------------------------------------------------------------------
struct FwdArgs {
  const float *params, *x;
  const int32_t *rows;
  const float *avail;
  float *out, *actions, *logp;
  mappo_net_desc desc;
  NetOff off;
  LdsMap map;
  int64_t B;
  int deterministic;
  uint64_t seed, counter;
  const uint64_t *counter_dev;   // optional device word added to `counter` (lets a captured hipGraph draw fresh numbers)
  // optional strided source rows (x_M > 0): sample i = (n, m) = (i / x_M, i % x_M) starts at x[n * x_sn + m * x_sm] — the
  // env's output read in place (fused rollout step); x_M == 0: contiguous rows x[i * in_dim]
  int64_t x_sn, x_sm;
  int x_M;
  // MODE 2 through forward16_tail (wide inputs) only: write the trunk output BLOCKED per 16-row tile, out[((i >> 4) * 4 + b) * 256 +
  // 4 * lane + r] = feature 16 b + 4 q + r of row i (B a multiple of 16) — the layout of the recurrent training kernels (gru_train16.hip)
  int out_blocked;
};

// XW: 0 = in_dim <= 32, 1 = in_dim <= 64 (rows prefetched into registers), 2 = in_dim > 64 (K-chunked layer 1)
// workgroup `bid` of `nb` workgroups that share the B rows (blockIdx / gridDim of a plain forward launch)
// MODE 5 (MultiDiscrete): MODE 1 with one sample / argmax per head of `md` -> actions / logp [B][md->n]
template <bool RELU, int LN, int MODE, int XW>
__device__ __forceinline__ void forward_body(const FwdArgs &p, float *lds, const int bid, const int nb, const MdHeads *md = nullptr) {
  constexpr bool WIDE = XW >= 1, XWIDE = XW == 2;
  const int n_waves = blockDim.x / WAVE;
  const NetOff &o = p.off;
  const LdsMap &m = p.map;
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), l31 = lane & 31, half = lane >> 5;
  const int D = p.desc.in_dim, Dp = (D + 1) & ~1, A = p.desc.out_dim;
  const uint32_t magic = (uint32_t)(0x100000000ull / (uint32_t)D) + 1u;
  const int64_t n_tiles = (p.B + TS - 1) / TS;
  const int64_t tile_stride = (int64_t)nb * n_waves;
  const int64_t n_btiles = (n_tiles + n_waves - 1) / n_waves;    // the tile loop is uniform over the workgroup's waves
  RowPrefetch<WIDE> pf;
  if (!XWIDE) prefetch_rows(pf, p.x, p.rows, ((int64_t)bid * n_waves + wave) * TS, p.B, D, lane, p.x_sn, p.x_sm, p.x_M);   // under the staging
  stage_all_weights<LN>(lds, m, p.params, o, p.desc);
  __syncthreads();
  float *tX = lds + m.tiles + wave * m.wave_stride;
  float *tH = tX + m.x_rows * TP;
  float *tZ = tH + (LN + 1) * HID * TP;
  for (int64_t tb = bid; tb < n_btiles; tb += nb) {
    const int64_t tile = tb * n_waves + wave;
    const int64_t base = tile * TS;
    int n_valid;
    TileStats<LN> st;
    if (!XWIDE) {
      n_valid = pf.n_valid;
      commit_rows(tX, tH + ((4 - ((m.x_rows * TP) & 3)) & 3), pf, D, magic, lane, p.desc.use_feature_norm != 0);   // 16-B aligned staging
      wave_lds_sync();
      prefetch_rows(pf, p.x, p.rows, (tile + tile_stride) * TS, p.B, D, lane, p.x_sn, p.x_sm, p.x_M);
      tile_forward<RELU, LN>(lds, m, tX, tH, D, l31, half, st);
    } else {
      n_valid = (int)max((int64_t)0, min((int64_t)TS, p.B - base));
      const bool ok = l31 < n_valid;
      const int64_t row = ok ? (p.rows ? (int64_t)p.rows[base + l31] : base + l31) : 0;
      const float *xr = p.x + row * D;
      float mean0, rstd0;
      wide_row_stats(xr, D, ok, half, p.desc.use_feature_norm != 0, mean0, rstd0);
      tile_forward_wide<RELU, LN>(lds, m, p.params + o.w1, xr, ok, mean0, rstd0, tX, tH, D, l31, half, st);
    }
    if (MODE == 2) {
      // trunk features (LayerNorm output of the last layer, affine applied) feature-major: out[f][B], the input
      // layout of the GRU kernels (gru.hip); a register's 32 lanes write one 128-B segment
      const float *tL = tH + LN * HID * TP, *sG = lds + ln_w_of<LN>(m, LN), *sBt = lds + ln_b_of<LN>(m, LN);
      if (l31 < n_valid) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int f = 32 * t + ROWMAP(r, half);
            p.out[(int64_t)f * p.B + base + l31] = tL[f * TP + l31] * sG[f] + sBt[f];
          }
      }
      wave_lds_sync();
      continue;
    }
    const f32x16 z = head_forward(lds, m, tH + LN * HID * TP, lds + ln_w_of<LN>(m, LN), lds + ln_b_of<LN>(m, LN), l31, half);
    head_to_tile(tZ, z, A, l31, half);
    wave_lds_sync();
    if (MODE == 0) {
      for (int e = lane; e < n_valid * A; e += WAVE) {
        const int s = e / A, a = e - s * A;
        p.out[base * A + e] = tZ[s * TP + a];
      }
    } else if (MODE == 5) {
      if (lane < n_valid) {
        const int64_t i = base + lane;
        const uint64_t ctr = p.counter + (p.counter_dev ? *p.counter_dev : 0ull);
        categorical_act_heads(tZ + lane * TP, *md, p.deterministic != 0, p.seed, ctr, (uint64_t)i, p.actions + i * md->n, p.logp + i * md->n);
      }
    } else {
      if (lane < n_valid) {
        const int64_t i = base + lane;
        const uint64_t ctr = p.counter + (p.counter_dev ? *p.counter_dev : 0ull);
        float action, logp;
        categorical_act_lane(tZ + lane * TP, A, p.avail ? p.avail + i * A : nullptr, p.deterministic != 0, p.seed, ctr, (uint64_t)i,
                             action, logp);
        p.actions[i] = action;
        p.logp[i] = logp;
      }
    }
    wave_lds_sync();
  }
}

template <bool RELU, int LN, int MODE, int XW>
__global__ __launch_bounds__(256, 1) void mlp_forward_kernel(FwdArgs p) {
  extern __shared__ __align__(16) float lds[];
  forward_body<RELU, LN, MODE, XW>(p, lds, blockIdx.x, gridDim.x);
}

// get_actions of a MultiDiscrete policy (mappo_actor_act_md): the forward above with the per-head epilogue
template <bool RELU, int LN, int XW>
__global__ __launch_bounds__(256, 1) void mlp_forward_md_kernel(FwdArgs p, MdHeads md) {
  extern __shared__ __align__(16) float lds[];
  forward_body<RELU, LN, 5, XW>(p, lds, blockIdx.x, gridDim.x, &md);
}

// Fused rollout step (K7 + K8 + K1 in ONE launch): workgroups [0, nA) run the actor's get_actions, [nA, nA + nC) the
// critic's get_values, the rest copy the env output the rows come from into the buffer slots (insert_core.h).  All
// three read only their sources and write disjoint outputs, so there is nothing to order inside the launch.
#include "insert_core.h"
struct StepArgs {
  FwdArgs a, c;
  InsertArgs ins;
  int nA, nC, nI;
};
#include "mlp_fwd16.h"
template <bool RELU, int LN>
__global__ __launch_bounds__(256, 1) void rollout_step_kernel(StepArgs s) {
  extern __shared__ __align__(16) float lds[];
  const int bid = blockIdx.x;
  if (bid < s.nA) forward16r_body<RELU, LN, 1>(s.a, lds, bid, s.nA);
  else if (bid < s.nA + s.nC) forward16r_body<RELU, LN, 0>(s.c, lds, bid - s.nA, s.nC);
  else insert_mpe_body(s.ins, bid - s.nA - s.nC, s.nI);
}

// The same step for a MultiDiscrete policy (mappo_rollout_step_md): the actor's workgroups sample every head of `md`
template <bool RELU, int LN>
__global__ __launch_bounds__(256, 1) void rollout_step_md_kernel(StepArgs s, MdHeads md) {
  extern __shared__ __align__(16) float lds[];
  const int bid = blockIdx.x;
  if (bid < s.nA) forward16r_body<RELU, LN, 5>(s.a, lds, bid, s.nA, &md);
  else if (bid < s.nA + s.nC) forward16r_body<RELU, LN, 0>(s.c, lds, bid - s.nA, s.nC);
  else insert_mpe_body(s.ins, bid - s.nA - s.nC, s.nI);
}

// One rollout episode in one launch (mappo_rollout_episode): for an env whose output for the whole episode exists before the
// episode starts (and does not depend on the actions), waves [0, wA) run the actor's get_actions of steps 0 .. T - 1, waves
// [wA, wA + wC) the critic's get_values of steps 0 .. T (step T: the bootstrap values), each network's (step, tile) items dealt
// over its waves; waves [wI0, wAll) then copy the env output of every step into the buffer slots (wI0 = 0: every wave, after its
// items; wI0 = wA + wC: waves of their own).  Rows of different threads never interact and the weights do not change: no
// inter-workgroup synchronisation.
struct EpisodeArgs {
  FwdArgs a, c;                  // a.actions / a.logp, c.out: [T][B]
  EpisodeSrc sa, sc;
  float *next_values;            // [B]: the critic at step T
  InsertArgs ins;                // the insert of step 0's env output; step t: sources + t * *_st, destinations t slots further
  int64_t ins_obs_st, ins_rew_st, ins_done_st;
  int T, M, wA, wC, wI0, wAll;
};
template <bool RELU, int LN>
__global__ __launch_bounds__(256, 1) void rollout_episode_kernel(EpisodeArgs e) {
  extern __shared__ __align__(16) float lds[];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const int gw = (int)blockIdx.x * (int)(blockDim.x / WAVE) + wave;
  float *tZ = lds + wave * 16 * TP;
  if (gw < e.wA) episode16r_body<RELU, LN, 1>(e.a, e.sa, e.M, e.T, -1, nullptr, tZ, gw, e.wA);
  else if (gw < e.wA + e.wC) episode16r_body<RELU, LN, 0>(e.c, e.sc, e.M, e.T + 1, e.T, e.next_values, tZ, gw - e.wA, e.wC);
  if (gw >= e.wI0 && gw < e.wAll) insert_mpe_episode_body<16>(e.ins, e.ins_obs_st, e.ins_rew_st, e.ins_done_st, e.T, gw - e.wI0, e.wAll - e.wI0);
}
#include "mlp_ep16l.h"             // the same episode with the weights in LDS (rollout_episode_lds_kernel: wA = the actor's workgroups)

// trunk features of a recurrent network (mappo_mlp_features, in_dim <= 64) on the same register-resident 16x16x4 path
template <bool RELU, int LN>
__global__ __launch_bounds__(256, 1) void features16_kernel(FwdArgs a) {
  extern __shared__ __align__(16) float lds[];
  forward16r_body<RELU, LN, 2>(a, lds, blockIdx.x, gridDim.x);
}
template <bool RELU, int LN>
__global__ __launch_bounds__(256, 1) void features16_dual_kernel(FwdArgs a, FwdArgs c, int nA) {
  extern __shared__ __align__(16) float lds[];
  if ((int)blockIdx.x < nA) forward16r_body<RELU, LN, 2>(a, lds, blockIdx.x, nA);
  else forward16r_body<RELU, LN, 2>(c, lds, blockIdx.x - nA, gridDim.x - nA);
}
