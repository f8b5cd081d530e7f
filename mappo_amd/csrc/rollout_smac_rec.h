// rollout_smac_rec.h — one rollout episode of a RECURRENT shared policy on SMAC-shaped env output in ONE launch
// (mappo_rollout_episode_smac_recurrent): per step the actor (trunk, GRU step, rnn.norm, head, available_actions mask, sampling),
// the critic (trunk, GRU step, value) and the SMAC insert of the env output (smac_runner.py:129-151).  The stepwise path is
// mappo_recurrent_step_dual on slot 0, then T - 1 x mappo_recurrent_rollout_step, then mappo_insert_smac into slot T: T + 1 dependent
// launches, T of which reload every weight.  The env output of the whole episode is an INPUT (the pool of mappo_synth_smac_pool: the
// synthetic SMAC env ignores the actions), so there is no env role: this is rollout_spread_rec.h without the float64 physics, plus
// available_actions and the SMAC mask rules.  The bootstrap value of slot T is NOT computed here: the runner's compute() takes it.
//
// Ownership: a workgroup owns G = floor(16 / M) whole environments = G M consecutive buffer rows of one 16-row tile — whole
// environments, so that dones_env = all_m dones[n][m] is local to the tile — and walks all T steps alone.  Its eight waves are the
// two 4-wave groups of gru_step3_tiles (waves 0..3 the actor, 4..7 the critic; source Step3Src::Episode), so each value is the one the
// stepwise launches compute for the row: same MFMA sequence, same LayerNorm exchange, same order of the partial logits, same
// categorical_act_mask call keyed by (seed, counter + k, buffer row).
//   * Registers: the GRU slices of a wave (96 VGPRs) for the episode; both trunks once into LDS (the EplMap image of mlp_ep16l.h
//     without the head, read through Trunk16L).  Eight waves = two per SIMD = 256 VGPRs each.  With up to 32 actions (a second
//     head block) the tanh instantiations spilled, so the biases, rnn.norm vectors and head rows (40 VGPRs, idle while the trunk
//     runs) wait in LDS and come back behind the trunk (Step3EpSmac::fill): no scratch in any of the four instantiations.
//   * Per step k: the tile's piece of env output k (contiguous: Rv D obs floats, Rv S share floats, Rv A avail floats, at most
//     4 + 2 floats per lane) is requested BEFORE the step and stored behind it, so its latency hides under the networks.  The
//     actor's waves carry obs and avail, the critic's the share rows; lanes 0..15 of the critic's first wave carry the row's done
//     byte and reward and derive masks / active_masks / bad_masks.
//   * LDS: both trunk images, the actor's and the critic's input tile and the rows' available_actions (rows of slot k; step k + 1
//     reads what the insert of step k put there, not the buffer; input rows SMREC_XS floats apart, so that the 16 rows one
//     quarter of a wave gathers lie 4 banks apart at every width, 64 included), per network the hidden state [2][16][68] (step k reads half k & 1 and writes the unmasked new state
//     into the other half; the next step multiplies by the mask, as the step kernel does with the state it is handed), masks, done
//     flags and actions of the tile.
//   * Barriers per step: the four of gru_step3_tiles, passed by both networks together — its last one is A_k (every read of input
//     tile k and of mask k is done) — and B_k (input tile k + 1 and mask k + 1 are in LDS).  No wave returns early; the idle lanes
//     of a partial tile pass every barrier.
#pragma once
#include "rollout_rec_frame.h"

#define SMREC_XS 68                                                 // row stride of the LDS input tiles (rows 4 banks apart)
#define SMREC_MAX_M 16

template <int LN>
struct Step3EpSmac : Step3EpFrame<LN> {
  static constexpr int HEAD_BLOCKS = 2;                             // up to MAPPO_MAX_ACTIONS actions
  // The biases, rnn.norm vectors and head rows of a wave (40 VGPRs) are not needed while the trunk runs, where the register
  // pressure peaks (the tanh trunk by itself takes what rollout_spread_rec.h has left): they wait in LDS and come back behind the
  // trunk, every step.  The vectors depend on (wave, q) only, the head rows on the lane.
  const g4_t *vs;                  // [8] bir biz bin bhr bhz bhn nw4 nb4 of this lane's (wave, q)
  const g4_t *hws;                 // [2][WAVE] + lane: this lane's head rows
  __device__ __forceinline__ void late() const {}                  // the GRU slices stay in registers
  // gru_step3_tiles hands over its own locals, behind the trunk
  __device__ __forceinline__ void fill(g4_t &bir, g4_t &biz, g4_t &bin, g4_t &bhr, g4_t &bhz, g4_t &bhn, g4_t &nw4, g4_t &nb4, g4_t (&hw)[2]) const {
    bir = vs[0]; biz = vs[1]; bin = vs[2]; bhr = vs[3]; bhz = vs[4]; bhn = vs[5]; nw4 = vs[6]; nb4 = vs[7];
    hw[0] = hws[0]; hw[1] = hws[WAVE];
  }
  const float *avail;              // [16][A] available_actions of the tile rows for this step (LDS), or NULL
};

struct SmacRecArgs {
  GruFwdArgs a, c;                 // a.actions / a.logp, c.out: [T][B]
  const float *e_obs, *e_share;    // env output [T][B][D], [T][B][S] (e_share = e_obs when the critic is not centralized)
  const float *e_avail, *e_rew;    // [T][B][A] or NULL, [T][N]
  const uint8_t *e_done, *e_bad;   // [T][B] bool bytes, [B] bool bytes or NULL
  float *obs_buf, *share_buf, *avail_buf;       // [T + 1][B][D | S | A]
  float *rew_buf;                               // [T][B]
  float *mask_buf, *bad_buf, *active_buf;       // [T + 1][B]
  float *rnn_a, *rnn_c;                         // [T + 1][B][64]
  int T, N, M, G;
};

template <int LN>
struct SmrecLds {
  static constexpr int IMG = EplMap<LN>::wh;                        // the trunk's part of the image
  static constexpr int imgA = 0, imgC = IMG, XA = 2 * IMG, XC = XA + 16 * SMREC_XS, hsA = XC + 16 * SMREC_XS, hsC = hsA + 2 * 16 * REC_HS,
                       mk = hsC + 2 * 16 * REC_HS, act = mk + 16, dn = act + 16, av = dn + 16, vst = av + 16 * MAPPO_MAX_ACTIONS, hst = vst + REC_WAVES * 4 * 8 * 4,
                       total = hst + REC_WAVES * 2 * WAVE * 4;
};

// one network's four waves over the whole episode
template <int HM, bool RELU, int LN>
__device__ __forceinline__ void smac_rec_role(const SmacRecArgs &e, const GruFwdArgs &p, Step3Shared &sh, float *lds, float *rnn, const int w) {
  typedef SmrecLds<LN> Ld;
  const int M = e.M, G = e.G, T = e.T;
  const int Dn = p.desc.in_dim;                                     // the input width of THIS network (actor: D, critic: S)
  const int A = e.a.A;
  const int64_t B = (int64_t)e.N * M;
  Step3W<LN> W;
  Step3EpSmac<LN> ep;
  const RecRole r = rec_role_begin<HM, Ld>(p, lds, B, G, M, w, W, ep);
  const int lane = r.lane, n = r.n, q = r.q, i0 = r.i0, Rv = r.Rv;
  const bool ok = r.ok;
  float *X = lds + (HM == 2 ? Ld::XA : Ld::XC), *mk = r.mk, *dn = lds + Ld::dn, *AV = lds + Ld::av;
  {
    const int gw = HM == 2 ? w : w + 4;                             // this wave among the workgroup's eight
    g4_t *vs = reinterpret_cast<g4_t *>(lds + Ld::vst) + (gw * 4 + q) * 8, *hws = reinterpret_cast<g4_t *>(lds + Ld::hst) + gw * 2 * WAVE + lane;
    if (n == 0) { vs[0] = W.bir; vs[1] = W.biz; vs[2] = W.bin; vs[3] = W.bhr; vs[4] = W.bhz; vs[5] = W.bhn; vs[6] = W.nw4; vs[7] = W.nb4; }
    hws[0] = W.hw[0]; hws[WAVE] = W.hw[1];
    ep.vs = vs; ep.hws = hws;
  }
  ep.xrow = X + r.jr * SMREC_XS;
  ep.avail = (HM == 2 && e.e_avail) ? AV : nullptr;                 // the rows' available_actions of the step: slot 0, then what the insert put there
  const int gt = w * WAVE + lane;                                   // this lane among the 256 of its network
  const bool flag_lane = HM == 1 && w == 0 && lane < 16 && ok;      // the lanes that derive the masks of row i0 + n
  const bool bad = flag_lane && e.e_bad && e.e_bad[i0 + n] != 0;    // constant over the episode, as the env returns it
  const float *src = HM == 2 ? e.e_obs : e.e_share;
  float *dst = HM == 2 ? e.obs_buf : e.share_buf;
  __syncthreads();                                                  // the prologue's LDS writes (images, slot 0 rows, states, masks)
  for (int k = 0; k < T; ++k) {
    asm volatile("" ::: "memory");          // the trunk image is loop-invariant: keep its reads inside the step (episode16l_body)
    const int64_t so = (int64_t)k * B;
    // ---- env output k, this tile's piece: requested here, stored behind the step ----
    float xv[4], av[2] = {0.f, 0.f}, rw = 0.f;
    uint8_t dbyte = 0;
    {
      const float *xs = src + (so + i0) * Dn;
#pragma unroll
      for (int j = 0; j < 4; ++j) { const int idx = gt + 256 * j; xv[j] = idx < Rv * Dn ? xs[idx] : 0.f; }
      if (HM == 2 && e.e_avail) {
        const float *as = e.e_avail + (so + i0) * A;
#pragma unroll
        for (int j = 0; j < 2; ++j) { const int idx = gt + 256 * j; av[j] = idx < Rv * A ? as[idx] : 0.f; }
      }
      if (flag_lane) { dbyte = e.e_done[so + i0 + n]; rw = e.e_rew[(int64_t)k * e.N + (i0 + n) / M]; }
    }
    rec_step_begin(ep, r, k, so);
    g4_t h;
    gru_step3_tiles<HM, Step3Src::Episode, RELU, LN>(W, p, sh, 0, 1, nullptr, &ep, &h);      // its last barrier is A_k
    // ---- what insert_smac_body writes into slot k + 1 (rewards: slot k); the input tiles and the mask of step k + 1 -> LDS ----
    {
      float *xd = dst + (so + B + i0) * Dn;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int idx = gt + 256 * j, row = idx / Dn;
        if (idx < Rv * Dn) { X[row * SMREC_XS + (idx - row * Dn)] = xv[j]; xd[idx] = xv[j]; }
      }
      if (HM == 2 && e.e_avail) {
        float *ad = e.avail_buf + (so + B + i0) * A;
#pragma unroll
        for (int j = 0; j < 2; ++j) { const int idx = gt + 256 * j; if (idx < Rv * A) { AV[idx] = av[j]; ad[idx] = av[j]; } }
      }
      if (HM == 1 && w == 0) {
        if (flag_lane) dn[n] = dbyte != 0 ? 1.f : 0.f;
        wave_lds_sync();
        if (flag_lane) {
          const int r0 = (n / M) * M;                               // the first row of this row's environment
          bool all = true;
          for (int m = 0; m < M; ++m) all = all && dn[r0 + m] != 0.f;
          const int64_t r = so + B + i0 + n;
          e.rew_buf[so + i0 + n] = rw;
          e.mask_buf[r] = all ? 0.f : 1.f;
          e.active_buf[r] = all ? 1.f : (dbyte != 0 ? 0.f : 1.f);
          e.bad_buf[r] = bad ? 0.f : 1.f;
          mk[n] = all ? 0.f : 1.f;
        }
      }
    }
    __syncthreads();                                                // B_k
    rec_store_state(rnn, h, r, lane, so + B + i0, w);
  }
}

template <bool RELU, int LN>
__global__ __launch_bounds__(REC_WAVES * WAVE, 1) void rollout_episode_smac_rec_kernel(SmacRecArgs e) {
  typedef SmrecLds<LN> Ld;
  extern __shared__ __align__(16) float lds[];
  __shared__ Step3Shared sh[2];
  const int tid = threadIdx.x, nt = REC_WAVES * WAVE;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  {
    const int M = e.M, D = e.a.desc.in_dim, S = e.c.desc.in_dim;
    const int64_t B = (int64_t)e.N * M;
    const int i0 = (int)blockIdx.x * e.G * M;
    const int Rv = (int)(B - i0 < e.G * M ? B - i0 : e.G * M);
    rec_stage<LN, Ld>(lds, e.a, e.c, e.rnn_a, e.rnn_c, e.mask_buf, i0, Rv);
    for (int k = tid; k < 16 * SMREC_XS; k += nt) {                 // the input tiles: rows SMREC_XS apart
      const int row = k / SMREC_XS, col = k - row * SMREC_XS;
      lds[Ld::XA + k] = (row < Rv && col < D) ? e.obs_buf[(int64_t)(i0 + row) * D + col] : 0.f;
      lds[Ld::XC + k] = (row < Rv && col < S) ? e.share_buf[(int64_t)(i0 + row) * S + col] : 0.f;
    }
    if (e.e_avail) {
      const int A = e.a.A;
      for (int k = tid; k < 16 * MAPPO_MAX_ACTIONS; k += nt) lds[Ld::av + k] = k < Rv * A ? e.avail_buf[(int64_t)i0 * A + k] : 1.f;
    }
    if (tid < 16) lds[Ld::dn + tid] = 0.f;
  }
  if (wave < 4) smac_rec_role<2, RELU, LN>(e, e.a, sh[0], lds, e.rnn_a, wave);
  else smac_rec_role<1, RELU, LN>(e, e.c, sh[1], lds, e.rnn_c, wave - 4);
}

extern "C" int mappo_rollout_episode_smac_recurrent(const float *actor_params, const mappo_net_desc *actor_desc, const float *critic_params,
                                                    const mappo_net_desc *critic_desc, int32_t T, int32_t N, int32_t M, const float *env_obs,
                                                    const float *env_share_obs, const float *env_avail, const float *env_rewards,
                                                    const uint8_t *env_dones, const uint8_t *env_bad_transition, int32_t deterministic,
                                                    uint64_t seed, uint64_t counter, const uint64_t *counter_dev, float *obs_buf,
                                                    float *share_buf, float *avail_buf, float *rew_buf, float *mask_buf, float *bad_mask_buf,
                                                    float *active_mask_buf, float *rnn_states, float *rnn_states_critic, float *actions,
                                                    float *logp, float *values, int32_t centralized, mappo_stream_t stream) {
  const char *who = "rollout_episode_smac_recurrent";
  if (int rc = rec_episode_check(actor_desc, critic_desc, N, M, who)) return rc;
  MAPPO_REQUIRE(M >= 1 && M <= SMREC_MAX_M, "%s: M=%d out of range (1 .. %d agents: a 16-row tile holds whole environments)", who, M,
                SMREC_MAX_M);
  MAPPO_REQUIRE(T >= 1 && N >= 1, "%s: bad shape T=%d N=%d", who, T, N);
  if (!centralized)
    MAPPO_REQUIRE(critic_desc->in_dim == actor_desc->in_dim, "%s: critic in_dim %d != actor in_dim %d (not centralized: the critic reads obs)",
                  who, critic_desc->in_dim, actor_desc->in_dim);
  MAPPO_REQUIRE(actor_params && critic_params && env_obs && (env_share_obs || !centralized) && env_rewards && env_dones && obs_buf && share_buf &&
                rew_buf && mask_buf && bad_mask_buf && active_mask_buf && rnn_states && rnn_states_critic && actions && logp && values,
                "%s: bad arguments (null pointer)", who);
  MAPPO_REQUIRE((env_avail != nullptr) == (avail_buf != nullptr), "%s: the env's avail and the buffer's available_actions go together (both or "
                "neither NULL)", who);
  MAPPO_CLEAR_STICKY();
  SmacRecArgs e = {};
  rec_episode_args(e.a, e.c, actor_params, actor_desc, critic_params, critic_desc, N * M, deterministic, seed, counter, counter_dev, actions, logp,
                   values);
  e.e_obs = env_obs; e.e_share = centralized ? env_share_obs : env_obs; e.e_avail = env_avail; e.e_rew = env_rewards; e.e_done = env_dones;
  e.e_bad = env_bad_transition;
  e.obs_buf = obs_buf; e.share_buf = share_buf; e.avail_buf = avail_buf; e.rew_buf = rew_buf; e.mask_buf = mask_buf; e.bad_buf = bad_mask_buf;
  e.active_buf = active_mask_buf; e.rnn_a = rnn_states; e.rnn_c = rnn_states_critic;
  e.T = T; e.N = N; e.M = M; e.G = 16 / M;
  const dim3 grid((unsigned)((N + e.G - 1) / e.G)), block(REC_WAVES * WAVE);
  if (int rc = dispatch_relu_ln<1>(actor_desc->use_relu != 0, actor_desc->layer_N, [&](auto R, auto L) {
        return launch_kernel<rollout_episode_smac_rec_kernel<R.value, L.value>, REC_LDS_MAX>(who, grid, block, sizeof(float) * SmrecLds<L.value>::total, as_stream(stream), e);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}
