// rollout_spread_rec.h — one rollout episode of a RECURRENT shared policy on the GPU-resident `simple_spread` environment in ONE
// launch (mappo_rollout_episode_spread_recurrent): per step the actor (trunk, GRU step, rnn.norm, head, sampling), the environment
// step, the critic (trunk, GRU step, value) and every buffer write.  The stepwise path is T x (mappo_recurrent_step_dual +
// mappo_mpe_spread_step + mappo_insert_mpe_rnn), 3 T dependent launches that each reload every weight.  The bootstrap value of
// slot T is NOT computed here: the runner's compute() takes it through its own kernels afterwards.
//
// Ownership is rollout_spread.h's: a workgroup owns G = floor(16 / M) whole environments = G M consecutive buffer rows of one
// 16-row tile and walks all T steps alone.  Its eight waves are the two 4-wave groups of gru_step3_tiles — waves 0..3 the actor,
// 4..7 the critic, wave w of a group owning hidden units [16 w, 16 w + 16) — and every row goes through that function (source
// Step3Src::Episode), so each value is the one mappo_recurrent_step_dual computes for the row: same MFMA sequence, same LayerNorm exchange,
// same order of the partial logits, same categorical_act_mask call keyed by the buffer row.
//   * Registers: the GRU slices, biases and head rows of a wave (Step3W, ~136 VGPRs) stay in registers for the episode; the trunk
//     (another ~180 at layer_N 1) does not fit beside them, so both trunks are staged once into LDS (the EplMap image of
//     mlp_ep16l.h without the head) and trunk16r_apply reads its operands from there (Trunk16L).  Eight waves = two per SIMD = 256
//     VGPRs each; a ninth (environment) wave would put three on one SIMD and cap all of them at 168, so the environments step in
//     lanes 0 .. G - 1 of the critic's last wave, between the two barriers where the networks have nothing to do anyway.  That
//     wave is a role of its own, built so that the float64 step and the GRU step never hold registers at the same time: the
//     environments' state stays in LDS for the episode (mpe_step_env reads and writes it in place; loaded before step 0, stored
//     after step T - 1), the wave's GRU slices (96 VGPRs) wait in LDS and are fetched behind the trunk (Step3Ep::late), its
//     biases and head rows at the top of the step.  No role spills: no scratch in any of the four instantiations.
//   * LDS: observation tile (written by the env lanes, read by both trunks, copied to obs / share_obs[t + 1]), the share rows of
//     slot 0, masks and actions of the tile, and per network the hidden state [2][16][68]: step t reads half t & 1 and writes the
//     new state (before the mask) into the other half; the next step multiplies by the mask, as the step kernel does with the
//     stored state.  The buffer gets h * (1 - done) (mappo_insert_mpe_rnn) once the env lanes have published the mask.
//   * Barriers per step: the four of gru_step3_tiles, passed by both networks together — its last one is A_t (actions of step t
//     are in LDS, every read of observation tile t is done) — and B_t (observation tile t + 1 and masks[t + 1] are in LDS).
#pragma once
#include "mpe_core.h"
#include "rollout_rec_frame.h"

#define SREC_ES (4 * MPE_MAX_M + 2 * MPE_MAX_L + 1)                 // doubles of one env lane's state row (agent_pos | agent_vel | landmark_pos, odd stride)

template <int LN, bool LATE>
struct Step3Ep : Step3EpFrame<LN> {
  static constexpr int HEAD_BLOCKS = 1;                             // the entry point takes 5 actions: no second head block
  static constexpr const float *avail = nullptr;                    // simple_spread has no available_actions
  // LATE (the env wave): the GRU slices are fetched from their LDS copy behind the trunk, so that they are live only from the
  // GRU products to the end of the tile function — not beside the trunk's temporaries, and not while the environments step
  Step3W<LN> *Wl;
  const g4_t *stash;               // [24][WAVE] + lane
  __device__ __forceinline__ void late() const {
    if constexpr (LATE) {
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int b = 0; b < 4; ++b) { Wl->wi[g][b] = stash[(8 * g + 2 * b) * WAVE]; Wl->wh[g][b] = stash[(8 * g + 2 * b + 1) * WAVE]; }
    }
  }
  __device__ __forceinline__ void fill(g4_t &, g4_t &, g4_t &, g4_t &, g4_t &, g4_t &, g4_t &, g4_t &, g4_t (&)[2]) const {}    // biases, head rows: the Step3W given
};

struct SpreadRecArgs {
  GruFwdArgs a, c;                 // a.actions / a.logp, c.out: [T][B]
  MpeArgs env;                     // state arrays, N, M, L, T = the ENV's episode length, mode 1, seed
  float *obs_buf, *share_buf;      // [T + 1][B][D], [T + 1][B][S]
  float *rew_buf, *mask_buf;       // [T][B], [T + 1][B]
  float *rnn_a, *rnn_c;            // [T + 1][B][64]
  int T, G, centralized;
};

template <int LN>
struct SrecLds {
  static constexpr int IMG = EplMap<LN>::wh;                        // the trunk's part of the image
  static constexpr int imgA = 0, imgC = IMG, X = 2 * IMG, X0 = X + 16 * MAXD, hsA = X0 + 16 * MAXD, hsC = hsA + 2 * 16 * REC_HS,
                       mk = hsC + 2 * 16 * REC_HS, act = mk + 16, stash = act + 16, envs = stash + 34 * 4 * WAVE,
                       total = envs + 16 * 2 * SREC_ES;
};

// one network's four waves over the whole episode; ENV: this group's last wave also steps the environments
template <int HM, bool RELU, int LN, bool ENV>
__device__ __forceinline__ void spread_rec_role(const SpreadRecArgs &e, const GruFwdArgs &p, Step3Shared &sh, float *lds, float *rnn,
                                                const int w) {
  typedef SrecLds<LN> Ld;
  const int M = e.env.M, G = e.G, T = e.T;
  const int D = e.a.desc.in_dim, S = e.c.desc.in_dim;
  const int64_t B = (int64_t)e.env.N * M;
  Step3W<LN> W;
  Step3Ep<LN, ENV> ep;
  const RecRole r = rec_role_begin<HM, Ld>(p, lds, B, G, M, w, W, ep);
  const int lane = r.lane, n0 = (int)blockIdx.x * G, i0 = r.i0, Rv = r.Rv, jr = r.jr;
  float *X = lds + Ld::X, *mk = r.mk, *act = r.act;
  ep.Wl = &W; ep.stash = reinterpret_cast<const g4_t *>(lds + Ld::stash) + lane;
  // The env wave (ENV: a role of its own, the critic's wave 3) keeps its operands in LDS as well: biases and head rows come back
  // at the top of every step, the GRU slices behind the trunk (Step3Ep::late) — all dead while the environments step.
  g4_t *stash = reinterpret_cast<g4_t *>(lds + Ld::stash) + lane;
  if (ENV) {
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int b = 0; b < 4; ++b) { stash[(8 * g + 2 * b) * WAVE] = W.wi[g][b]; stash[(8 * g + 2 * b + 1) * WAVE] = W.wh[g][b]; }
    const g4_t v[10] = {W.bir, W.biz, W.bin, W.bhr, W.bhz, W.bhn, W.nw4, W.nb4, W.hw[0], W.hw[1]};
#pragma unroll
    for (int k = 0; k < 10; ++k) stash[(24 + k) * WAVE] = v[k];
  }
  // the environments' float64 state: LDS for the whole episode (one row of SREC_ES doubles per env lane), read and written in
  // place by mpe_step_env — the values and their order are those of the per-step load / store of mappo_mpe_spread_step
  int32_t env_tstep = 0;
  int64_t env_episode = 0;
  const bool env_lane = ENV && lane < G && n0 + lane < e.env.N;
  if (env_lane) {
    double *es = reinterpret_cast<double *>(lds + Ld::envs) + lane * SREC_ES;
    mpe_load(e.env, n0 + lane, *reinterpret_cast<double (*)[MPE_MAX_M][2]>(es), *reinterpret_cast<double (*)[MPE_MAX_M][2]>(es + 2 * MPE_MAX_M),
             *reinterpret_cast<double (*)[MPE_MAX_L][2]>(es + 4 * MPE_MAX_M));
    env_tstep = e.env.tstep[n0 + lane];
    env_episode = e.env.episode[n0 + lane];
  }
  __syncthreads();                                                 // the prologue's LDS writes (images, slot 0 rows, states, masks)
  for (int t = 0; t < T; ++t) {
    asm volatile("" ::: "memory");          // the trunk image is loop-invariant: keep its reads inside the step (episode16l_body)
    if (ENV) {
      W.bir = stash[24 * WAVE]; W.biz = stash[25 * WAVE]; W.bin = stash[26 * WAVE]; W.bhr = stash[27 * WAVE]; W.bhz = stash[28 * WAVE];
      W.bhn = stash[29 * WAVE]; W.nw4 = stash[30 * WAVE]; W.nb4 = stash[31 * WAVE]; W.hw[0] = stash[32 * WAVE]; W.hw[1] = stash[33 * WAVE];
    }
    const int64_t so = (int64_t)t * B;
    if (HM == 2) ep.xrow = X + jr * D;
    else ep.xrow = t == 0 ? lds + Ld::X0 + jr * S : X + (e.centralized ? (jr / M) * S : jr * D);
    rec_step_begin(ep, r, t, so);
    g4_t h;
    gru_step3_tiles<HM, Step3Src::Episode, RELU, LN>(W, p, sh, 0, 1, nullptr, &ep, &h);      // its last barrier is A_t
    if (ENV) {
      // ---- environments: one lane each; obs -> the tile (rows lane M ..), rewards -> slot t, masks -> slot t + 1 and LDS ----
      int el = lane;
      asm volatile("" : "+v"(el));          // the env lane's addresses are made here, every step: hoisted, they would sit in registers through the networks' part
      const int nn = n0 + el;
      if (el < G && nn < e.env.N) {
        double *es = reinterpret_cast<double *>(lds + Ld::envs) + el * SREC_ES;
        const bool done = mpe_step_env(e.env, nn, act + el * M, *reinterpret_cast<double (*)[MPE_MAX_M][2]>(es),
                                       *reinterpret_cast<double (*)[MPE_MAX_M][2]>(es + 2 * MPE_MAX_M),
                                       *reinterpret_cast<double (*)[MPE_MAX_L][2]>(es + 4 * MPE_MAX_M), env_tstep, env_episode,
                                       X + el * M * D, e.rew_buf + so + (int64_t)nn * M, nullptr, e.mask_buf + so + B + (int64_t)nn * M);
        for (int m = 0; m < M; ++m) mk[el * M + m] = done ? 0.f : 1.f;
      }
    }
    __syncthreads();                                                // B_t
    // ---- what insert_mpe_rnn writes into slot t + 1: states * (1 - done), the observation tile, the share rows ----
    int sl = lane;
    asm volatile("" : "+v"(sl));            // the store addresses are made here, every step: hoisted, they sit in registers through the tile function
    rec_store_state(rnn, h, r, sl, so + B + i0, w);
    const int k0 = w * WAVE + sl;
    if (HM == 2) {
      float *od = e.obs_buf + (so + B + i0) * D;
      for (int k = k0; k < Rv * D; k += 4 * WAVE) od[k] = X[k];
    } else {
      float *sd = e.share_buf + (so + B + i0) * S;
      if (e.centralized) {      // the environment's M rows side by side, once per agent
        for (int k = k0; k < Rv * S; k += 4 * WAVE) { const int row = k / S; sd[k] = X[(row / M) * S + (k - row * S)]; }
      } else {
        for (int k = k0; k < Rv * S; k += 4 * WAVE) sd[k] = X[k];
      }
    }
  }
  if (env_lane) {           // the environment continues from here in either path
    double *es = reinterpret_cast<double *>(lds + Ld::envs) + lane * SREC_ES;
    mpe_store(e.env, n0 + lane, *reinterpret_cast<double (*)[MPE_MAX_M][2]>(es), *reinterpret_cast<double (*)[MPE_MAX_M][2]>(es + 2 * MPE_MAX_M),
              *reinterpret_cast<double (*)[MPE_MAX_L][2]>(es + 4 * MPE_MAX_M), true);
    e.env.tstep[n0 + lane] = env_tstep;
    e.env.episode[n0 + lane] = env_episode;
  }
}

template <bool RELU, int LN>
__global__ __launch_bounds__(REC_WAVES * WAVE, 1) void rollout_episode_spread_rec_kernel(SpreadRecArgs e) {
  typedef SrecLds<LN> Ld;
  extern __shared__ __align__(16) float lds[];
  __shared__ Step3Shared sh[2];
  const int tid = threadIdx.x, nt = REC_WAVES * WAVE;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  {
    const int M = e.env.M, D = e.a.desc.in_dim, S = e.c.desc.in_dim;
    const int64_t B = (int64_t)e.env.N * M;
    const int i0 = (int)blockIdx.x * e.G * M;
    const int Rv = (int)(B - i0 < e.G * M ? B - i0 : e.G * M);
    rec_stage<LN, Ld>(lds, e.a, e.c, e.rnn_a, e.rnn_c, e.mask_buf, i0, Rv);
    for (int k = tid; k < 16 * MAXD; k += nt) {                     // the input tiles: rows packed D | S apart
      lds[Ld::X + k] = k < Rv * D ? e.obs_buf[(int64_t)i0 * D + k] : 0.f;
      lds[Ld::X0 + k] = k < Rv * S ? e.share_buf[(int64_t)i0 * S + k] : 0.f;
    }
  }
  if (wave < 4) spread_rec_role<2, RELU, LN, false>(e, e.a, sh[0], lds, e.rnn_a, wave);
  else if (wave < 7) spread_rec_role<1, RELU, LN, false>(e, e.c, sh[1], lds, e.rnn_c, wave - 4);
  else spread_rec_role<1, RELU, LN, true>(e, e.c, sh[1], lds, e.rnn_c, 3);
}

extern "C" int mappo_rollout_episode_spread_recurrent(const float *actor_params, const mappo_net_desc *actor_desc, const float *critic_params,
                                                      const mappo_net_desc *critic_desc, int32_t T, int32_t N, int32_t M, int32_t L,
                                                      int32_t env_episode_length, uint64_t env_seed, double *agent_pos, double *agent_vel,
                                                      double *landmark_pos, int32_t *tstep, int64_t *episode, int32_t deterministic,
                                                      uint64_t seed, uint64_t counter, const uint64_t *counter_dev, float *obs_buf,
                                                      float *share_buf, float *rew_buf, float *mask_buf, float *actions, float *logp,
                                                      float *values, float *rnn_states, float *rnn_states_critic, int32_t centralized,
                                                      mappo_stream_t stream) {
  const char *who = "rollout_episode_spread_recurrent";
  if (int rc = rec_episode_check(actor_desc, critic_desc, N, M, who)) return rc;
  MAPPO_REQUIRE(actor_desc->out_dim == 5, "%s: actor out_dim %d: simple_spread has 5 actions (Discrete(5))", who, actor_desc->out_dim);
  MAPPO_REQUIRE(T >= 1 && N >= 1 && env_episode_length >= 1, "%s: bad shape T=%d N=%d env episode length %d", who, T, N, env_episode_length);
  MAPPO_REQUIRE(M >= 1 && M <= MPE_MAX_M && L >= 1 && L <= MPE_MAX_L, "%s: M=%d L=%d out of range (1 .. %d)", who, M, L, MPE_MAX_M);
  const int D = 4 + 2 * L + 4 * (M - 1);
  MAPPO_REQUIRE(actor_desc->in_dim == D, "%s: actor in_dim %d: simple_spread with M=%d L=%d has %d observation features", who,
                actor_desc->in_dim, M, L, D);
  if (centralized)
    MAPPO_REQUIRE(critic_desc->in_dim == M * D, "%s: centralized critic needs in_dim M*D = %d (got %d)", who, M * D, critic_desc->in_dim);
  else
    MAPPO_REQUIRE(critic_desc->in_dim == D, "%s: critic in_dim %d != actor in_dim %d", who, critic_desc->in_dim, D);
  MAPPO_REQUIRE(actor_params && critic_params && agent_pos && agent_vel && landmark_pos && tstep && episode && obs_buf && share_buf && rew_buf &&
                mask_buf && actions && logp && values && rnn_states && rnn_states_critic, "%s: bad arguments (null pointer)", who);
  MAPPO_CLEAR_STICKY();
  SpreadRecArgs e = {};
  rec_episode_args(e.a, e.c, actor_params, actor_desc, critic_params, critic_desc, N * M, deterministic, seed, counter, counter_dev, actions, logp,
                   values);
  e.env.apos = agent_pos; e.env.avel = agent_vel; e.env.lpos = landmark_pos; e.env.tstep = tstep; e.env.episode = episode;
  e.env.N = N; e.env.M = M; e.env.L = L; e.env.T = env_episode_length; e.env.mode = 1; e.env.seed = env_seed;
  e.obs_buf = obs_buf; e.share_buf = share_buf; e.rew_buf = rew_buf; e.mask_buf = mask_buf; e.rnn_a = rnn_states; e.rnn_c = rnn_states_critic;
  e.T = T; e.G = 16 / M; e.centralized = centralized;
  const dim3 grid((unsigned)((N + e.G - 1) / e.G)), block(REC_WAVES * WAVE);
  if (int rc = dispatch_relu_ln<1>(actor_desc->use_relu != 0, actor_desc->layer_N, [&](auto R, auto L) {
        return launch_kernel<rollout_episode_spread_rec_kernel<R.value, L.value>, REC_LDS_MAX>(who, grid, block, sizeof(float) * SrecLds<L.value>::total, as_stream(stream), e);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}
