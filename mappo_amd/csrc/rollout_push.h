// rollout_push.h — one rollout episode on the GPU-resident `simple_push` environment in ONE launch (mappo_rollout_episode_push), for
// the SEPARATED runner: two agents (the adversary with 8 features, the good agent with 19), each with its own actor, critic,
// per-agent reward and SeparatedReplayBuffer.  It does what T x (two mappo_rollout_step + mappo_mpe_push_step + the two agents'
// inserts) + the two bootstrap launches do, ~5 T + 2 dependent launches.
//
// The two-barrier skeleton of rollout_comm.h / rollout_sep_img.h / rollout_tag.h (read their headers first): a tile is 16 whole
// environments, one workgroup of FOUR waves per tile, one per SIMD, one row per environment and agent.  Two agents are four
// networks, one per wave as in rollout_comm.h — but that kernel keeps all four in registers and steps the environments in a critic
// wave's lanes, which at tanh / layer_N 1 already costs it 112 B of scratch with an env that has no float64 exp / log1p.  This env's
// contact force does, so here only the ACTORS, the step's critical path (actor -> environment -> actor), keep their weights in
// registers; the CRITICS read theirs from LDS images, which leaves their waves' registers to the environment step:
//   wave m = 0, 1      agent m's ACTOR, weights in registers (Trunk16R / Head16R): tile16r_step MODE 1 on the agent's slice of the
//           observation tile, Philox (seed_m, counter + t (+ *counter_dev_m), row = environment), the sampled action also to the
//           action tile.  Between the two barriers it has nothing to do.
//   wave 2 + m         agent m's CRITIC, weights in an LDS image (EplMap / Trunk16L / Head16L of mlp_ep16l.h: the same 16-byte
//           operands in the same order as the register trunk, so the same bits).  It runs BESIDE the actors, in front of A_t — the
//           value of step t needs only observation tile t —, so it is off the critical path; step T writes next_values.  Behind
//           B_t, before its next critic, the wave copies agent m's rows of observation tile t + 1 into that agent's obs[t + 1] /
//           share_obs[t + 1] (what the stepwise insert writes).
//   wave 3, lanes 0 .. 15   also the environments, between the two barriers: mpe_push_step_env (mpe_push_core.h) with mode 1, the
//           state in the lane for the whole episode; each agent's OWN reward -> its rew_buf[t], 1 - done -> its mask_buf[t + 1].
// The same two workgroup barriers per step in every role (A_t: the actions of step t are in LDS, every read of observation tile t is
// in registers and every copy of it is done; B_t: observation tile t + 1 is in LDS), behind one barrier that closes the staging of
// the critic images, in which all four waves take part.  No role returns early: a wave whose rows or lanes do not exist (last
// partial tile) still walks all T steps and their barriers.
//
// LDS (floats): two critic images, EplMap<LN>::total each (11424 at layer_N 1, 6880 at 0) | the observation tile [16][27] — a row is
// the adversary's 8 features, then the good agent's 19: the centralized share row as it stands, each network reads its slice | one
// [16][TP] logits tile per wave | the action tile, one column of 16 per agent.  At layer_N 1 that is 2 x 11424 + 432 + 4 x 528 + 32
// = 25424 floats = 101696 B of 163840; at layer_N 0 16336 floats = 65344 B.  One workgroup per CU.
// Every value goes through the stepwise kernels' own code (tile16r_step, mpe_push_step_env), so the two buffers and the environment
// state end up bit-identical to the stepwise path's.
#pragma once
#include "mpe_push_core.h"
#include "rollout_comm.h"

typedef SepEpisodeArgs<MpePushArgs, MPE_PUSH_M> PushEpisodeArgs;      // agent 0: adversary, 1: good agent

#define PUSH_X_TILE (16 * MPE_PUSH_SHARE)
template <int LN>
constexpr int push_ep_lds_floats() { return MPE_PUSH_M * EplMap<LN>::total + PUSH_X_TILE + SEP_EP_WAVES * 16 * TP + MPE_PUSH_M * 16; }

template <bool RELU, int LN>
__global__ __launch_bounds__(SEP_EP_WAVES * WAVE, 1) void rollout_episode_push_kernel(PushEpisodeArgs e) {
  extern __shared__ __align__(16) float lds[];
  constexpr int IMG = EplMap<LN>::total, W = MPE_PUSH_SHARE;
  float *X = lds + MPE_PUSH_M * IMG, *tZ = X + PUSH_X_TILE, *act = tZ + SEP_EP_WAVES * 16 * TP;
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), j = lane & 15, q = lane >> 4;
  const int T = e.T;
  const int64_t B = e.env.N;                                        // rows of every buffer: one per environment
  const int n0 = (int)blockIdx.x * SEP_EP_G;                        // first environment / buffer row of this tile
  const int64_t i = (int64_t)n0 + j;
  const bool ok = i < B;
  const int jr = ok ? j : 0;
  if (wave < MPE_PUSH_M) {
    // ---- agent m's actor (registers); step 0 reads buffer slot 0, as the stepwise path does ----
    const int m = wave;
    const int D = MpePush::obs_dim(m), xo = MpePush::obs_off(m);
    FwdArgs fa;
    comm_fwd_args(fa, e.a[m], B, e.deterministic);
    f32x4 xa[4];
    spread_load_x(xa, e.obs_buf[m] + (ok ? i : 0) * D, D, q);
    Trunk16R<LN> tw;
    trunk16r_load<LN>(tw, fa.params, fa.off, fa.desc, j, q);
    Head16R<1> hd;
    head16r_load<1>(hd, fa.params, fa.off, fa.desc.out_dim, j, q);
    const uint64_t ctr0 = e.counter + (e.a[m].counter_dev ? *e.a[m].counter_dev : 0ull);      // read once: the word is fixed for the launch
#pragma unroll
    for (int k = 0; k < MPE_PUSH_M; ++k) epl_stage<LN, 1>(lds + k * IMG, e.c[k].params, e.c[k].off, e.c[k].desc);
    __syncthreads();                                                // the critic images are staged
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B;
      tile16r_step<RELU, LN, 1, false, true>(fa, tw, hd, xa, nullptr, fa.actions + so, fa.logp + so, ctr0 + (uint64_t)t, nullptr,
                                             tZ + wave * 16 * TP, i, ok, j, q, act + m * 16);
      __syncthreads();                                              // A_t
      __syncthreads();                                              // B_t
      spread_load_x(xa, X + jr * W + xo, D, q);
    }
  } else {
    // ---- agent m's critic (LDS image), its rows of the buffer's observations and, in wave 3's lanes 0 .. 15, the environments, the
    // state in the lane for the whole episode ----
    const int m = wave - MPE_PUSH_M;
    const int D = MpePush::obs_dim(m), xo = MpePush::obs_off(m);
    const bool env_wave = wave == SEP_EP_WAVES - 1;
    const int n = n0 + lane;
    const bool env_lane = env_wave && lane < SEP_EP_G && n < e.env.N;
    const int Rv = (int)(B - n0 < 16 ? B - n0 : 16);                // rows of the tile that exist (the last tile may be partial)
    FwdArgs fc;
    comm_fwd_args(fc, e.c[m], B, 0);
    const int S = fc.desc.in_dim, so_x = e.centralized ? 0 : xo;    // 27 (centralized) or D
    f32x4 xc[4];
    spread_load_x(xc, e.share_buf[m] + (ok ? i : 0) * S, S, q);
    MpePushState s = {};
    if (env_lane) mpe_push_load(e.env, n, s);
#pragma unroll
    for (int k = 0; k < MPE_PUSH_M; ++k) epl_stage<LN, 1>(lds + k * IMG, e.c[k].params, e.c[k].off, e.c[k].desc);
    __syncthreads();                                                // the critic images are staged
    const float *img = lds + m * IMG;
    const Trunk16L<LN> cw = {img + j * EPL_WS + 4 * q, img + 4 * q};
    const Head16L<LN, 0> ch = {cw.m, cw.v};
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B;
      asm volatile("" ::: "memory");        // the image is loop-invariant: keep its reads inside the step (hoisted, they are a register network)
      tile16r_step<RELU, LN, 0>(fc, cw, ch, xc, fc.out + so, nullptr, nullptr, 0ull, nullptr, tZ + wave * 16 * TP, i, ok, j, q);
      __syncthreads();                                              // A_t
      if (env_lane) {       // sep_env_step, kept inline: through the shared function the register allocation moved and a rollout took 1.5 % longer
        float reward[MPE_PUSH_M];
        float *row = X + lane * W;
        const bool done = mpe_push_step_env(e.env, n, act + lane, 16, s, row, row + MpePush::obs_off(1), reward);
#pragma unroll
        for (int k = 0; k < MPE_PUSH_M; ++k) {
          e.rew_buf[k][so + n] = reward[k];
          e.mask_buf[k][so + B + n] = done ? 0.f : 1.f;
        }
      }
      __syncthreads();                                              // B_t
      // what the stepwise insert writes into agent m's slot t + 1 (centralized: the tile's row as it stands); the next write of the
      // tile is behind A_{t + 1}, which this wave passes after the copy
      sep_copy_rows<W>(e, X, m, D, xo, so + B + n0, Rv, lane);
      spread_load_x(xc, X + jr * W + so_x, S, q);
    }
    asm volatile("" ::: "memory");
    tile16r_step<RELU, LN, 0>(fc, cw, ch, xc, e.next_values[m], nullptr, nullptr, 0ull, nullptr, tZ + wave * 16 * TP, i, ok, j, q);
    if (env_lane) mpe_push_store(e.env, n, s, true);                // the environment continues from here in either path
  }
}

template <bool RELU, int LN>
struct PushEpisode {
  static constexpr auto kernel = rollout_episode_push_kernel<RELU, LN>;
  static constexpr int lds_bytes = sizeof(float) * push_ep_lds_floats<LN>();
};

extern "C" int mappo_rollout_episode_push(const mappo_comm_agent *agents, double *agent_pos, double *agent_vel, double *landmark_pos,
                                          int32_t *goal, int32_t *tstep, int64_t *episode, int32_t T, int32_t N, int32_t env_episode_length,
                                          uint64_t env_seed, int32_t deterministic, uint64_t counter, int32_t centralized,
                                          mappo_stream_t stream) {
  const char *who = "rollout_episode_push";
  MAPPO_REQUIRE(agents, "%s: null agent descriptors (needs num_agents = 2 of them: adversary, good agent)", who);
  const char *const name[MPE_PUSH_M] = {"adversary", "good agent"};
  const int Dm[MPE_PUSH_M] = {MPE_PUSH_OBS_A, MPE_PUSH_OBS_G}, Am[MPE_PUSH_M] = {MPE_PUSH_U, MPE_PUSH_U};
  PushEpisodeArgs e;
  if (int rc = sep_episode_fill(e, who, agents, name, Dm, Am, MPE_PUSH_SHARE, centralized, deterministic, counter, T, N, env_episode_length)) return rc;
  MAPPO_REQUIRE(agent_pos && agent_vel && landmark_pos && goal && tstep && episode, "%s: bad arguments (null state pointer)", who);
  MAPPO_CLEAR_STICKY();
  e.env.apos = agent_pos; e.env.avel = agent_vel; e.env.lpos = landmark_pos; e.env.goal = goal; e.env.tstep = tstep; e.env.episode = episode;
  e.env.N = N; e.env.T = env_episode_length; e.env.mode = 1; e.env.seed = env_seed;
  return sep_episode_launch<PushEpisode>(who, N, agents[0], e, stream);
}
