// rollout_comm.h — one rollout episode on the GPU-resident `simple_speaker_listener` environment in ONE launch
// (mappo_rollout_episode_comm), for the SEPARATED runner: two agents of different shapes, each with its own actor, critic and
// SeparatedReplayBuffer.  It does what T x (two mappo_rollout_step + mappo_mpe_comm_step + the two agents' inserts) + the two
// bootstrap launches do, ~5 T + 2 dependent launches.
//
// The role skeleton of rollout_spread.h / rollout_reference.h (read their headers first), with one row per environment and agent: a
// tile is 16 whole environments, one workgroup of FOUR waves per tile, one per SIMD —
//   wave 0  speaker actor   (in 3, out 3)      tile16r_step MODE 1, Philox (seed_0, counter + t (+ *counter_dev_0), row = environment)
//   wave 1  listener actor  (in 11, out 5)     the same with seed_1 and counter_dev_1: each agent samples from its own stream and
//           advances its own counter word, as the stepwise path does
//   wave 2  speaker critic,  wave 3  listener critic: steps 0 .. T; they also copy the observation tile of step t >= 1 into their
//           agent's obs[t] / share_obs[t] (what the stepwise insert writes)
//   the environments are lanes 0 .. 15 of wave 2: mpe_comm_step_env (mpe_comm_core.h) with mode 1 between the two barriers of a step,
//           the state in the lane for the whole episode; rewards[t] and masks[t + 1] of BOTH buffers come from here
// and the same two workgroup barriers per step in every role (A_t: the actions of step t are in LDS and every read of observation
// tile t is done; B_t: observation tile t + 1 is in LDS).  No role returns early: a wave whose rows or lanes do not exist (last
// partial tile) still walks all T steps and their 2 T barriers.
// Why the environments have no wave of their own, as they have in the two kernels above: a fifth wave shares a SIMD with another, which
// halves the register budget of EVERY wave (256), and the networks live in registers — at layer_N 1 the compiler then spilled 319
// VGPRs to scratch.  Between A_t and B_t a critic wave has nothing to do (its forward of step t runs beside the actors'), so the
// environment step sits there at no cost to the step's critical path (actor -> environment -> actor), with one wave per SIMD.
//
// LDS: the observation tile [16][14] — a row is the speaker's 3 features followed by the listener's 11, i.e. the centralized share
// row as it stands, and each actor reads its slice; one [16][TP] logits tile per actor wave; the action tile, one column of 16 per
// agent (tile16r_step's ACT_TILE writes act_tile[j], so a column per agent keeps that function as it is).
// Every value goes through the stepwise kernels' own code (tile16r_step, mpe_comm_step_env), so both buffers and the environment
// state end up bit-identical to the stepwise path's.
#pragma once
#include "mpe_comm_core.h"
#include "rollout_separated.h"

typedef SepEpisodeArgs<MpeCommArgs, MPE_COMM_M> CommEpisodeArgs;     // agent 0: speaker, 1: listener

#define COMM_EP_G 16                                                // environments per tile (workgroup)
#define COMM_EP_WAVES 4
#define COMM_X_TILE (16 * MPE_COMM_SHARE)
#define COMM_EP_LDS_FLOATS (COMM_X_TILE + 2 * 16 * TP + 2 * 16)     // observation tile | two logits tiles | action tile

template <bool RELU, int LN>
__global__ __launch_bounds__(COMM_EP_WAVES * WAVE, 1) void rollout_episode_comm_kernel(CommEpisodeArgs e) {
  extern __shared__ __align__(16) float lds[];
  float *X = lds, *tZ = lds + COMM_X_TILE, *act = tZ + 2 * 16 * TP;
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), j = lane & 15, q = lane >> 4;
  constexpr int W = MPE_COMM_SHARE;
  const int T = e.T;
  const int64_t B = e.env.N;                                        // rows of every buffer: one per environment
  const int n0 = (int)blockIdx.x * COMM_EP_G;                       // first environment / buffer row of this tile
  const int64_t i = (int64_t)n0 + j;
  const bool ok = i < B;
  const int jr = ok ? j : 0;
  if (wave < 2) {
    // ---- actor of agent m: step 0 reads buffer slot 0, as the stepwise path does; rows requested before the weights ----
    const int m = wave;
    const int D = m == 0 ? MPE_COMM_OBS_S : MPE_COMM_OBS_L, xo = m == 0 ? 0 : MPE_COMM_OBS_S;
    FwdArgs fa;
    comm_fwd_args(fa, e.a[m], B, e.deterministic);
    f32x4 x[4];
    spread_load_x(x, e.obs_buf[m] + (ok ? i : 0) * D, D, q);
    Trunk16R<LN> tw;
    trunk16r_load<LN>(tw, fa.params, fa.off, fa.desc, j, q);
    Head16R<1> hd;
    head16r_load<1>(hd, fa.params, fa.off, fa.desc.out_dim, j, q);
    const uint64_t ctr0 = e.counter + (e.a[m].counter_dev ? *e.a[m].counter_dev : 0ull);      // read once: the word is fixed for the launch
    for (int t = 0; t < T; ++t) {
      const int64_t so = (int64_t)t * B;
      tile16r_step<RELU, LN, 1, false, true>(fa, tw, hd, x, nullptr, fa.actions + so, fa.logp + so, ctr0 + (uint64_t)t, nullptr,
                                             tZ + m * 16 * TP, i, ok, j, q, act + m * 16);
      __syncthreads();                                              // A_t
      __syncthreads();                                              // B_t
      spread_load_x(x, X + jr * W + xo, D, q);
    }
  } else {
    // ---- critic of agent m: steps 0 .. T; the observation tile of step t >= 1 also goes to the agent's obs[t] / share_obs[t] ----
    const int m = wave - 2;
    const int D = m == 0 ? MPE_COMM_OBS_S : MPE_COMM_OBS_L, xo = m == 0 ? 0 : MPE_COMM_OBS_S;
    FwdArgs fc;
    comm_fwd_args(fc, e.c[m], B, 0);
    const int S = fc.desc.in_dim;                                   // 14 (centralized) or D
    f32x4 x[4];
    spread_load_x(x, e.share_buf[m] + (ok ? i : 0) * S, S, q);
    Trunk16R<LN> tw;
    trunk16r_load<LN>(tw, fc.params, fc.off, fc.desc, j, q);
    Head16R<0> hd;
    head16r_load<0>(hd, fc.params, fc.off, 1, j, q);
    const int Rv = (int)(B - n0 < 16 ? B - n0 : 16);                // rows of the tile that exist (the last tile may be partial)
    // the environments: lanes 0 .. 15 of the speaker's critic wave, one each, the state stays in the lane for the whole episode
    const int n = n0 + lane;
    const bool env_lane = m == 0 && lane < COMM_EP_G && n < e.env.N;
    MpeCommState s = {};
    if (env_lane) mpe_comm_load(e.env, n, s);
    for (int t = 0;; ++t) {
      const int64_t so = (int64_t)t * B;
      if (t >= 1) {         // what the stepwise insert writes for this agent (centralized: the tile's row as it stands)
        float *od = e.obs_buf[m] + (so + n0) * D, *sd = e.share_buf[m] + (so + n0) * S;
        for (int k = lane; k < Rv * D; k += WAVE) { const int row = k / D; od[k] = X[row * W + xo + (k - row * D)]; }
        if (e.centralized) {
          for (int k = lane; k < Rv * W; k += WAVE) sd[k] = X[k];
        } else {
          for (int k = lane; k < Rv * D; k += WAVE) { const int row = k / D; sd[k] = X[row * W + xo + (k - row * D)]; }
        }
      }
      tile16r_step<RELU, LN, 0>(fc, tw, hd, x, t == T ? e.next_values[m] : fc.out + so, nullptr, nullptr, 0ull, nullptr, tZ, i, ok, j, q);
      if (t == T) break;
      __syncthreads();                                              // A_t
      if (env_lane) {       // obs -> the tile's row, rewards -> slot t, masks -> slot t + 1 of both agents' buffers
        float reward;
        const bool done = mpe_comm_step_env(e.env, n, act + lane, act + 16 + lane, s, X + lane * W, X + lane * W + MPE_COMM_OBS_S, reward);
#pragma unroll
        for (int k = 0; k < MPE_COMM_M; ++k) {
          e.rew_buf[k][so + n] = reward;
          e.mask_buf[k][so + B + n] = done ? 0.f : 1.f;
        }
      }
      __syncthreads();                                              // B_t
      spread_load_x(x, X + jr * W + (e.centralized ? 0 : xo), S, q);
    }
    if (env_lane) mpe_comm_store(e.env, n, s, true);                // the environment continues from here in either path
  }
}

extern "C" int mappo_rollout_episode_comm(const mappo_comm_agent *speaker, const mappo_comm_agent *listener, int32_t T, int32_t N,
                                          int32_t env_episode_length, uint64_t env_seed, double *listener_pos, double *listener_vel,
                                          double *landmark_pos, int32_t *goal, int32_t *symbol, int32_t *tstep, int64_t *episode,
                                          int32_t deterministic, uint64_t counter, int32_t centralized,
                                          mappo_stream_t stream) {
  const char *who = "rollout_episode_comm";
  MAPPO_REQUIRE(speaker && listener, "%s: null agent descriptor", who);
  const mappo_comm_agent ag[MPE_COMM_M] = {*speaker, *listener};
  const char *const name[MPE_COMM_M] = {"speaker", "listener"};
  const int Dm[MPE_COMM_M] = {MPE_COMM_OBS_S, MPE_COMM_OBS_L}, Am[MPE_COMM_M] = {MPE_COMM_C, MPE_COMM_U};
  CommEpisodeArgs e;
  if (int rc = sep_episode_fill(e, who, ag, name, Dm, Am, MPE_COMM_SHARE, centralized, deterministic, counter, T, N, env_episode_length)) return rc;
  MAPPO_REQUIRE(listener_pos && listener_vel && landmark_pos && goal && symbol && tstep && episode, "%s: bad arguments (null state pointer)", who);
  MAPPO_CLEAR_STICKY();
  e.env.pos = listener_pos; e.env.vel = listener_vel; e.env.lpos = landmark_pos; e.env.goal = goal; e.env.symbol = symbol; e.env.tstep = tstep;
  e.env.episode = episode; e.env.N = N; e.env.T = env_episode_length; e.env.mode = 1; e.env.seed = env_seed;
  const dim3 grid((unsigned)((N + COMM_EP_G - 1) / COMM_EP_G));
  constexpr int lds_bytes = sizeof(float) * COMM_EP_LDS_FLOATS;
  if (int rc = dispatch_relu_ln<1>(ag[0].actor_desc.use_relu != 0, ag[0].actor_desc.layer_N, [&](auto R, auto L) {
        return launch_kernel<rollout_episode_comm_kernel<R.value, L.value>, lds_bytes>(who, grid, dim3(COMM_EP_WAVES * WAVE), lds_bytes, as_stream(stream), e);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}
