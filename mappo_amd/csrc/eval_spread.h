// eval_spread.h — one EVALUATION episode on the GPU-resident `simple_spread` environment in ONE launch
// (mappo_eval_episode_spread): per step the actor forward and the action choice, then the environment step; the step rewards are
// summed per (environment, agent) row on the device.  No critic, no buffer: what leaves the launch is returns [N][M], the
// optional actions [T][N M] and the environments' state.  The stepwise eval is T x (act, one-hot, env step, mask update) plus a
// stack and a host read, ~4 T launches.
//
// With the rollout episode's critic and buffer writes gone (rollout_spread.h: three waves with a role each and two workgroup
// barriers per step) the dependent chain of a tile is actor -> environment -> actor and nothing runs beside it, so ONE wave walks
// the chain of its tile by itself:
//   * a tile is G = floor(16 / M) whole environments = G M consecutive rows, as in the rollout episode;
//   * the actor's weights sit in LDS (the image of mlp_ep16l.h, staged once per workgroup): the wave holds the tile's activations
//     only, so the environments' float64 state fits in the same wave's registers — lanes 0 .. G - 1 step one environment each
//     (mpe_step_env, the state in the lane for the whole episode) right behind the action choice.  Between the two halves of a
//     step there is a wave-private LDS hand-off (wave_lds_sync) and no workgroup barrier;
//   * a workgroup is EVAL_WAVES = 4 such waves, one per SIMD, that share the image: one barrier (behind the staging) per launch;
//   * lane j (q = 0) of the wave, which chooses row j's action, owns row j's return: acc += r_t in step order, fp32.
// The arithmetic is the rollout episode's: trunk16r_apply on the same 16-byte operands (Trunk16L), the head block of
// tile16r_step's MODE 1 (out_dim 5: block 0 only), categorical_act_lane with Philox (seed, counter + t (+ *counter_dev), row) and
// mpe_step_env — given the same parameters, state, seed and counter the actions and the environments' state are bit-identical to
// mappo_rollout_episode_spread's.  Step 0's observation rows come from the state (mpe_write_obs: what the env's reset / step
// kernels write and warmup copies into the rollout buffer's slot 0).
#pragma once
#include "mpe_core.h"

struct SpreadEvalArgs {
  FwdArgs a;                       // params, desc, off, B, deterministic, seed, counter, counter_dev
  MpeArgs env;                     // state arrays, N, M, L, T = the ENV's episode length, mode 1, seed
  float *returns;                  // [B]
  float *actions;                  // [T][B] or NULL
  int T, G;                        // eval steps, environments per tile (wave)
};

#define EVAL_WAVES 4
#define EVAL_WAVE_FLOATS (16 * MAXD + 16 * TP + 16 + 16)            // per wave: observation tile | logits tile | action tile | reward tile
template <int LN>
constexpr int eval_lds_floats() { return EplMap<LN>::total + EVAL_WAVES * EVAL_WAVE_FLOATS; }

template <bool RELU, int LN>
__global__ __launch_bounds__(EVAL_WAVES * WAVE) void eval_episode_spread_kernel(SpreadEvalArgs e) {
  extern __shared__ __align__(16) float lds[];
  const int lane = threadIdx.x & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE)), j = lane & 15, q = lane >> 4;
  float *X = lds + EplMap<LN>::total + wave * EVAL_WAVE_FLOATS, *tZ = X + 16 * MAXD, *act = tZ + 16 * TP, *rew = act + 16;
  const int M = e.env.M, G = e.G, R = G * M, T = e.T, D = e.a.desc.in_dim, A = e.a.desc.out_dim;
  const int64_t B = e.a.B;
  const int64_t n0 = ((int64_t)blockIdx.x * EVAL_WAVES + wave) * G; // first environment of this wave's tile (beyond N: no tile)
  const int64_t i0 = n0 * M, i = i0 + j;
  const bool ok = j < R && i < B;
  const int jr = ok ? j : 0;
  // ---- environments: one lane each, the state stays in the lane for the whole episode; step 0's observation rows ----
  const int n = (int)(n0 + lane < e.env.N ? n0 + lane : 0);
  const bool env_lane = lane < G && n0 + lane < e.env.N;
  double ap[MPE_MAX_M][2], av[MPE_MAX_M][2], lp[MPE_MAX_L][2];
  int32_t tstep = 0;
  int64_t episode = 0;
  if (env_lane) {
    mpe_load(e.env, n, ap, av, lp);
    tstep = e.env.tstep[n];
    episode = e.env.episode[n];
    mpe_write_obs(e.env, X + lane * M * D, ap, av, lp);
  }
  epl_stage<LN, 1>(lds, e.a.params, e.a.off, e.a.desc);             // every wave, one without a tile too
  const uint64_t ctr0 = e.a.counter + (e.a.counter_dev ? *e.a.counter_dev : 0ull);     // read once: the word is fixed for the launch
  __syncthreads();
  if (n0 >= e.env.N) return;
  const Trunk16L<LN> tw = {lds + j * EPL_WS + 4 * q, lds + 4 * q};
  const Head16L<LN, 1> hd = {tw.m, tw.v};
  const bool fnorm = e.a.desc.use_feature_norm != 0;
  float acc = 0.f;
  for (int t = 0; t < T; ++t) {
    asm volatile("" ::: "memory");          // the image is loop-invariant: keep its reads inside the step (episode16l_body)
    // ---- actor: lane (j, q)'s inputs of tile row j (rows beyond the tile: row 0, zeroed by trunk16r_apply), trunk, head block 0 ----
    f32x4 x[4], h[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) x[b][r] = X[jr * D + min(16 * b + 4 * q + r, D - 1)];
    trunk16r_apply<RELU, LN>(tw, x, h, D, ok, fnorm, q);
    f32x4 z = hd.BH(0);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const f32x4 a = hd.WH(0, b);
#pragma unroll
      for (int r = 0; r < 4; ++r) z = mfma16(a[r], h[b][r], z);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int a = 4 * q + r; if (a < A) tZ[j * TP + a] = z[r]; }
    wave_lds_sync();
    if (ok && q == 0) {
      float action, lgp;
      categorical_act_lane(tZ + j * TP, A, nullptr, e.a.deterministic != 0, e.a.seed, ctr0 + (uint64_t)t, (uint64_t)i, action, lgp);
      act[j] = action;
      if (e.actions) e.actions[(int64_t)t * B + i] = action;
    }
    wave_lds_sync();
    // ---- environments: obs -> the tile (rows lane M ..), rewards -> the reward tile ----
    if (env_lane) mpe_step_env(e.env, n, act + lane * M, ap, av, lp, tstep, episode, X + lane * M * D, rew + lane * M, nullptr, nullptr);
    wave_lds_sync();
    if (ok && q == 0) acc += rew[j];
  }
  if (ok && q == 0) e.returns[i] = acc;
  if (env_lane) {           // the environment continues from here, as after the rollout episode
    mpe_store(e.env, n, ap, av, lp, true);
    e.env.tstep[n] = tstep;
    e.env.episode[n] = episode;
  }
}

extern "C" int mappo_eval_episode_spread(const float *actor_params, const mappo_net_desc *actor_desc, int32_t T, int32_t N, int32_t M,
                                         int32_t L, int32_t env_episode_length, uint64_t env_seed, double *agent_pos, double *agent_vel,
                                         double *landmark_pos, int32_t *tstep, int64_t *episode, int32_t deterministic, uint64_t seed,
                                         uint64_t counter, const uint64_t *counter_dev, float *returns, float *actions,
                                         mappo_stream_t stream) {
  const char *who = "eval_episode_spread";
  if (int rc = check_desc(actor_desc, who)) return rc;
  MAPPO_REQUIRE(actor_desc->in_dim <= MAXD, "%s: in_dim %d: the actor must be narrow (<= %d)", who, actor_desc->in_dim, MAXD);
  MAPPO_REQUIRE(actor_desc->layer_N <= 1, "%s: layer_N %d: the LDS weight image covers layer_N <= 1", who, actor_desc->layer_N);
  MAPPO_REQUIRE(T >= 1 && N >= 1 && env_episode_length >= 1, "%s: bad shape T=%d N=%d env episode length %d", who, T, N, env_episode_length);
  MAPPO_REQUIRE(M >= 1 && M <= MPE_MAX_M && L >= 1 && L <= MPE_MAX_L, "%s: M=%d L=%d out of range (1 .. %d)", who, M, L, MPE_MAX_M);
  const int D = 4 + 2 * L + 4 * (M - 1);
  MAPPO_REQUIRE(actor_desc->in_dim == D && actor_desc->out_dim == 5, "%s: actor in_dim %d / out_dim %d: simple_spread with M=%d L=%d has "
                "%d observation features and 5 actions", who, actor_desc->in_dim, actor_desc->out_dim, M, L, D);
  MAPPO_REQUIRE(actor_params && agent_pos && agent_vel && landmark_pos && tstep && episode && returns, "%s: bad arguments (null pointer)", who);
  MAPPO_CLEAR_STICKY();
  SpreadEvalArgs e = {};
  e.a.params = actor_params; e.a.desc = *actor_desc; e.a.B = (int64_t)N * M; e.a.deterministic = deterministic;
  e.a.seed = seed; e.a.counter = counter; e.a.counter_dev = counter_dev; e.a.off = net_offsets(e.a.desc);
  e.env.apos = agent_pos; e.env.avel = agent_vel; e.env.lpos = landmark_pos; e.env.tstep = tstep; e.env.episode = episode;
  e.env.N = N; e.env.M = M; e.env.L = L; e.env.T = env_episode_length; e.env.mode = 1; e.env.seed = env_seed;
  e.returns = returns; e.actions = actions;
  e.T = T; e.G = 16 / M;
  const int64_t n_tiles = ((int64_t)N + e.G - 1) / e.G;
  const dim3 grid((unsigned)((n_tiles + EVAL_WAVES - 1) / EVAL_WAVES)), block(EVAL_WAVES * WAVE);
  if (int rc = dispatch_relu_ln<1>(actor_desc->use_relu != 0, actor_desc->layer_N, [&](auto R, auto L) {
        constexpr int lds_bytes = (int)sizeof(float) * eval_lds_floats<L.value>();
        return launch_kernel<eval_episode_spread_kernel<R.value, L.value>, lds_bytes>(who, grid, block, lds_bytes, as_stream(stream), e);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}
