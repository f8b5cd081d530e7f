// rollout_separated.h — what the one-launch episodes of the SEPARATED runner share (rollout_comm.h, rollout_sep_img.h, rollout_tag.h,
// rollout_push.h; rollout_world_comm.h uses the checks and the actors' half of the fill): M agents of different shapes, each with its
// own actor, critic and SeparatedReplayBuffer, on a GPU-resident env whose steps run inside the launch.  The kernels differ — where the
// weights live and which wave steps the environments; their headers say why — but around them they are one thing:
//   the argument block (SepEpisodeArgs: two CommNet per agent, the env's own args, the agents' buffer arrays);
//   the host's checks of the M agent descriptors and the fill of that block (sep_episode_fill); an entry point adds its env state
//   and launches through sep_episode_launch: one workgroup of SEP_EP_WAVES waves per tile of SEP_EP_G environments;
//   for the scenarios with a traits struct (rollout_sep_img.h, rollout_tag.h, rollout_push.h), the two pieces of a step that touch
//   the buffers: the row copy "what the stepwise insert writes" (sep_copy_rows) and the env lanes' step (sep_env_step; the tag and
//   push kernels keep that block inline: through the function their register allocation moved and a rollout took ~2 % longer).
// rollout_comm.h and rollout_world_comm.h keep their own inline copies of those two and of the launch tail: their environments have
// another shape (one shared reward and split action pointers; a MultiDiscrete leader), and both kernels sit at the register limit —
// the comm kernel with 112 B of scratch, where a shared row copy moved its register count.
#pragma once
#include "rollout_spread.h"
#include <cstdio>

#define SEP_EP_G 16                                                 // environments per tile (workgroup)
#define SEP_EP_WAVES 4                                              // one per SIMD

struct CommNet {                   // what tile16r_step reads of a FwdArgs, per network (2 M FwdArgs would not fit the kernel arguments)
  const float *params;
  float *out, *actions, *logp;     // critic: values [T][N] | actor: actions / logp [T][N]
  mappo_net_desc desc;
  NetOff off;
  uint64_t seed;
  const uint64_t *counter_dev;     // actor: the agent's own device word added to the counter (may be null)
};

template <class EnvArgs, int M>
struct SepEpisodeArgs {
  CommNet a[M], c[M];                            // per agent, in the env's agent order
  EnvArgs env;                                   // state arrays, N, T = the ENV's episode length, mode 1, seed
  float *obs_buf[M], *share_buf[M];              // [T + 1][N][D_m], [T + 1][N][S_m]
  float *rew_buf[M], *mask_buf[M];               // [T][N], [T + 1][N]
  float *next_values[M];                         // [N]: the critic at step T
  uint64_t counter;
  int T, centralized, deterministic;             // rollout steps
};

__device__ __forceinline__ void comm_fwd_args(FwdArgs &f, const CommNet &n, int64_t B, int deterministic) {
  f = FwdArgs{};
  f.params = n.params; f.out = n.out; f.actions = n.actions; f.logp = n.logp; f.desc = n.desc; f.off = n.off; f.B = B;
  f.deterministic = deterministic; f.seed = n.seed;
}

// The host side of an entry point up to its env: refuse what the kernels are not built for — agent m's actor is Dm[m] -> Am[m], its
// critic share -> 1 (centralized) or Dm[m] -> 1, all 2 M networks feed-forward with one layer_N <= 1 and one activation — and fill
// everything of `e` but e.env.  ag: the M descriptors; name: what the messages call each agent.
template <class EnvArgs, int M>
static int sep_episode_fill(SepEpisodeArgs<EnvArgs, M> &e, const char *who, const mappo_comm_agent *ag, const char *const *name, const int *Dm,
                            const int *Am, int share, int32_t centralized, int32_t deterministic, uint64_t counter, int32_t T, int32_t N,
                            int32_t env_episode_length) {
  for (int m = 0; m < M; ++m) {
    const mappo_net_desc &da = ag[m].actor_desc, &dc = ag[m].critic_desc;
    MAPPO_REQUIRE(!da.recurrent && !dc.recurrent, "%s: %s: recurrent networks take the stepwise path (this launch is feed-forward only)", who,
                  name[m]);
    MAPPO_REQUIRE(da.layer_N >= 0 && da.layer_N <= 1, "%s: %s: layer_N %d: this launch takes layer_N <= 1", who, name[m], da.layer_N);
    if (int rc = check_desc(&da, who)) return rc;
    if (int rc = check_desc(&dc, who)) return rc;
    MAPPO_REQUIRE(da.in_dim == Dm[m] && da.out_dim == Am[m], "%s: %s actor in_dim %d / out_dim %d: the scenario has in_dim %d and %d actions "
                  "there", who, name[m], da.in_dim, da.out_dim, Dm[m], Am[m]);
    MAPPO_REQUIRE(dc.out_dim == 1, "%s: %s critic out_dim must be 1", who, name[m]);
    if (centralized && dc.in_dim != share) {
      char sum[16 * M];                                             // "8 + 10 + 10"
      for (int k = 0, n = 0; k < M; ++k) n += snprintf(sum + n, sizeof(sum) - n, k ? " + %d" : "%d", Dm[k]);
      MAPPO_REQUIRE(false, "%s: %s: centralized critic needs in_dim %s = %d (got %d)", who, name[m], sum, share, dc.in_dim);
    }
    MAPPO_REQUIRE(centralized || dc.in_dim == Dm[m], "%s: %s critic in_dim %d != actor in_dim %d", who, name[m], dc.in_dim, Dm[m]);
    MAPPO_REQUIRE(da.layer_N == ag[0].actor_desc.layer_N && dc.layer_N == da.layer_N && da.use_relu == ag[0].actor_desc.use_relu &&
                  dc.use_relu == da.use_relu, "%s: all %d networks must share layer_N and the activation", who, 2 * M);
  }
  MAPPO_REQUIRE(T >= 1 && N >= 1 && env_episode_length >= 1, "%s: bad shape T=%d N=%d env episode length %d (each needs >= 1)", who, T, N,
                env_episode_length);
  for (int m = 0; m < M; ++m)
    MAPPO_REQUIRE(ag[m].actor_params && ag[m].critic_params && ag[m].obs_buf && ag[m].share_buf && ag[m].rew_buf && ag[m].mask_buf &&
                  ag[m].actions && ag[m].logp && ag[m].values && ag[m].next_values, "%s: bad arguments (null pointer, %s)", who, name[m]);
  e = {};
  for (int m = 0; m < M; ++m) {
    e.a[m].params = ag[m].actor_params; e.a[m].actions = ag[m].actions; e.a[m].logp = ag[m].logp; e.a[m].desc = ag[m].actor_desc;
    e.a[m].off = net_offsets(e.a[m].desc); e.a[m].seed = ag[m].seed; e.a[m].counter_dev = ag[m].counter_dev;
    e.c[m].params = ag[m].critic_params; e.c[m].out = ag[m].values; e.c[m].desc = ag[m].critic_desc; e.c[m].off = net_offsets(e.c[m].desc);
    e.obs_buf[m] = ag[m].obs_buf; e.share_buf[m] = ag[m].share_buf; e.rew_buf[m] = ag[m].rew_buf; e.mask_buf[m] = ag[m].mask_buf;
    e.next_values[m] = ag[m].next_values;
  }
  e.counter = counter; e.T = T; e.centralized = centralized; e.deterministic = deterministic;
  return MAPPO_OK;
}

// What the stepwise insert writes into agent m's slot t + 1 (dst row offset `row0` = (t + 1) N + n0), by one whole wave: the agent's D
// columns from xo of the observation tile X [16][W] -> obs, and the tile's whole row (centralized) or the same columns again ->
// share_obs.  Rv: rows of the tile that exist.
template <int W, class EnvArgs, int M>
__device__ __forceinline__ void sep_copy_rows(const SepEpisodeArgs<EnvArgs, M> &e, const float *X, int m, int D, int xo, int64_t row0, int Rv,
                                              int lane) {
  float *od = e.obs_buf[m] + row0 * D;
  for (int k = lane; k < Rv * D; k += WAVE) { const int r = k / D; od[k] = X[r * W + xo + (k - r * D)]; }
  if (e.centralized) {
    float *sd = e.share_buf[m] + row0 * W;
    for (int k = lane; k < Rv * W; k += WAVE) sd[k] = X[k];
  } else {
    float *sd = e.share_buf[m] + row0 * D;
    for (int k = lane; k < Rv * D; k += WAVE) { const int r = k / D; sd[k] = X[r * W + xo + (k - r * D)]; }
  }
}

// The env lane's part of step t (so = t N), between the barriers A_t and B_t: environment n, whose state s the lane holds, takes the
// agents' actions from column `lane` of the action tile, writes its observations into row `lane` of the tile X [16][Env::SHARE], each
// agent's OWN reward into slot t of its buffer and 1 - done into slot t + 1.  Env: the scenario's traits (mpe_*_core.h).
template <class Env>
__device__ __forceinline__ void sep_env_step(const SepEpisodeArgs<typename Env::Args, Env::M> &e, int n, int64_t so, int64_t B,
                                             typename Env::State &s, float *X, const float *act, int lane) {
  float reward[Env::M];
  float *o[Env::M];
#pragma unroll
  for (int k = 0; k < Env::M; ++k) o[k] = X + lane * Env::SHARE + Env::obs_off(k);
  const bool done = Env::step_env(e.env, n, act + lane, 16, s, o, reward);
#pragma unroll
  for (int k = 0; k < Env::M; ++k) {
    e.rew_buf[k][so + n] = reward[k];
    e.mask_buf[k][so + B + n] = done ? 0.f : 1.f;
  }
}

// The tail of an entry point: the grid, the (activation, layer_N) instantiation and the launch.  K<RELU, LN> names it: `kernel` and
// its dynamic `lds_bytes`.  first: the descriptor all networks were checked against (sep_episode_fill).
template <template <bool, int> class K, class Args>
static int sep_episode_launch(const char *who, int32_t N, const mappo_comm_agent &first, const Args &e, mappo_stream_t stream) {
  const dim3 grid((unsigned)((N + SEP_EP_G - 1) / SEP_EP_G));
  if (int rc = dispatch_relu_ln<1>(first.actor_desc.use_relu != 0, first.actor_desc.layer_N, [&](auto R, auto L) {
        typedef K<R.value, L.value> Inst;
        return launch_kernel<Inst::kernel, Inst::lds_bytes>(who, grid, dim3(SEP_EP_WAVES * WAVE), Inst::lds_bytes, as_stream(stream), e);
      }))
    return rc;
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}
