/*
 * mappo_hip.h — C ABI of libmappo_hip.so: the MI355X (gfx950) hot path of MAPPO training
 * (rollout forward -> GAE -> PPO minibatch update) as hand-written HIP kernels.
 *
 * The reference (Chen001117/mappo) has no FFI on this path: everything is Python/NumPy/torch
 * (SURVEY.md §8b).  Each entry point therefore cites the reference *Python* site it replaces; the
 * binding a maintainer would add on the reference side is the ctypes stub in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success or a negative MAPPO_E* code; mappo_last_error() gives text.
 *   - all pointers are DEVICE pointers owned by the caller unless marked "host"; no hidden allocation,
 *     no host synchronisation; work is enqueued on `stream` (a hipStream_t passed as void*).
 *   - all arrays are float32, row-major.  Buffer arrays use the reference's memory order
 *     [T(+1)][R = n_rollout_threads * num_agents][D] (shared_buffer.py:45-75), so a "flat row" is t*R + r.
 *   - `rows` arguments are int32 flat rows selecting the minibatch (the generators' fancy indexing,
 *     shared_buffer.py:246-286, 397-494); NULL means the identity 0..B-1.
 *   - ValueNorm state is 3 device floats {running_mean, running_mean_sq, debiasing_term} (valuenorm.py:21-23).
 */
#ifndef MAPPO_HIP_H
#define MAPPO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *mappo_stream_t; /* hipStream_t */

#define MAPPO_OK 0
#define MAPPO_EINVAL (-1)    /* bad argument / unsupported shape */
#define MAPPO_ELAUNCH (-2)   /* HIP launch error */
#define MAPPO_ENOTIMPL (-3)  /* valid in the reference but not built here (e.g. popart) */

#define MAPPO_HIDDEN 64      /* hidden_size the MFMA kernels are tiled for (config.py:199 default) */
#define MAPPO_MAX_IN_DIM 2048 /* obs / share_obs width (Discrete action spaces; 65..512: the tuned wide kernels, 513..2048: the
                               * sliced layer-1 kernels — the entry points that stay at 512 or 64 say so below and refuse by name) */
#define MAPPO_MAX_ACTIONS 32 /* Discrete(n) with n <= 32 */
#define MAPPO_MAX_LAYER_N 2

const char *mappo_last_error(void);
int mappo_abi_version(void);

/* ---- network description -------------------------------------------------------------------------
 * One actor or critic: MLPBase (mlp.py:31-55) -> [GRU + LayerNorm (rnn.py:7-80)] -> Linear head
 * (Categorical logits, distributions.py:55-68, or v_out, r_actor_critic.py:136-142).
 * Parameters live in ONE flat float array in this order (state_dict order minus the unused fc_h):
 *   feature_norm.{w,b}[in_dim] (if use_feature_norm) | fc1.0.{W[H][in_dim], b[H]} | fc1.2.{w,b}[H] |
 *   layer_N x { fc2.i.0.{W[H][H], b[H]} | fc2.i.2.{w,b}[H] } |
 *   (if recurrent) rnn.{weight_ih[3H][H], weight_hh[3H][H], bias_ih[3H], bias_hh[3H]} | rnn.norm.{w,b}[H] |
 *   head.{W[out_dim][H], b[out_dim]}
 * mappo_net_param_count() returns the float count; offsets follow from the order above. */
typedef struct {
  int32_t in_dim;            /* obs_dim (actor) or share_obs_dim (critic) */
  int32_t hidden;            /* must be MAPPO_HIDDEN */
  int32_t out_dim;           /* n actions (actor) or 1 (critic) */
  int32_t layer_N;           /* config.py:201, 0..MAPPO_MAX_LAYER_N */
  int32_t use_relu;          /* config.py:203 (0 = tanh) */
  int32_t use_feature_norm;  /* config.py:208 */
  int32_t recurrent;         /* use_recurrent_policy || use_naive_recurrent_policy */
} mappo_net_desc;

int64_t mappo_net_param_count(const mappo_net_desc *desc /*host*/);

/* ---- K1: MPE rollout insert (mpe_runner.py:125-139, shared_buffer.py:96-112) in one launch -----------------------
 * Sources may be strided / broadcast views (strides in elements); destinations are the contiguous buffer slots
 * obs[step+1], share_obs[step+1], rewards[step], masks[step+1].  centralized != 0 builds share_obs as the thread's
 * concatenated agent observations repeated per agent (use_centralized_V). */
int mappo_insert_mpe(const float *obs, int64_t obs_stride_n, int64_t obs_stride_m, const float *rewards,
                     int64_t rew_stride_n, int64_t rew_stride_m, const uint8_t *dones /*bool bytes*/,
                     int64_t done_stride_n, int64_t done_stride_m, float *obs_dst, float *share_dst, float *rew_dst,
                     float *mask_dst, int32_t N, int32_t M, int32_t D, int32_t centralized, mappo_stream_t stream);
/* The same for recurrent policies (mpe_runner.py:126-128 + shared_buffer.py:96-97): additionally
 * rnn_dst / rnn_critic_dst [N*M][H] (slot step+1) = rnn_states / rnn_states_critic * (1 - done); H = recurrent_N * hidden. */
int mappo_insert_mpe_rnn(const float *obs, int64_t obs_stride_n, int64_t obs_stride_m, const float *rewards,
                         int64_t rew_stride_n, int64_t rew_stride_m, const uint8_t *dones, int64_t done_stride_n,
                         int64_t done_stride_m, float *obs_dst, float *share_dst, float *rew_dst, float *mask_dst, int32_t N,
                         int32_t M, int32_t D, int32_t centralized, const float *rnn_states, const float *rnn_states_critic,
                         float *rnn_dst, float *rnn_critic_dst, int32_t H, mappo_stream_t stream);

/* K1 for the SMAC runner (smac_runner.py:129-151 + shared_buffer.py:74-112) in one launch.  dones_env[n] = all_m dones[n][m];
 * masks = 1 - dones_env, active_masks = dones_env ? 1 : 1 - dones, bad_masks = 1 - bad_transition (NULL: all 1),
 * rnn slots = states * (1 - dones_env) (rnn_states NULL: skipped); obs [N*M][D], share_obs [N*M][S], avail [N*M][A] (or NULL)
 * and rewards are copied to their slots.  dones / bad_transition are bool bytes. */
int mappo_insert_smac(const float *obs, const float *share_obs, const float *avail, const float *rewards, int64_t rew_stride_n,
                      int64_t rew_stride_m, const uint8_t *dones, int64_t done_stride_n, int64_t done_stride_m,
                      const uint8_t *bad_transition, const float *rnn_states, const float *rnn_states_critic, float *obs_dst,
                      float *share_dst, float *avail_dst, float *rew_dst, float *mask_dst, float *bad_mask_dst,
                      float *active_mask_dst, float *rnn_dst, float *rnn_critic_dst, int32_t N, int32_t M, int32_t D, int32_t S,
                      int32_t A, int32_t H, mappo_stream_t stream);

/* recurrent_generator's row indices (shared_buffer.py:385-494) for all ppo epochs of one train() in one launch: perm
 * [n_epochs][data_chunks] (int64 permutations of the chunks, device), mbs = data_chunks / num_mini_batch;
 * rows [n_epochs][num_mini_batch][L*mbs] (time-major: l*mbs + j) and h0_rows [n_epochs][num_mini_batch][mbs] are buffer rows
 * (q % T)*R + q / T of flat position q = chunk*L + l in the reference's (n, m, t) order (T = episode_length, R = N*M). */
int mappo_recurrent_rows(const int64_t *perm, int32_t n_epochs, int64_t data_chunks, int32_t L, int32_t T, int32_t R,
                         int32_t num_mini_batch, int32_t *rows, int32_t *h0_rows, mappo_stream_t stream);

/* K1, after_update (shared_buffer.py:114-131): `count` (<= 16) independent fp32 device copies in one launch.
 * dst / src / n_floats are HOST arrays of device pointers / lengths. */
int mappo_copy_batch(int32_t count, float *const *dst, const float *const *src, const int64_t *n_floats, mappo_stream_t stream);

/* ---- K2: compute_returns (shared_buffer.py:168-224), all four flag branches ------------------------
 * Segmented affine-map scan over T: one wavefront per (64 series x time segment), segment composites
 * combined through LDS.  Writes value_preds[T] <- next_value (GAE branches) or returns[T] <- next_value
 * (discounted branches) exactly like the reference.  vn_state NULL => no value normaliser. */
int mappo_gae_scan(const float *rewards /*[T][R]*/, float *value_preds /*[T+1][R]*/,
                   const float *next_value /*[R]*/, const float *masks /*[T+1][R]*/,
                   const float *bad_masks /*[T+1][R]*/, float *returns /*[T+1][R]*/,
                   const float *vn_state /*[3] or NULL*/, int32_t T, int32_t R, float gamma,
                   float gae_lambda, int32_t use_gae, int32_t use_proper_time_limits,
                   mappo_stream_t stream);

/* ---- K3: advantage build + normalisation (r_mappo.py:174-182) ---------------------------------------
 * adv = returns - denorm(value_preds); moments {sum, sum_sq, count} over entries with active != 0
 * (double accumulation, deterministic two-stage reduction); adv <- (adv - mean) / (std + 1e-5).
 * The two calls are split so that a multi-GPU caller can all-reduce `moments` in between (§8e C2). */
int64_t mappo_adv_workspace_bytes(int64_t n);
int mappo_adv_moments(const float *returns /*[n]*/, const float *value_preds /*[n]*/,
                      const float *active_masks /*[n]*/, const float *vn_state /*[3] or NULL*/,
                      float *adv /*[n] out (raw)*/, double *moments /*[3] out*/, void *workspace,
                      int64_t n, mappo_stream_t stream);
int mappo_adv_normalize(float *adv /*[n] in/out*/, const double *moments /*[3]*/, int64_t n,
                        mappo_stream_t stream);

/* ---- K12: ValueNorm (valuenorm.py:37-54) + minibatch denominators ---------------------------------
 * mappo_minibatch_moments: {sum ret, sum ret^2, sum active, B} over the minibatch rows (double).
 * mappo_valuenorm_update: EMA update of vn_state from those moments (batch mean = sum/B). */
int64_t mappo_moments_workspace_bytes(int64_t B);
int mappo_minibatch_moments(const float *returns, const float *active_masks, const int32_t *rows,
                            int64_t B, double *mb_moments /*[4] out*/, void *workspace,
                            mappo_stream_t stream);
int mappo_valuenorm_update(float *vn_state /*[3] in/out*/, const double *mb_moments /*[4]*/,
                           double beta, mappo_stream_t stream);
/* n successive ValueNorm.update calls with the SAME batch moments (ppo_epoch updates on whole-buffer minibatches) in
 * one launch: states_out[e] (e = 0..n-1, 3 floats each) is the state after e+1 updates — what update e's value loss
 * normalises with — and vn_state ends as states_out[n-1].  Same fp32 rounding sequence as n single calls. */
int mappo_valuenorm_update_n(float *vn_state /*[3] in/out*/, const double *mb_moments /*[4]*/, double beta, int32_t n,
                             float *states_out /*[n][3]*/, mappo_stream_t stream);

/* ---- K5 (+K6): fused PPO loss forward+backward (r_mappo.py:52-89,124-141; act.py:154-160) ----------
 * One pass over the minibatch: availability masking, log-softmax, log-prob gather, entropy,
 * ratio / clipped surrogate, clipped Huber|MSE value error; emits d(actor objective)/d logits,
 * d(value_loss_coef * value loss)/d values and per-block double partial sums of the 4 statistics.
 * [B][A] tiles are staged through LDS so that HBM sees only full-line traffic.
 * Algorithmic bytes per sample: 4*(3A+8) with avail, 4*(2A+8) without. */
typedef struct {
  float clip_param, entropy_coef, value_loss_coef, huber_delta;
  int32_t use_huber_loss, use_clipped_value_loss, use_policy_active_masks, use_value_active_masks,
      use_valuenorm;
  /* mappo_actor_update / mappo_critic_update: != 0 ADDS this launch's per-workgroup loss sums to `partials` instead of
   * overwriting them.  With identical denominators in every update (whole-buffer minibatches) one mappo_update_stats
   * call after the last epoch then yields the sum of the per-update statistics the trainer logs. */
  int32_t accumulate_partials;
} mappo_ppo_cfg;

int64_t mappo_ppo_loss_workspace_bytes(int64_t B);
int mappo_ppo_loss_fwd_bwd(const float *logits /*[B][A] minibatch order, pre-mask*/,
                           const float *values /*[B] minibatch order*/, const int32_t *rows /*[B]|NULL*/,
                           const float *avail /*[.][A] buffer order or NULL*/, const float *actions,
                           const float *old_logp, const float *adv, const float *active,
                           const float *v_old, const float *returns /*buffer order, indexed by rows*/,
                           const float *vn_state /*[3] AFTER update, or NULL*/,
                           const double *mb_moments /*[4] from mappo_minibatch_moments*/,
                           float *dlogits /*[B][A]*/, float *dvalues /*[B]*/, double *stats /*[6] out:
                           value_loss, policy_loss, dist_entropy, ratio_mean, sum_active, B*/,
                           void *workspace, const mappo_ppo_cfg *cfg /*host*/, int64_t B, int32_t A,
                           mappo_stream_t stream);

/* ---- K7/K6/K8: fused MLP trunk + head on fp32 MFMA (mlp.py:18-28,50-55; act.py:78-81) --------------
 * Weights resident in LDS, activations of a 32-sample wave tile live in registers/LDS; LayerNorm and
 * the activation are fused between the v_mfma_f32_32x32x2_f32 chains.
 *   mappo_mlp_forward : out[B][out_dim] = head(trunk(x[rows]))                       (evaluate / get_values)
 *   mappo_actor_act   : same trunk + masking + sample|argmax + log-prob               (get_actions / act)
 *   mappo_mlp_backward: recomputes the forward per tile (no activation round trip through HBM) and
 *                       accumulates the parameter gradient of sum_b <dout[b], out[b]> into per-block
 *                       slabs [n_slabs][slab_stride] at column `slab_col0` (flat parameter order). */
int mappo_mlp_forward(const float *params, const mappo_net_desc *desc /*host*/, const float *x /*[.][in_dim]*/,
                      const int32_t *rows /*[B] or NULL*/, int64_t B, float *out /*[B][out_dim]*/,
                      mappo_stream_t stream);
/* Sampling contract (tests/rollout_ref.py restates it on the host): the draw of a row is Philox4x32-10 with key words {seed lo, seed hi}
 * and counter words {row index lo, row index hi, counter lo, counter hi}; u = (output word 0 >> 8) * 2^-24, a 24-bit uniform in [0, 1).
 * The action is the first a with u < p_0 + ... + p_a over the masked softmax (unavailable actions have p = 0); if rounding leaves u
 * at or above the last sum, it is the last action with p > 0.  deterministic: the first maximum.  Every sampling entry point uses
 * row index = the row's position in its [B] (per step of [T][B]) output, and counter + t (+ *counter_dev) for step t (t = 0 for one step). */
int mappo_actor_act(const float *params, const mappo_net_desc *desc /*host*/, const float *obs,
                    const float *avail /*[B][A] or NULL*/, int64_t B, int32_t deterministic,
                    uint64_t seed, uint64_t counter, const uint64_t *counter_dev /*device word added to counter, or NULL*/,
                    float *actions /*[B] fp32 (buffer dtype)*/, float *logp /*[B]*/, mappo_stream_t stream);
/* One launch per rollout step (mpe_runner.py:95-139): actor get_actions + critic get_values (+ optionally the insert
 * of the env output the rows are read from).  Rows may be strided views of the env's output: with M > 0 sample i is
 * (thread n, agent m) = (i / M, i % M) and starts at base[n*stride_n + m*stride_m]; M == 0: contiguous [B][in_dim].
 * obs_dst != NULL additionally performs mappo_insert_mpe(obs, rewards, dones -> obs_dst, share_dst, rew_dst, mask_dst)
 * (N = B / M threads) inside the same launch.  actions == logp == NULL skips the actor (bootstrap value of the last
 * step: critic + insert).  Networks with in_dim <= 64 that share layer_N and the activation. */
int mappo_rollout_step(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, const float *critic_params,
                       const mappo_net_desc *critic_desc /*host*/, const float *obs, int64_t obs_stride_n,
                       int64_t obs_stride_m, const float *share_obs, int64_t share_stride_n, int64_t share_stride_m,
                       int32_t M, int64_t B, const float *avail /*[B][A] or NULL*/, int32_t deterministic, uint64_t seed,
                       uint64_t counter, const uint64_t *counter_dev, float *actions /*[B]*/, float *logp /*[B]*/,
                       float *values /*[B]*/, float *obs_dst /*or NULL: no insert*/, float *share_dst, const float *rewards,
                       int64_t rew_stride_n, int64_t rew_stride_m, const uint8_t *dones, int64_t done_stride_n,
                       int64_t done_stride_m, float *rew_dst, float *mask_dst, int32_t centralized, mappo_stream_t stream);
/* ---- MultiDiscrete action spaces (envs/mpe/environment.py:82-86; act.py:27-33,65-76,139-152): one Categorical head per
 * sub-action.  Head j has d_j = head_dims[j] actions; the actor's out_dim is A = sum d_j and its head parameters are the heads'
 * weight rows / biases side by side (W[A][H] | b[A], head j = rows [d_0 + .. + d_{j-1}, .. + d_j)).  actions / logp are [B][K]
 * (K = n_heads): the head-local index as fp32 and one log-prob per head, not summed.
 * Limits, checked on the host before any launch (MAPPO_EINVAL, mappo_last_error() names the limit): 1 <= K <= 4, every d_j >= 1,
 * sum d_j == out_dim <= 16, in_dim <= 64, layer_N <= 1, not recurrent, avail == NULL (the space has no available_actions).
 * Sampling contract: head j of row i draws Philox index (j << 32) | i — counter words {i, j, counter lo, counter hi} — with the key
 * and counter of the contract above; inside a head the rule is the same (first a with u < C_a, fallback to the last action with
 * p > 0, deterministic = first maximum).  Head 0 therefore draws exactly what a Discrete policy draws. */
int mappo_actor_act_md(const float *params, const mappo_net_desc *desc /*host*/, const float *obs, const float *avail /*NULL*/,
                       const int32_t *head_dims /*host*/, int32_t n_heads, int64_t B, int32_t deterministic, uint64_t seed,
                       uint64_t counter, const uint64_t *counter_dev, float *actions /*[B][K]*/, float *logp /*[B][K]*/,
                       mappo_stream_t stream);
/* mappo_rollout_step for such a policy: actor + critic + optional insert in one launch (both networks in_dim <= 64). */
int mappo_rollout_step_md(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, const float *critic_params,
                          const mappo_net_desc *critic_desc /*host*/, const float *obs, int64_t obs_stride_n, int64_t obs_stride_m,
                          const float *share_obs, int64_t share_stride_n, int64_t share_stride_m, int32_t M, int64_t B,
                          const float *avail /*NULL*/, const int32_t *head_dims /*host*/, int32_t n_heads, int32_t deterministic,
                          uint64_t seed, uint64_t counter, const uint64_t *counter_dev, float *actions /*[B][K]*/, float *logp /*[B][K]*/,
                          float *values /*[B]*/, float *obs_dst /*or NULL: no insert*/, float *share_dst, const float *rewards,
                          int64_t rew_stride_n, int64_t rew_stride_m, const uint8_t *dones, int64_t done_stride_n, int64_t done_stride_m,
                          float *rew_dst, float *mask_dst, int32_t centralized, mappo_stream_t stream);
/* One launch per rollout EPISODE, for envs whose output for the whole episode exists before it starts and does not depend on
 * the actions (synthetic MPE): what T + 1 mappo_rollout_step calls do, with the env output of step t at
 * env_obs[t*obs_stride_t + n*obs_stride_n + m*obs_stride_m + d], rewards / dones likewise (bool bytes).  Actor on the rows of
 * step t < T (step 0: obs_buf slot 0, step t >= 1: the env output of step t - 1 in place) with counter + t (+ *counter_dev)
 * -> actions / logp [T][B]; critic on the share rows of step t <= T -> values [T][B], step T -> next_values [B]; the env output
 * of step t is copied into obs_buf / share_buf slot t + 1 ([T+1][B][in_dim]), rew_buf [T][B] slot t and mask_buf [T+1][B]
 * slot t + 1.  B = N*M rows; networks with in_dim <= 64 that share layer_N and the activation; not recurrent; no available
 * actions.  centralized: the critic's row of (n, m) is the thread's M agent rows side by side (obs_stride_m == in_dim). */
int mappo_rollout_episode(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, const float *critic_params,
                          const mappo_net_desc *critic_desc /*host*/, int32_t T, int32_t N, int32_t M, const float *env_obs,
                          int64_t obs_stride_t, int64_t obs_stride_n, int64_t obs_stride_m, const float *rewards,
                          int64_t rew_stride_t, int64_t rew_stride_n, int64_t rew_stride_m, const uint8_t *dones,
                          int64_t done_stride_t, int64_t done_stride_n, int64_t done_stride_m, int32_t deterministic,
                          uint64_t seed, uint64_t counter, const uint64_t *counter_dev, float *obs_buf, float *share_buf,
                          float *rew_buf, float *mask_buf, float *actions /*[T][B]*/, float *logp /*[T][B]*/,
                          float *values /*[T][B]*/, float *next_values /*[B]*/, int32_t centralized, mappo_stream_t stream);
/* Which kernel body mappo_rollout_episode takes for this layer_N under the current environment: 1 = weights in LDS, several waves
 * per SIMD (layer_N 0 / 1, the default), 0 = weights in registers (layer_N 2, MAPPO_EPISODE_LDS=0, or any of the register body's
 * geometry overrides MAPPO_EPISODE_WAVES / _NET_WAVES / _INS_WAVES / _COST_A set without MAPPO_EPISODE_LDS). */
int mappo_rollout_episode_uses_lds(int32_t layer_N);
int32_t mappo_mlp_backward_slabs(int64_t B); /* number of slabs the launch below will write */
int mappo_mlp_backward(const float *params, const mappo_net_desc *desc /*host*/, const float *x,
                       const int32_t *rows, int64_t B, const float *dout /*[B][out_dim]*/,
                       float *slabs, int64_t slab_stride, int64_t slab_col0,
                       float *wide_ws /*in_dim > 64: mappo_wide_workspace_floats(B) floats, else NULL*/,
                       mappo_stream_t stream);
/* Wide observations (64 < in_dim <= MAPPO_MAX_IN_DIM = 2048; up to 512 the tuned kernels, beyond them layer 1 in K slices; reference: mlp.py:18-55 with a wide input layer): the update / backward launches
 * run layer 1 as their own MFMA kernel and leave d z1 plus the per-row LayerNorm statistics in `wide_ws`;
 * mappo_wide_l1_backward then produces the W1 and feature-norm gradient columns (one slab row per workgroup of its grid.x,
 * mappo_wide_l1_slabs(B) rows).  The workspace has one of two layouts, a PURE function of the descriptor and of which
 * entry point filled it — mappo_wide_layout(desc, producer) — and the caller hands that value to mappo_wide_l1_backward:
 * the library keeps no host-side record of workspaces (re-entrant per stream, safe across allocator address reuse). */
#define MAPPO_WIDE_LAYOUT_FEATURE_MAJOR 0   /* dz1 [64][B] | mean0 [B] | rstd0 [B]                       (K-chunked kernels)   */
#define MAPPO_WIDE_LAYOUT_BLOCKED 1         /* dz1 [tile][64][16] | padded statistics | z1 [B][64]        (16-sample-tile path) */
#define MAPPO_PRODUCER_MLP_BACKWARD 0       /* mappo_mlp_backward   */
#define MAPPO_PRODUCER_ACTOR_UPDATE 1       /* mappo_actor_update   */
#define MAPPO_PRODUCER_CRITIC_UPDATE 2      /* mappo_critic_update  */
#define MAPPO_PRODUCER_TRUNK_BACKWARD 3     /* mappo_trunk_backward */
int64_t mappo_wide_workspace_floats(int64_t B);
int32_t mappo_wide_l1_slabs(int64_t B);
int32_t mappo_wide_layout(const mappo_net_desc *desc /*host*/, int32_t producer /*MAPPO_PRODUCER_**/); /* layout id, or MAPPO_EINVAL */
int mappo_wide_l1_backward(const float *params, const mappo_net_desc *desc /*host*/, const float *x, const int32_t *rows,
                           int64_t B, const float *wide_ws, float *slabs, int64_t slab_stride, int64_t slab_col0,
                           int32_t layout /*mappo_wide_layout(desc, producer) of the launch that filled wide_ws*/,
                           mappo_stream_t stream);

/* ---- fused update kernels (K7 + K5 + K7-backward in ONE launch per network; r_mappo.py:91-164) --------------
 * The forward of a 32-sample tile, the loss gradient at the head and the backward pass run back to back in the
 * same wavefront: logits / values / d(logits) / d(values) never leave the CU.  Per-sample loss inputs are read
 * in buffer order through `rows` (NULL = identity), exactly like mappo_ppo_loss_fwd_bwd, whose arithmetic they
 * share.  Outputs: one gradient slab per workgroup (as mappo_mlp_backward) and per-workgroup double partial
 * sums `partials[n_slabs][4]` (actor: sum w*min(s1,s2), sum w*H, sum ratio, - ; critic: sum w_v*l, -, -, -),
 * turned into the 6 statistics by mappo_update_stats (actor_partials may be NULL when update_actor is off). */
int64_t mappo_update_partials_bytes(void);
int mappo_actor_update(const float *params, const mappo_net_desc *desc /*host*/, const float *obs,
                       const int32_t *rows, int64_t B, const float *avail /*or NULL*/, const float *actions,
                       const float *old_logp, const float *adv, const float *active,
                       const double *mb_moments /*[4]*/, const mappo_ppo_cfg *cfg /*host*/, float *slabs,
                       int64_t slab_stride, int64_t slab_col0, double *partials, float *wide_ws /*or NULL*/,
                       int32_t n_blocks /*0 = mappo_mlp_backward_slabs(B); else the grid size = slab rows written*/,
                       mappo_stream_t stream);
int mappo_critic_update(const float *params, const mappo_net_desc *desc /*host*/, const float *share_obs,
                        const int32_t *rows, int64_t B, const float *v_old, const float *returns,
                        const float *active, const float *vn_state /*[3] after update, or NULL*/,
                        const double *mb_moments /*[4]*/, const mappo_ppo_cfg *cfg /*host*/, float *slabs,
                        int64_t slab_stride, int64_t slab_col0, double *partials, float *wide_ws /*or NULL*/,
                        int32_t n_blocks, mappo_stream_t stream);
/* mappo_actor_update + mappo_critic_update in ONE launch (in_dim <= 64, shared layer_N / activation).  The networks run side
 * by side on disjoint CUs (shares proportional to their per-tile cost); each writes its own slab columns and loss partials.
 * mappo_dual_update_slabs = the slab rows / partial rows the caller provides PER NETWORK: every one of them is written by
 * the launch (a network with fewer workgroups has its remaining rows zero-filled), so the reduction runs over that count.
 * layer_N <= 1 and out_dim <= 16 take the one-wave-per-16-sample-tile kernel (csrc/mlp_upd16.h), the rest the pair kernel
 * (so does an actor with 33..64 inputs and layer_N = 1, whose 16-sample-tile layout does not fit the LDS). */
int32_t mappo_dual_update_slabs(const mappo_net_desc *actor_desc /*host*/, const mappo_net_desc *critic_desc /*host*/, int64_t B);
int mappo_actor_critic_update(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, const float *obs,
                              const float *critic_params, const mappo_net_desc *critic_desc /*host*/, const float *share_obs,
                              const int32_t *rows, int64_t B, const float *avail, const float *actions, const float *old_logp,
                              const float *adv, const float *active, const float *v_old, const float *returns,
                              const float *vn_state, const double *mb_moments, const mappo_ppo_cfg *cfg /*host*/, float *slabs,
                              int64_t slab_stride, int64_t actor_col0, int64_t critic_col0, double *actor_partials,
                              double *critic_partials, mappo_stream_t stream);
/* The work of n_jobs mappo_actor_critic_update calls — the agents of a separated run (share_policy = False) — in ONE launch.
 * A job holds exactly that call's arguments (descriptors and cfg by value); jobs may differ in in_dim, out_dim, B, rows and every
 * pointer.  The grid is the sum of the single calls' grids; every job's slab rows and loss-partial rows [0, mappo_dual_update_slabs)
 * come out bit for bit as its single call writes them (the same rows written, the same rows zero-filled).  Accepted jobs are
 * those the single call serves with the 16-sample-tile kernel: both networks feed-forward with in_dim <= 64, Discrete head with
 * out_dim <= 16, layer_N <= 1 (not the actor with 33..64 inputs and layer_N = 1: pair kernel), and all jobs agree in layer_N,
 * use_relu and use_feature_norm (the launch is one template instance).  Anything else — n_jobs outside 1..MAPPO_MAX_GROUP, a
 * NULL pointer, a wide, recurrent or pair-kernel job — returns MAPPO_EINVAL before any launch, naming the job. */
#define MAPPO_MAX_GROUP 8
typedef struct mappo_update_job {
  const float *actor_params;
  mappo_net_desc actor_desc;
  const float *obs;
  const float *critic_params;
  mappo_net_desc critic_desc;
  const float *share_obs;
  const int32_t *rows;       /* or NULL */
  int64_t B;
  const float *avail;        /* or NULL */
  const float *actions, *old_logp, *adv, *active, *v_old, *returns;
  const float *vn_state;     /* or NULL without use_valuenorm */
  const double *mb_moments;
  mappo_ppo_cfg cfg;
  float *slabs;
  int64_t slab_stride, actor_col0, critic_col0;
  double *actor_partials, *critic_partials;
} mappo_update_job;
int mappo_actor_critic_update_group(const mappo_update_job *jobs /*host [n_jobs]*/, int32_t n_jobs, mappo_stream_t stream);
/* 1 if a job with these two descriptors passes the shape checks above (jobs of one launch must also agree with each other), else 0 */
int32_t mappo_update_group_accepts(const mappo_net_desc *actor_desc /*host*/, const mappo_net_desc *critic_desc /*host*/);
/* The same two launches for a MultiDiscrete actor (limits and layout: mappo_actor_act_md; r_mappo.py:124-141 with act.py:139-152):
 * actions / old_logp are [.][K] in buffer order.  With r_j = exp(lp_j - old_lp_j) and s_j = min(r_j adv, clip(r_j) adv) the actor's
 * per-workgroup partials are {sum w sum_j s_j, sum w (1/K) sum_j H_j, sum (1/K) sum_j r_j, -}, so mappo_update_stats yields the policy
 * loss, the mean-of-heads entropy and the mean ratio over all B K entries unchanged.  Slab / partial rows: as for the Discrete
 * launches (mappo_mlp_backward_slabs / n_blocks; mappo_dual_update_slabs PER NETWORK, every one of them written). */
int mappo_actor_update_md(const float *params, const mappo_net_desc *desc /*host*/, const float *obs, const int32_t *rows, int64_t B,
                          const float *avail /*NULL*/, const int32_t *head_dims /*host*/, int32_t n_heads, const float *actions /*[.][K]*/,
                          const float *old_logp /*[.][K]*/, const float *adv, const float *active, const double *mb_moments /*[4]*/,
                          const mappo_ppo_cfg *cfg /*host*/, float *slabs, int64_t slab_stride, int64_t slab_col0, double *partials,
                          float *wide_ws /*unused (in_dim <= 64): NULL*/, int32_t n_blocks, mappo_stream_t stream);
int mappo_actor_critic_update_md(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, const float *obs,
                                 const float *critic_params, const mappo_net_desc *critic_desc /*host*/, const float *share_obs,
                                 const int32_t *rows, int64_t B, const float *avail /*NULL*/, const int32_t *head_dims /*host*/,
                                 int32_t n_heads, const float *actions, const float *old_logp, const float *adv, const float *active,
                                 const float *v_old, const float *returns, const float *vn_state, const double *mb_moments,
                                 const mappo_ppo_cfg *cfg /*host*/, float *slabs, int64_t slab_stride, int64_t actor_col0,
                                 int64_t critic_col0, double *actor_partials, double *critic_partials, mappo_stream_t stream);
int mappo_update_stats(const double *actor_partials, int32_t n_actor /*workgroups that wrote them*/,
                       const double *critic_partials, int32_t n_critic, const double *mb_moments,
                       const mappo_ppo_cfg *cfg /*host*/, double *stats /*[6]*/,
                       double *acc /*[>=4] running sums of stats[0..3] over the updates of one train(), or NULL*/,
                       mappo_stream_t stream);

/* ---- once-per-train() glue of a whole-buffer update (every epoch's minibatch is the buffer), fused ---------------------
 * mappo_train_prologue = mappo_adv_moments + mappo_minibatch_moments (rows NULL, B = n) + mappo_valuenorm_update_n + a fill, in ONE
 * launch with bit-identical results: adv [n] (raw; mappo_adv_normalize follows as its own launch), adv_moments [3],
 * mb_moments [4], and, when vn_state is not NULL, the n_epochs ValueNorm states (states_out, vn_state; the advantages use the
 * state from before the call).  zero[0..n_zero) is set to 0.0 (n_zero may be 0).  The workgroup that finishes last does the
 * one-workgroup work; `ticket` is ONE int32 word that must be 0 before the first call and is 0 again after every call (so the
 * call can be captured into a hipGraph and replayed); workspace (mappo_train_prologue_workspace_bytes) and ticket must not be
 * shared by calls that may run concurrently. */
int64_t mappo_train_prologue_workspace_bytes(int64_t n);
int mappo_train_prologue(const float *returns /*[n]*/, const float *value_preds /*[n]*/, const float *active_masks /*[n]*/,
                         float *vn_state /*[3] in/out or NULL*/, float *adv /*[n] out (raw)*/, double *adv_moments /*[3] out*/,
                         double *mb_moments /*[4] out*/, double beta, int32_t n_epochs, float *states_out /*[n_epochs][3] or NULL*/,
                         double *zero, int64_t n_zero, void *workspace, int32_t *ticket, int64_t n, mappo_stream_t stream);
/* mappo_train_epilogue = mappo_update_stats + mappo_copy_batch (same arguments, same results) in one launch. */
int mappo_train_epilogue(const double *actor_partials, int32_t n_actor, const double *critic_partials, int32_t n_critic,
                         const double *mb_moments, const mappo_ppo_cfg *cfg /*host*/, double *stats /*[6]*/, double *acc,
                         int32_t count, float *const *dst, const float *const *src, const int64_t *n_floats, mappo_stream_t stream);

/* ---- K9: recurrent layer (onpolicy/algorithms/utils/rnn.py:7-80: nn.GRU(64,64) with per-step h*mask + LayerNorm) ----
 * A recurrent network = trunk (mappo_mlp_features) -> GRU -> rnn.norm -> head.  Outside the training pass (below: the
 * mappo_gru16_* entry points) features are feature-major: featT is [64][B], B = L*Nc, column t*Nc + c (time-major over Nc
 * sequences, the order of recurrent_generator's stacked chunks, shared_buffer.py:438-474); `rows` maps column -> flat buffer row.
 *   mappo_mlp_features   trunk forward, LayerNorm output of the last layer, feature-major
 *   mappo_gru_forward    L steps from h0[h0_rows] (row-major [.][64]); head_mode 0: states only, 1: head output
 *                        out[B][A] per step, 2: sample/argmax + log-prob (rollout, L = 1)
 *   mappo_trunk_backward backward of the trunk given dxT (forward recomputed per tile, as mappo_mlp_backward) */
int mappo_mlp_features(const float *params, const mappo_net_desc *desc /*host*/, const float *x, const int32_t *rows,
                       int64_t B, float *featT /*[64][B]*/, mappo_stream_t stream);
int mappo_gru_forward(const float *params, const mappo_net_desc *desc /*host*/, const float *featT, const float *h0,
                      const int32_t *h0_rows /*[Nc] or NULL*/, const float *masks, const int32_t *rows /*[B] or NULL*/,
                      int32_t L, int32_t Nc, float *h_last /*[Nc][64] or NULL*/,
                      int32_t head_mode, float *out, const float *avail /*[B][A] or NULL*/, int32_t deterministic,
                      uint64_t seed, uint64_t counter, const uint64_t *counter_dev, float *actions, float *logp,
                      mappo_stream_t stream);
/* One rollout step (L = 1) of a recurrent actor AND critic in one launch (r_actor_critic.py:43-70 + :146-165 on the same Nc rows):
 * actions / logp [Nc] sampled from the actor's head, values [Nc] from the critic's, next states to *_h_last [Nc][64]. */
int mappo_gru_step_dual(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, const float *actor_featT /*[64][Nc]*/,
                        const float *actor_h0 /*[Nc][64]*/, float *actor_h_last, const float *critic_params,
                        const mappo_net_desc *critic_desc /*host*/, const float *critic_featT, const float *critic_h0,
                        float *critic_h_last, const float *masks /*[Nc]*/, int32_t Nc, const float *avail /*[Nc][A] or NULL*/,
                        int32_t deterministic, uint64_t seed, uint64_t counter, const uint64_t *counter_dev, float *actions,
                        float *logp, float *values, mappo_stream_t stream);
/* The same step with the trunks included: obs / share_obs rows [Nc][in_dim] instead of precomputed features —
 * mappo_mlp_features_dual + mappo_gru_step_dual in ONE launch (r_actor_critic.py:43-70,146-165 end to end).  Both networks narrow
 * (in_dim <= 64, layer_N <= 1: every wave runs the tile's trunk from registers) or both wide (65..512, up to 16 384 rows: the
 * workgroup that ran a tile's split-K trunk goes straight on to its GRU step, the GRU operands fetched under the trunk). */
int mappo_recurrent_step_dual(const float *actor_params, const mappo_net_desc *actor_desc, const float *obs,
                              const float *actor_h0, float *actor_h_last, const float *critic_params,
                              const mappo_net_desc *critic_desc, const float *share_obs, const float *critic_h0,
                              float *critic_h_last, const float *masks, int32_t Nc, const float *avail, int32_t deterministic,
                              uint64_t seed, uint64_t counter, const uint64_t *counter_dev, float *actions, float *logp,
                              float *values, mappo_stream_t stream);
/* The SMAC rollout step in ONE launch (smac_runner.py:110-151 across two consecutive steps): the insert of the env output of step
 * k - 1 into buffer slot k (what mappo_insert_smac does: slot copies, masks / active_masks / bad_masks, states x (1 - env done)) AND
 * get_actions / get_values of step k, reading that env output (obs [N*M][D], share_obs [N*M][S], avail [N*M][A] or NULL, contiguous)
 * and the states the step before returned (actor_h / critic_h [N*M][64], unmasked) in place; the row mask is derived from `dones`
 * exactly as masks[k] is.  Next states go to *_h_next (not aliasing *_h); actions / logp / values are slot k's arrays. */
typedef struct mappo_smac_slot {
  float *obs, *share_obs, *available_actions /*or NULL*/, *rewards /*slot k - 1*/, *masks, *bad_masks, *active_masks, *rnn_states,
        *rnn_states_critic;
} mappo_smac_slot;
int mappo_recurrent_rollout_step(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, const float *critic_params,
                                 const mappo_net_desc *critic_desc /*host*/, const float *obs, const float *share_obs, const float *avail,
                                 const float *rewards, int64_t rew_stride_n, int64_t rew_stride_m, const uint8_t *dones,
                                 int64_t done_stride_n, int64_t done_stride_m, const uint8_t *bad_transition /*[N*M] or NULL*/,
                                 const float *actor_h, const float *critic_h, float *actor_h_next, float *critic_h_next, int32_t N, int32_t M,
                                 int32_t deterministic, uint64_t seed, uint64_t counter, const uint64_t *counter_dev, float *actions,
                                 float *logp, float *values, const mappo_smac_slot *dst /*host*/, mappo_stream_t stream);
/* Trunk features of two networks (same layer_N / activation, in_dim <= 64) on the same B rows in one launch. */
int mappo_mlp_features_dual(const float *params_a, const mappo_net_desc *desc_a /*host*/, const float *x_a, float *featT_a,
                            const float *params_c, const mappo_net_desc *desc_c /*host*/, const float *x_c, float *featT_c,
                            int64_t B, mappo_stream_t stream);
int mappo_trunk_backward(const float *params, const mappo_net_desc *desc /*host*/, const float *x, const int32_t *rows,
                         int64_t B, const float *dxT /*[64][B]*/, float *slabs, int64_t slab_stride, int64_t slab_col0,
                         float *wide_ws /*or NULL*/, mappo_stream_t stream);

/* ---- K9, training pass on 16-sequence tiles (gru_train16.hip; rnn.py:25-79 inside r_mappo.py:91-164) -------------------------
 * One PPO update of a recurrent network on Nc sequences of L steps (time-major minibatch, column t*Nc + c) is
 *   mappo_mlp_features_seq   trunk features, tiled per (t, 16 sequences), BLOCKED per tile (in_dim <= 64 with layer_N <= 1, or in_dim 65..512
 *                            with Nc % 16 == 0; otherwise mappo_mlp_features, feature-major, with x_blocked = 0 below)
 *   mappo_gru16_forward_loss gi = W_ih x AND gh = W_hh (h mask) in one accumulator set, gates, h_t, then rnn.norm -> head -> PPO /
 *                            value loss -> their backward in the same registers: stores {h mask, r, z, n, W_hn h + b_hn, d h_t} per
 *                            step (gi and h_t never reach HBM), head + rnn.norm gradient columns of one slab row per workgroup,
 *                            loss partial sums [grid][4] (layout of mappo_actor_update's partials: mappo_update_stats reads them)
 *   mappo_gru16_backward     reverse time: d gates (in place over r, z, n, gh_n), carry = (W_hh^T d gh + d h z) mask, and
 *                            d x_t = W_ih^T d gi from the same registers (blocked over the d h component, or feature-major dxT)
 *   mappo_gru16_wgrad        dW_ih, dW_hh, db_ih, db_hh = sum over rows (d gates)^T (x | h mask) -> slab rows
 *   mappo_trunk_backward_seq backward of the trunk from the blocked d x (same shapes as mappo_mlp_features_seq; otherwise
 *                            mappo_trunk_backward with dxT)
 * scratch: mappo_gru16_scratch_floats(L, Nc) floats, [6][L][ceil(Nc/16)][4][64 lanes][4]: component c, step t, tile j, feature
 * block b; lane (n, q) holds features 16 b + 4 q + 0..3 of sequence 16 j + n (one contiguous KiB per wave access).  A blocked
 * feature array (x, d x) is one such component: mappo_gru16_blocked_floats(L, Nc).  mappo_gru16_slabs: slab rows written.
 * Write contract (tests/test_gpu_gru_matrix.py): each slab-writing kernel of the chain (the head kernel or the unsplit forward;
 * wgrad; the trunk backward — the split recurrence kernels write no slab row) writes its own columns of ONE slab row per workgroup
 * of its own grid (the grids differ; none exceeds mappo_gru16_slabs(L, Nc)) and zero-fills nothing, so rows [0, mappo_gru16_slabs)
 * of the network's column range must be zero beforehand; the partials are [forward grid][4], the forward grid being that of the
 * head kernel (split recurrence) or of the sequence kernel (unsplit) — at most mappo_gru16_slabs rows as well. */
int64_t mappo_gru16_scratch_floats(int32_t L, int32_t Nc);
int64_t mappo_gru16_blocked_floats(int32_t L, int32_t Nc);
int32_t mappo_gru16_slabs(int32_t L, int32_t Nc);
int mappo_mlp_features_seq(const float *params, const mappo_net_desc *desc /*host*/, const float *x, const int32_t *rows /*[L*Nc] or NULL*/,
                           int32_t L, int32_t Nc, float *out_blocked, mappo_stream_t stream);
int mappo_gru16_forward_loss(const float *params, const mappo_net_desc *desc /*host*/, const float *x, int32_t x_blocked, const float *h0,
                             const int32_t *h0_rows /*[Nc] or NULL*/, const float *masks, const int32_t *rows /*[L*Nc] or NULL*/,
                             int32_t L, int32_t Nc, int32_t head /*1 actor, 2 critic*/, const float *avail, const float *actions,
                             const float *old_logp, const float *adv, const float *active, const float *v_old, const float *returns,
                             const float *vn_state, const double *mb_moments, const mappo_ppo_cfg *cfg /*host*/, float *scratch,
                             float *slabs, int64_t slab_stride, int64_t slab_col0, double *partials, mappo_stream_t stream);
int mappo_gru16_backward(const float *params, const mappo_net_desc *desc /*host*/, const float *masks, const int32_t *rows, int32_t L,
                         int32_t Nc, float *scratch, float *dxT /*[64][L*Nc] feature-major, or NULL: blocked, in scratch component 5*/,
                         mappo_stream_t stream);
int mappo_gru16_wgrad(const mappo_net_desc *desc /*host*/, const float *x, int32_t x_blocked, const float *scratch, int32_t L, int32_t Nc,
                      float *slabs, int64_t slab_stride, int64_t slab_col0, mappo_stream_t stream);
int mappo_trunk_backward_seq(const float *params, const mappo_net_desc *desc /*host*/, const float *x, const int32_t *rows, int32_t L,
                             int32_t Nc, const float *dx_blocked, float *slabs, int64_t slab_stride, int64_t slab_col0,
                             float *wide_ws /*in_dim > 64 (then Nc % 16 == 0): mappo_wide_workspace_floats(L*Nc) floats, followed by
                                              mappo_wide_l1_backward with the layout of MAPPO_PRODUCER_TRUNK_BACKWARD; else NULL*/,
                             mappo_stream_t stream);

/* ---- K10/K11: slab reduction, global-norm clip, Adam (r_mappo.py:143-148,157-162; torch Adam) -------
 * The flat gradient covers `n_seg` parameter segments (actor, critic); norms/clip/lr are per segment.
 * opt_hyper (device floats, per segment, stride 8): {lr, beta1, beta2, eps, weight_decay, max_grad_norm,
 * use_clip, enabled}.  opt_step: device int32 per segment (Adam's `step`, incremented by the call).
 * grad_norms out: device floats per segment (pre-clip norm, what train_info logs). */
int64_t mappo_optim_workspace_bytes(int64_t P);
int mappo_slab_reduce(const float *slabs, int32_t n_slabs, int64_t slab_stride, int64_t P,
                      float *grad /*[P] out*/, mappo_stream_t stream);
int mappo_clip_adam(float *params, const float *grad, float *exp_avg, float *exp_avg_sq,
                    const int64_t *seg_bounds /*host, [n_seg+1], multiples of 256*/, int32_t n_seg,
                    const float *opt_hyper, int32_t *opt_step, float *grad_norms,
                    double *norm_acc /*[n_seg] running sums of the norms, or NULL*/, void *workspace,
                    mappo_stream_t stream);
/* mappo_slab_reduce + mappo_clip_adam in two launches instead of four (single-process training: nothing has to happen
 * between the reduction and the optimizer step).  Same arithmetic; the squared-norm partials are taken per 128
 * entries inside the reduction.  workspace: mappo_optim_workspace_bytes(P) bytes. */
int mappo_reduce_clip_adam(const float *slabs, int32_t n_slabs, int64_t slab_stride, float *params, float *grad /*out*/,
                           float *exp_avg, float *exp_avg_sq, const int64_t *seg_bounds /*host [n_seg+1]*/, int32_t n_seg,
                           const float *opt_hyper, int32_t *opt_step, float *grad_norms, double *norm_acc /*or NULL*/,
                           void *workspace, mappo_stream_t stream);
/* n_jobs mappo_reduce_clip_adam calls (1..MAPPO_MAX_GROUP; a job holds that call's arguments, the workspace is per job) in the
 * same TWO launches: within a job the same reduction order over slab rows, the same norm, clip, Adam and norm_acc, so params,
 * grad, moments, opt_step and grad_norms equal the single call's bit for bit. */
typedef struct mappo_optim_job {
  const float *slabs;
  int32_t n_slabs;
  int64_t slab_stride;
  float *params, *grad, *exp_avg, *exp_avg_sq;
  int64_t seg_bounds[5];     /* [n_seg + 1], increasing multiples of 256 from 0 */
  int32_t n_seg;             /* 1..4 */
  const float *opt_hyper;
  int32_t *opt_step;
  float *grad_norms;
  double *norm_acc;          /* or NULL */
  void *workspace;           /* mappo_optim_workspace_bytes(seg_bounds[n_seg]) bytes */
} mappo_optim_job;
int mappo_reduce_clip_adam_group(const mappo_optim_job *jobs /*host [n_jobs]*/, int32_t n_jobs, mappo_stream_t stream);

/* GPU-vectorised MPE simple_spread (csrc/mpe_env.hip): N environments x M agents x L landmarks, one launch per
 * step.  Replaces World.step / Scenario.reward / Scenario.observation / MultiAgentEnv.step + the vec-env's reset-on-done
 * (onpolicy/envs/mpe/core.py:207-322, scenarios/simple_spread.py:32-103, environment.py:117-256, env_wrappers.py:146-152).
 * State is caller-owned device memory: agent_pos / agent_vel [N][M][2] and landmark_pos [N][L][2] in float64 (the reference's
 * NumPy dtype), tstep [N] int32, episode [N] int64 (reset counter = Philox counter).  Outputs: obs [N][M][4+2L+4(M-1)] fp32,
 * rewards [N][M] fp32 (shared reward), dones [N][M] bool bytes.  action_mode 0: actions = the reference's actions_env
 * [N][M][5] (one-hot, or any row of five weights such as probabilities: the force is 5 * [a1 - a2, a3 - a4] of what is given,
 * environment.py:223-235); 1: action indices [N][M] as fp32 (the buffer's own format).  An index is truncated towards zero to an
 * int and moves the agent only if that int is 1..4: 2.7 acts as 2, and every other value (-3, 9, 0) as 0, no force.  There is no
 * clamp to the nearest move (simple_tag's kernel clamps; this one does not); the sampler only produces 0..4.  An environment whose
 * episode ends is reset inside the same launch and returns the reset observation, as DummyVecEnv / SubprocVecEnv do. */
int mappo_mpe_spread_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode, float *obs,
                           int32_t N, int32_t M, int32_t L, uint64_t seed, mappo_stream_t stream);
int mappo_mpe_spread_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                          const float *actions, int32_t action_mode, float *obs, float *rewards, uint8_t *dones, int32_t N, int32_t M,
                          int32_t L, int32_t episode_length, uint64_t seed, mappo_stream_t stream);
/* One launch per rollout EPISODE on the environment above, env steps included (csrc/rollout_spread.h): what T x
 * (mappo_rollout_step + mappo_mpe_spread_step with action_mode 1) + the bootstrap mappo_rollout_step do, bit for bit
 * (mpe_runner.py:22-40,95-139 collect / env.step / insert; core.py:207-322, simple_spread.py:32-103, environment.py:117-256 the step).
 * Per step t < T: actor on the observation rows of step t (step 0: obs_buf slot 0) with counter + t (+ *counter_dev) and row
 * index n*M + m -> actions / logp [T][B]; the environments step in float64 on the sampled indices from the state in agent_pos /
 * agent_vel / landmark_pos / tstep / episode (reset-on-done after env_episode_length steps, Philox stream (env_seed, episode, n));
 * obs -> obs_buf / share_buf slot t + 1 ([T+1][B][in_dim]), rewards -> rew_buf [T][B] slot t, 1 - done -> mask_buf [T+1][B] slot
 * t + 1.  Critic on the share rows of step t <= T -> values [T][B], step T -> next_values [B].  The five state arrays are stored
 * back at the end, so the environment continues in either path.  B = N*M rows; M, L <= 8; actor in_dim = 4 + 2L + 4(M-1), out_dim 5;
 * critic in_dim = M * in_dim (centralized) or in_dim; both <= 64, same layer_N and activation; not recurrent; no available
 * actions.  Validates on the host before the launch. */
int mappo_rollout_episode_spread(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, const float *critic_params,
                                 const mappo_net_desc *critic_desc /*host*/, int32_t T, int32_t N, int32_t M, int32_t L,
                                 int32_t env_episode_length, uint64_t env_seed, double *agent_pos, double *agent_vel,
                                 double *landmark_pos, int32_t *tstep, int64_t *episode, int32_t deterministic, uint64_t seed,
                                 uint64_t counter, const uint64_t *counter_dev, float *obs_buf, float *share_buf, float *rew_buf,
                                 float *mask_buf, float *actions /*[T][B]*/, float *logp /*[T][B]*/, float *values /*[T][B]*/,
                                 float *next_values /*[B]*/, int32_t centralized, mappo_stream_t stream);
/* The same episode for a RECURRENT shared policy (csrc/rollout_spread_rec.h): what T x (mappo_recurrent_step_dual +
 * mappo_mpe_spread_step with action_mode 1 + mappo_insert_mpe_rnn) do, bit for bit while the stepwise step is the fused one
 * (N*M <= 1024 rows).  Per step t < T: actor and critic (trunk, GRU step on rnn_states[t] * mask_buf[t], rnn.norm, head) on the rows
 * of step t (step 0: slot 0 of obs_buf / share_buf / rnn_states / rnn_states_critic / mask_buf) -> actions / logp / values [T][B],
 * sampling with counter + t (+ *counter_dev) and the row index; the environments step as above; obs / share / 1 - done -> slot t + 1,
 * rewards -> slot t, next states * (1 - done) -> rnn_states / rnn_states_critic [T+1][B][64] slot t + 1.  The bootstrap value of
 * slot T is NOT computed (the caller takes it through mappo_mlp_features + mappo_gru_forward, as the stepwise path does).
 * Limits, each refused with a message that names it: both descriptors recurrent; both in_dim <= 64; layer_N <= 1; same layer_N and
 * activation; actor out_dim 5 and in_dim = 4 + 2L + 4(M-1); critic out_dim 1 and in_dim = M * in_dim (centralized) or in_dim;
 * M, L in 1..8; no available actions.  Validates on the host before the launch. */
int mappo_rollout_episode_spread_recurrent(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, const float *critic_params,
                                           const mappo_net_desc *critic_desc /*host*/, int32_t T, int32_t N, int32_t M, int32_t L,
                                           int32_t env_episode_length, uint64_t env_seed, double *agent_pos, double *agent_vel,
                                           double *landmark_pos, int32_t *tstep, int64_t *episode, int32_t deterministic, uint64_t seed,
                                           uint64_t counter, const uint64_t *counter_dev, float *obs_buf, float *share_buf, float *rew_buf,
                                           float *mask_buf, float *actions /*[T][B]*/, float *logp /*[T][B]*/, float *values /*[T][B]*/,
                                           float *rnn_states /*[T+1][B][64]*/, float *rnn_states_critic /*[T+1][B][64]*/,
                                           int32_t centralized, mappo_stream_t stream);
/* One launch per EVALUATION episode on the same environment (csrc/eval_spread.h; mpe_runner.py:141-183 eval: act, env.step, sum of
 * the step rewards): only the policy acting — no critic, no buffer.  Per step t < T: actor on the observation rows of the current
 * state with counter + t (+ *counter_dev) and row index n*M + m, argmax (deterministic) or a sample; the environments step in
 * float64 as above, reset-on-done included.  returns [N][M]: acc = 0; acc += r_t for t = 0 .. T-1, in fp32, per row.  actions:
 * [T][N*M] or NULL.  The five state arrays are advanced in place; nothing else is written.  Given the same parameters, state, seed
 * and counter, the actions and the state are bit-identical to mappo_rollout_episode_spread's.
 * Limits, each refused with a message that names it: not recurrent; in_dim <= 64 and = 4 + 2L + 4(M-1); layer_N <= 1; out_dim 5;
 * T, N, env_episode_length >= 1; M, L in 1..8.  Validates on the host before the launch; no allocation, no host sync. */
int mappo_eval_episode_spread(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, int32_t T, int32_t N, int32_t M,
                              int32_t L, int32_t env_episode_length, uint64_t env_seed, double *agent_pos, double *agent_vel,
                              double *landmark_pos, int32_t *tstep, int64_t *episode, int32_t deterministic, uint64_t seed,
                              uint64_t counter, const uint64_t *counter_dev, float *returns /*[N][M]*/, float *actions /*[T][N*M] or NULL*/,
                              mappo_stream_t stream);
/* One launch per rollout EPISODE of a RECURRENT shared policy on SMAC-shaped env output (csrc/rollout_smac_rec.h;
 * smac_runner.py:110-151 collect / insert over a whole episode): what mappo_recurrent_step_dual on slot 0, then for k = 1 .. T-1
 * mappo_recurrent_rollout_step (insert of env output k - 1 into slot k + the step on it), then mappo_insert_smac of env output T - 1
 * into slot T do, bit for bit while the stepwise step is the fused one (N*M <= 1024 rows).  The env output of all T steps is an
 * input (the pool of mappo_synth_smac_pool: an env that ignores the actions): env_obs [T][N*M][D], env_share_obs [T][N*M][S],
 * env_avail [T][N*M][A] or NULL (then avail_buf is NULL too), env_rewards [T][N] (shared by an env's agents), env_dones [T][N*M]
 * bool bytes, env_bad_transition [N*M] bool bytes or NULL (constant over the episode).  Per step k < T: actor and critic (trunk,
 * GRU step on rnn_states[k] * mask_buf[k], rnn.norm, head) on the rows of slot k -> actions / logp / values [T][B], B = N*M, the
 * actor's logits masked by available_actions[k] (-1e10), sampling with counter + k (+ *counter_dev) and the buffer row; then
 * env output k -> slot k + 1 of obs_buf / share_buf / avail_buf ([T+1][B][D | S | A]), rewards -> rew_buf [T][B] slot k,
 * mask_buf[k+1] = 1 - dones_env (all agents of the env done), active_mask_buf[k+1] = dones_env ? 1 : 1 - done, bad_mask_buf[k+1] =
 * 1 - bad_transition (all [T+1][B]), next states * (1 - dones_env) -> rnn_states / rnn_states_critic [T+1][B][64] slot k + 1
 * (smac_runner.py:129-151).  centralized 0: the critic reads obs (in_dim = the actor's) and share_buf receives obs; env_share_obs
 * is ignored.  The bootstrap value of slot T is NOT computed (the caller takes it, as the stepwise path does).
 * Limits, each refused with a message that names it: both descriptors recurrent; both in_dim <= 64 (wider inputs step one launch at
 * a time); layer_N <= 1; same layer_N and activation; actor out_dim <= MAPPO_MAX_ACTIONS; critic out_dim 1; 1 <= M <= 16; T >= 1;
 * no NULL among the required arrays.  Validates on the host before the launch. */
int mappo_rollout_episode_smac_recurrent(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, const float *critic_params,
                                         const mappo_net_desc *critic_desc /*host*/, int32_t T, int32_t N, int32_t M, const float *env_obs,
                                         const float *env_share_obs, const float *env_avail /*or NULL*/, const float *env_rewards,
                                         const uint8_t *env_dones, const uint8_t *env_bad_transition /*or NULL*/, int32_t deterministic,
                                         uint64_t seed, uint64_t counter, const uint64_t *counter_dev, float *obs_buf, float *share_buf,
                                         float *avail_buf /*or NULL*/, float *rew_buf, float *mask_buf, float *bad_mask_buf,
                                         float *active_mask_buf, float *rnn_states, float *rnn_states_critic, float *actions /*[T][B]*/,
                                         float *logp /*[T][B]*/, float *values /*[T][B]*/, int32_t centralized, mappo_stream_t stream);

/* GPU-vectorised MPE simple_reference (csrc/mpe_ref_env.hip, device functions in csrc/mpe_ref_core.h): N environments of
 * the scenario's fixed shape — 2 agents, 3 landmarks, dim_c = 10, action space MultiDiscrete([[0, 4], [0, 9]]) — one launch per step.
 * Replaces MultiAgentEnv.step / _set_action (environment.py:117-256, MultiDiscrete split :198-205), World.step (core.py:207-287; the
 * agents do not collide), Scenario.reset_world / reward / observation (scenarios/simple_reference.py:34-97) + the vec-env's
 * reset-on-done (env_wrappers.py:146-152).  State is caller-owned device memory: agent_pos / agent_vel [N][2][2] and landmark_pos
 * [N][3][2] in float64, goal [N][2] int32 (the landmark index of each agent's goal_b), tstep [N] int32, episode [N] int64 (reset
 * counter = Philox counter).  The communication state is not stored: the step that sets it writes it into the observations.
 * Outputs: obs [N][2][21] fp32 = [vel (2), landmarks - pos (6), colour of the own goal landmark (3), the other agent's c (10)],
 * rewards [N][2] fp32 (both agents receive r_0 + r_1, r_i = -|pos(other agent) - landmark[goal_i]|^2), dones [N][2] bool bytes.
 * action_mode 0: actions = the reference's actions_env [N][2][15] (move one-hot / probabilities [5], then c [10] taken verbatim);
 * 1: head indices [N][2][2] as fp32 (the buffer's own K-wide action columns; move 1/2/3/4 = +x/-x/+y/-y, c = one-hot of the second).
 * Physics in float64 with contraction off: obs and rewards EQUAL the fp32 cast of the reference's float64 values.  An environment
 * whose episode ends (tstep >= episode_length) is reset inside the same launch and returns the reset observation (c = 0).
 * Reset draws: Philox stream (seed, episode), 64-bit uniform number 16 n + k of environment n — k = 2 i, 2 i + 1: position of agent
 * i in U(-1,1); k = 4 + 2 l, 5 + 2 l: position of landmark l in 0.8 U(-1,1); k = 10 + i: goal of agent i = min(2, floor(3 u)),
 * u in [0,1); k = 12..15 unused.  Both validate on the host and name the fault: N >= 1, non-null pointers, action_mode 0 or 1,
 * episode_length >= 1. */
int mappo_mpe_reference_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                              int64_t *episode, float *obs, int32_t N, uint64_t seed, mappo_stream_t stream);
int mappo_mpe_reference_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                             int64_t *episode, const float *actions, int32_t action_mode, float *obs, float *rewards, uint8_t *dones,
                             int32_t N, int32_t episode_length, uint64_t seed, mappo_stream_t stream);
/* One launch per rollout EPISODE on the environment above, env steps included (csrc/rollout_reference.h): what T x
 * (mappo_rollout_step_md + mappo_mpe_reference_step with action_mode 1) + the bootstrap mappo_rollout_step do, bit for bit.
 * Per step t < T: actor on the observation rows of step t (step 0: obs_buf slot 0), head k of row i = 2 n + m sampled with counter
 * + t (+ *counter_dev) and Philox index (k << 32) | i -> actions / logp [T][B][2]; the environments step in float64 on the sampled
 * indices (reset-on-done after env_episode_length steps); obs -> obs_buf / share_buf slot t + 1, rewards -> rew_buf [T][B] slot t,
 * 1 - done -> mask_buf [T+1][B] slot t + 1.  Critic on the share rows of step t <= T -> values [T][B], step T -> next_values [B].
 * The six state arrays are stored back at the end, so the environment continues in either path.  B = 2 N rows.  Host checks, each
 * named in the error: head_dims exactly (5, 10); actor in_dim 21, out_dim 15; both networks in_dim <= 64; the limits of the
 * mappo_*_md entry points (layer_N <= 1, not recurrent); critic in_dim 42 (centralized) or 21, out_dim 1; same layer_N and
 * activation; T, N, env_episode_length >= 1; non-null pointers. */
int mappo_rollout_episode_reference(const float *actor_params, const mappo_net_desc *actor_desc /*host*/, const float *critic_params,
                                    const mappo_net_desc *critic_desc /*host*/, const int32_t *head_dims /*host [n_heads]*/,
                                    int32_t n_heads, int32_t T, int32_t N, int32_t env_episode_length, uint64_t env_seed,
                                    double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                                    int64_t *episode, int32_t deterministic, uint64_t seed, uint64_t counter,
                                    const uint64_t *counter_dev, float *obs_buf, float *share_buf, float *rew_buf, float *mask_buf,
                                    float *actions /*[T][B][2]*/, float *logp /*[T][B][2]*/, float *values /*[T][B]*/,
                                    float *next_values /*[B]*/, int32_t centralized, mappo_stream_t stream);

/* GPU-vectorised MPE simple_speaker_listener (csrc/mpe_comm_env.hip, device functions in csrc/mpe_comm_core.h): N environments of the
 * scenario's fixed shape — agent 0 the SPEAKER (does not move; observes the goal landmark's colour, 3 features; Discrete(3): the
 * symbol it says), agent 1 the LISTENER (silent; observes velocity 2, the 3 landmarks relative to itself 6, the speaker's symbol 3 =
 * 11 features; Discrete(5)), 3 landmarks — one launch per step.  Replaces MultiAgentEnv.step / _set_action (environment.py:117-256),
 * World.step (core.py:207-287; nothing collides), Scenario.reset_world / reward / observation
 * (scenarios/simple_speaker_listener.py:38-98) + the vec-env's reset-on-done (env_wrappers.py:146-152).  State is caller-owned device
 * memory: listener_pos / listener_vel [N][2] and landmark_pos [N][3][2] in float64, goal [N] int32 (the landmark index of the
 * speaker's goal_b), symbol [N] int32 (what the channel holds: 0..2, or -1 for none after a reset), tstep [N] int32, episode [N]
 * int64 (reset counter = Philox counter).  The speaker's own position and velocity are neither observed nor rewarded and are not
 * kept.  Outputs: obs_speaker [N][3], obs_listener [N][11] fp32 (the listener hears the symbol said in the same step; zeros after a
 * reset), rewards [N][2] fp32 (collaborative: both agents receive the sum over the agents, 2 x -|listener - goal landmark|^2), dones
 * [N][2] bool bytes.  action_mode 0: the reference's one-hots / probabilities, actions_speaker [N][3] (taken verbatim as c) and
 * actions_listener [N][5]; 1: indices as fp32, actions_speaker = [N][2] (symbol, move; a symbol outside 0..2 is clamped, in the state and in the observation alike), actions_listener unused (may be NULL; move
 * 1/2/3/4 = +x/-x/+y/-y).  Physics in float64 with contraction off: obs and rewards EQUAL the fp32 cast of the reference's float64
 * values.  An environment whose episode ends (tstep >= episode_length) is reset inside the same launch and returns the reset
 * observation.  Reset draws: Philox stream (seed, episode), 64-bit uniform number 16 n + k of environment n — k = 0, 1: listener
 * position in U(-1,1); k = 2 + 2 l, 3 + 2 l: position of landmark l in U(-1,1); k = 8: goal = min(2, floor(3 u)), u in [0,1);
 * k = 9..15 unused.  Both validate on the host and name the fault: N >= 1, non-null pointers, action_mode 0 or 1,
 * episode_length >= 1. */
int mappo_mpe_comm_reset(double *listener_pos, double *listener_vel, double *landmark_pos, int32_t *goal, int32_t *symbol,
                         int32_t *tstep, int64_t *episode, float *obs_speaker, float *obs_listener, int32_t N, uint64_t seed,
                         mappo_stream_t stream);
int mappo_mpe_comm_step(double *listener_pos, double *listener_vel, double *landmark_pos, int32_t *goal, int32_t *symbol,
                        int32_t *tstep, int64_t *episode, const float *actions_speaker, const float *actions_listener,
                        int32_t action_mode, float *obs_speaker, float *obs_listener, float *rewards, uint8_t *dones, int32_t N,
                        int32_t episode_length, uint64_t seed, mappo_stream_t stream);
/* One agent of the separated runner's episode launches below (mappo_rollout_episode_comm, mappo_rollout_episode_adversary): its two networks, its sampling seed and counter word and the arrays of its SeparatedReplayBuffer (contiguous;
 * rows = environments): obs_buf [T+1][N][D_m], share_buf [T+1][N][S_m], rew_buf [T][N], mask_buf [T+1][N], actions / logp / values
 * [T][N] (values: slots 0..T-1 of value_preds), next_values [N]. */
typedef struct mappo_comm_agent {
  const float *actor_params, *critic_params;
  mappo_net_desc actor_desc, critic_desc;
  uint64_t seed;
  const uint64_t *counter_dev;   /* device word added to `counter` for this agent's draws, or NULL */
  float *obs_buf, *share_buf, *rew_buf, *mask_buf, *actions, *logp, *values, *next_values;
} mappo_comm_agent;
/* One launch per rollout EPISODE on the environment above, env steps included, for the SEPARATED runner (csrc/rollout_comm.h): what
 * T x (one mappo_rollout_step per agent + mappo_mpe_comm_step with action_mode 1 + the agents' inserts) + one bootstrap
 * mappo_rollout_step per agent do, bit for bit.  Per step t < T: agent m's actor on its observation rows of step t (step 0: obs_buf
 * slot 0), row n sampled with (agent's seed, counter + t (+ the agent's *counter_dev), Philox index n) -> actions / logp slot t; the environments
 * step in float64 on the sampled indices (reset-on-done after env_episode_length steps); each agent's observation -> its obs_buf
 * slot t + 1, its share row (centralized: speaker's 3 then listener's 11 = 14; else its own observation) -> share_buf slot t + 1,
 * the shared reward -> rew_buf slot t, 1 - done -> mask_buf slot t + 1.  Each critic on its share rows of step t <= T -> values,
 * step T -> next_values.  The seven state arrays are stored back at the end, so the environment continues in either path.  Host
 * checks, each named in the error: non-null descriptors; not recurrent; layer_N <= 1; speaker actor in 3 / out 3, listener actor in
 * 11 / out 5; critics out 1 and in 14 (centralized) or the agent's own in_dim; the same layer_N and activation in all four
 * networks; T, N, env_episode_length >= 1; non-null pointers. */
int mappo_rollout_episode_comm(const mappo_comm_agent *speaker /*host*/, const mappo_comm_agent *listener /*host*/, int32_t T,
                               int32_t N, int32_t env_episode_length, uint64_t env_seed, double *listener_pos, double *listener_vel,
                               double *landmark_pos, int32_t *goal, int32_t *symbol, int32_t *tstep, int64_t *episode,
                               int32_t deterministic, uint64_t counter, int32_t centralized,
                               mappo_stream_t stream);

/* GPU-vectorised MPE simple_adversary, "physical deception" (csrc/mpe_ragged_env.hip, device functions in csrc/mpe_adv_core.h): N
 * environments of the fixed shape num_agents = 3 — agent 0 the ADVERSARY (observes the 2 landmarks relative to itself 4, the two
 * others relative to itself 4 = 8 features; it is not told which landmark is the goal), agents 1 and 2 the GOOD agents (the goal
 * landmark relative to themselves 2, then the same 8 = 10 features), 2 landmarks; every agent moves, Discrete(5); nobody speaks,
 * nothing collides — one launch per step.  "Others" are in world-agent order, skipping the agent itself.  Replaces
 * MultiAgentEnv.step / _set_action (environment.py:117-256: u = (a1 - a2, a3 - a4) * 5, accel is None), World.step (core.py:207-287:
 * no environment forces, damping 0.25, dt 0.1, mass 1, no speed clamp), Scenario.reset_world / reward / observation
 * (scenarios/simple_adversary.py:36-137) + the vec-env's reset-on-done (env_wrappers.py:146-152).  State is caller-owned device
 * memory: agent_pos / agent_vel [N][3][2] and landmark_pos [N][2][2] in float64, goal [N] int32 (the landmark index of every
 * agent's goal_a), tstep [N] int32, episode [N] int64 (reset counter = Philox counter).  Outputs: obs_adversary [N][8], obs_good1 /
 * obs_good2 [N][10] fp32; rewards [N][3] fp32, ONE PER AGENT and never summed (world.collaborative is not set,
 * environment.py:49-50,142): the adversary -|p_adv - p_goal|^2 (no square root), each good agent the same
 * -min over the good agents of |p - p_goal| + |p_adv - p_goal| (square roots); dones [N][3] bool bytes.  action_mode 0: the
 * reference's one-hots / probabilities, actions [N][3][5]; 1: indices as fp32, actions [N][3], clamped to 0..4 (1/2/3/4 =
 * +x/-x/+y/-y).  Physics in float64 with contraction off and a correctly rounded sqrt: obs and rewards EQUAL the fp32 cast of the
 * reference's float64 values.  An environment whose episode ends (tstep >= episode_length) is reset inside the same launch and
 * returns the reset observation.  Reset draws: Philox stream (seed, episode), 64-bit uniform number 16 n + k of environment n —
 * k = 2 a, 2 a + 1: position of agent a in U(-1,1); k = 6 + 2 l, 7 + 2 l: position of landmark l in U(-1,1); k = 10: goal =
 * min(1, floor(2 u)), u in [0,1); k = 11..15 unused; velocities start at zero.  Both validate on the host and name the fault:
 * num_agents == 3 (the only shape built), N >= 1, non-null pointers, action_mode 0 or 1, episode_length >= 1. */
int mappo_mpe_adversary_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                              int64_t *episode, float *obs_adversary, float *obs_good1, float *obs_good2, int32_t N,
                              int32_t num_agents, uint64_t seed, mappo_stream_t stream);
int mappo_mpe_adversary_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                             int64_t *episode, const float *actions, int32_t action_mode, float *obs_adversary, float *obs_good1,
                             float *obs_good2, float *rewards, uint8_t *dones, int32_t N, int32_t num_agents,
                             int32_t episode_length, uint64_t seed, mappo_stream_t stream);
/* One launch per rollout EPISODE on the environment above, env steps included, for the SEPARATED runner
 * (csrc/rollout_sep_img.h): what T x (one mappo_rollout_step per agent + mappo_mpe_adversary_step with action_mode 1 + the
 * agents' inserts) + one bootstrap mappo_rollout_step per agent do, bit for bit.  agents: the three mappo_comm_agent above
 * (adversary, good agent 1, good agent 2).  Per step t < T: agent m's actor on its observation rows of step t (step 0: obs_buf
 * slot 0), row n sampled with (agent's seed, counter + t (+ the agent's *counter_dev), Philox index n) -> actions / logp slot t;
 * the environments step in float64 on the sampled indices (reset-on-done after env_episode_length steps); each agent's
 * observation -> its obs_buf slot t + 1, its share row (centralized: the three observations side by side, 8 | 10 | 10 = 28; else
 * its own observation) -> share_buf slot t + 1, its OWN reward -> rew_buf slot t, 1 - done -> mask_buf slot t + 1.  Each critic on
 * its share rows of step t <= T -> values, step T -> next_values.  The six state arrays are stored back at the end, so the
 * environment continues in either path.  Host checks, each named in the error: non-null descriptors; not recurrent; layer_N <= 1;
 * actors in 8 / 10 / 10 and out 5; critics out 1 and in 28 (centralized) or the agent's own in_dim; the same layer_N and
 * activation in all six networks; T, N, env_episode_length >= 1; non-null pointers. */
int mappo_rollout_episode_adversary(const mappo_comm_agent *agents /*host, [3]*/, double *agent_pos, double *agent_vel,
                                    double *landmark_pos, int32_t *goal, int32_t *tstep, int64_t *episode, int32_t T, int32_t N,
                                    int32_t env_episode_length, uint64_t env_seed, int32_t deterministic, uint64_t counter,
                                    int32_t centralized, mappo_stream_t stream);

/* GPU-vectorised MPE simple_tag, predator-prey (csrc/mpe_ragged_env.hip, device functions in csrc/mpe_tag_core.h): N environments of
 * the fixed shape num_adversaries = 3, num_good_agents = 1, num_landmarks = 2 (num_agents = 4) — agents 0..2 the ADVERSARIES (size
 * 0.075, accel 3, max_speed 1), agent 3 the GOOD agent (size 0.05, accel 4, max_speed 1.3), landmarks of size 0.2 that collide and
 * do not move; every agent moves, Discrete(5); nobody speaks — one launch per step.  Observation of agent m: own velocity 2, own
 * position 2, the 2 landmarks relative to it 4, the three other agents relative to it in world-agent order 6, and for an adversary
 * the good agent's velocity 2: 16 | 16 | 16 | 14 features.  Replaces MultiAgentEnv.step / _set_action (environment.py:117-256:
 * u = (a1 - a2, a3 - a4) * accel), World.step (core.py:207-322: action force accel * u — accel a second time —, the soft-collision
 * force between every pair of entities of which one can move, dist_min the two sizes added, pairs a < b over agents then landmarks;
 * damping 0.25; the max_speed clamp; dt 0.1; mass 1), Scenario.reset_world / reward / observation (scenarios/simple_tag.py:37-144) +
 * the vec-env's reset-on-done (env_wrappers.py:146-152).  State is caller-owned device memory: agent_pos / agent_vel [N][4][2] and
 * landmark_pos [N][2][2] in float64, tstep [N] int32, episode [N] int64 (reset counter = Philox counter).  Outputs: obs_adv0 /
 * obs_adv1 / obs_adv2 [N][16], obs_good [N][14] fp32; rewards [N][4] fp32, ONE PER AGENT and never summed (world.collaborative is not
 * set, environment.py:49-50,142): every adversary 10 x (adversaries within 0.125 of the good agent), the good agent the negative of
 * that minus the boundary penalty of |x| and of |y| (0 below 0.9, 10 (x - 0.9) below 1, else min(exp(2 x - 2), 10)); dones [N][4]
 * bool bytes.  action_mode 0: the reference's one-hots / probabilities, actions [N][4][5]; 1: indices as fp32, actions [N][4],
 * clamped to 0..4 (1/2/3/4 = +x/-x/+y/-y).  Physics in float64 with contraction off; the contact force and the penalty go through
 * the device's exp / log1p, so obs and rewards match the fp32 cast of the reference's float64 values to 1e-6 rather than to the
 * bit.  An environment whose episode ends (tstep >= episode_length) is reset inside the same launch and returns the reset
 * observation.  Reset draws: Philox stream (seed, episode), 64-bit uniform number 16 n + k of environment n — k = 2 a, 2 a + 1:
 * position of agent a in U(-1,1); k = 8 + 2 l, 9 + 2 l: position of landmark l in 0.8 U(-1,1); k = 12..15 unused; velocities start
 * at zero.  Both validate on the host and name the fault: num_agents == 4 (the only shape built), N >= 1, non-null pointers,
 * action_mode 0 or 1, episode_length >= 1. */
int mappo_mpe_tag_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                        float *obs_adv0, float *obs_adv1, float *obs_adv2, float *obs_good, int32_t N, int32_t num_agents,
                        uint64_t seed, mappo_stream_t stream);
int mappo_mpe_tag_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                       const float *actions, int32_t action_mode, float *obs_adv0, float *obs_adv1, float *obs_adv2,
                       float *obs_good, float *rewards, uint8_t *dones, int32_t N, int32_t num_agents, int32_t episode_length,
                       uint64_t seed, mappo_stream_t stream);
/* One launch per rollout EPISODE on the environment above, env steps included, for the SEPARATED runner (csrc/rollout_tag.h): what
 * T x (one mappo_rollout_step per agent + mappo_mpe_tag_step with action_mode 1 + the agents' inserts) + one bootstrap
 * mappo_rollout_step per agent do, bit for bit.  agents: four mappo_comm_agent (adversaries 0, 1, 2, then the good agent).  Per step
 * t < T: agent m's actor on its observation rows of step t (step 0: obs_buf slot 0), row n sampled with (agent's seed, counter + t
 * (+ the agent's *counter_dev), Philox index n) -> actions / logp slot t; the environments step in float64 on the sampled indices
 * (reset-on-done after env_episode_length steps); each agent's observation -> its obs_buf slot t + 1, its share row (centralized:
 * the four observations side by side, 16 | 16 | 16 | 14 = 62; else its own observation) -> share_buf slot t + 1, its OWN reward ->
 * rew_buf slot t, 1 - done -> mask_buf slot t + 1.  Each critic on its share rows of step t <= T -> values, step T -> next_values.
 * The five state arrays are stored back at the end, so the environment continues in either path.  Host checks, each named in the
 * error: non-null descriptors; not recurrent; layer_N <= 1; actors in 16 / 16 / 16 / 14 and out 5; critics out 1 and in 62
 * (centralized) or the agent's own in_dim; the same layer_N and activation in all eight networks; T, N, env_episode_length >= 1;
 * non-null pointers. */
int mappo_rollout_episode_tag(const mappo_comm_agent *agents /*host, [4]*/, double *agent_pos, double *agent_vel,
                              double *landmark_pos, int32_t *tstep, int64_t *episode, int32_t T, int32_t N,
                              int32_t env_episode_length, uint64_t env_seed, int32_t deterministic, uint64_t counter,
                              int32_t centralized, mappo_stream_t stream);

/* GPU-vectorised MPE simple_push, "keep-away" (csrc/mpe_ragged_env.hip, device functions in csrc/mpe_push_core.h): N environments of
 * the fixed shape num_agents = 2, num_landmarks = 2 — agent 0 the ADVERSARY (own velocity 2, the 2 landmarks relative to itself 4,
 * the other agent relative to itself 2 = 8 features; it is not told which landmark is the goal), agent 1 the GOOD agent (own
 * velocity 2, the goal relative to itself 2, its own colour 3, the 2 landmarks relative to itself 4, the landmarks' colours 6, the
 * other agent relative to itself 2 = 19 features); both move, Discrete(5); nobody speaks; the two agents (size 0.05) collide with
 * each other, the landmarks with nothing — one launch per step.  Replaces MultiAgentEnv.step / _set_action (environment.py:117-256:
 * u = (a1 - a2, a3 - a4) * 5, accel is None), World.step (core.py:207-322: the soft-collision force between the two agents,
 * dist_min 0.1, damping 0.25, dt 0.1, mass 1, no speed clamp), Scenario.reset_world / reward / observation
 * (scenarios/simple_push.py:42-107) + the vec-env's reset-on-done (env_wrappers.py:146-152).  Colours are the reference's float64
 * sums cast to fp32: landmark k is 0.1 everywhere with [k + 1] += 0.8, the good agent 0.25 everywhere with [goal + 1] += 0.5.  State
 * is caller-owned device memory: agent_pos / agent_vel [N][2][2] and landmark_pos [N][2][2] in float64, goal [N] int32 (the
 * landmark index of both agents' goal_a), tstep [N] int32, episode [N] int64 (reset counter = Philox counter).  Outputs:
 * obs_adversary [N][8], obs_good [N][19] fp32; rewards [N][2] fp32, ONE PER AGENT and never summed (world.collaborative is not set,
 * environment.py:49-50,142): the adversary |p_good - p_goal| - |p_goal - p_adv|, the good agent -|p_good - p_goal|; dones [N][2]
 * bool bytes.  action_mode 0: the reference's one-hots / probabilities, actions [N][2][5]; 1: indices as fp32, actions [N][2],
 * clamped to 0..4 (1/2/3/4 = +x/-x/+y/-y).  Physics in float64 with contraction off; the contact force goes through the device's
 * exp / log1p, so obs and rewards are held to 1e-6 of the fp32 cast of the reference's float64 values rather than to the bit.  An
 * environment whose episode ends (tstep >= episode_length) is reset inside the same launch and returns the reset observation.
 * Reset draws: Philox stream (seed, episode), 64-bit uniform number 16 n + k of environment n — k = 2 a, 2 a + 1: position of
 * agent a in U(-1,1); k = 4 + 2 l, 5 + 2 l: position of landmark l in 0.8 U(-1,1); k = 8: goal = min(1, floor(2 u)), u in [0,1);
 * k = 9..15 unused; velocities start at zero.  Both validate on the host and name the fault: num_agents == 2 (the only shape
 * built), N >= 1, non-null pointers, action_mode 0 or 1, episode_length >= 1. */
int mappo_mpe_push_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                         int64_t *episode, float *obs_adversary, float *obs_good, int32_t N, int32_t num_agents, uint64_t seed,
                         mappo_stream_t stream);
int mappo_mpe_push_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *goal, int32_t *tstep,
                        int64_t *episode, const float *actions, int32_t action_mode, float *obs_adversary, float *obs_good,
                        float *rewards, uint8_t *dones, int32_t N, int32_t num_agents, int32_t episode_length, uint64_t seed,
                        mappo_stream_t stream);
/* One launch per rollout EPISODE on the environment above, env steps included, for the SEPARATED runner (csrc/rollout_push.h): what
 * T x (one mappo_rollout_step per agent + mappo_mpe_push_step with action_mode 1 + the agents' inserts) + one bootstrap
 * mappo_rollout_step per agent do, bit for bit.  agents: two mappo_comm_agent (the adversary, then the good agent).  Per step
 * t < T: agent m's actor on its observation rows of step t (step 0: obs_buf slot 0), row n sampled with (agent's seed, counter + t
 * (+ the agent's *counter_dev), Philox index n) -> actions / logp slot t; the environments step in float64 on the sampled indices
 * (reset-on-done after env_episode_length steps); each agent's observation -> its obs_buf slot t + 1, its share row (centralized:
 * the two observations side by side, 8 | 19 = 27; else its own observation) -> share_buf slot t + 1, its OWN reward -> rew_buf
 * slot t, 1 - done -> mask_buf slot t + 1.  Each critic on its share rows of step t <= T -> values, step T -> next_values.  The six
 * state arrays are stored back at the end, so the environment continues in either path.  Host checks, each named in the error:
 * non-null descriptors; not recurrent; layer_N <= 1; actors in 8 / 19 and out 5; critics out 1 and in 27 (centralized) or the
 * agent's own in_dim; the same layer_N and activation in all four networks; T, N, env_episode_length >= 1; non-null pointers. */
int mappo_rollout_episode_push(const mappo_comm_agent *agents /*host, [2]*/, double *agent_pos, double *agent_vel,
                               double *landmark_pos, int32_t *goal, int32_t *tstep, int64_t *episode, int32_t T, int32_t N,
                               int32_t env_episode_length, uint64_t env_seed, int32_t deterministic, uint64_t counter,
                               int32_t centralized, mappo_stream_t stream);

/* GPU-vectorised MPE simple_crypto (csrc/mpe_ragged_env.hip, device functions in csrc/mpe_crypto_core.h): N environments of
 * num_agents = 3 and num_landmarks L = 2, 3 or 4 — agent 0 the ADVERSARY "Eve" (observes what the speaker said: 4 features), agent 1
 * the good listener "Bob" (the key, then what the speaker said: 8), agent 2 the SPEAKER "Alice" (the goal, then the key: 8).  Nobody
 * moves and nothing collides; every agent only speaks, Discrete(4) = dim_c, and landmark k's colour is the one-hot e_k of R^4 — one
 * launch per step.  Replaces MultiAgentEnv.step / _set_action (environment.py:117-256: an agent that does not move speaks its whole
 * action vector), World.step (core.py:280-287: state.c = action.c, no noise), Scenario.reset_world / reward / observation
 * (scenarios/simple_crypto.py:47-171) + the vec-env's reset-on-done (env_wrappers.py:146-152).  State is caller-owned device
 * memory, all integers: goal [N] and key [N] int32 (landmark indices 0 .. L - 1), comm [N][3] int32 (the symbol each agent last
 * said, -1: nothing said, the reference's zero vector), tstep [N] int32, episode [N] int64 (reset counter = Philox counter); the
 * positions the reference also draws enter no observation and no reward and are not kept.  Outputs: obs_eve [N][4] = Alice's c,
 * obs_bob [N][8] = e_key | Alice's c, obs_alice [N][8] = e_goal | e_key, fp32; rewards [N][3] fp32, ONE PER AGENT and never summed
 * (world.collaborative is not set, environment.py:49-50,142): with d(a) = |c_a - e_goal|^2 (0 or 2 for a one-hot; an agent whose c
 * is all zeros is skipped, as in the reference) Eve gets -d(Eve), Bob and Alice d(Eve) - d(Bob); dones [N][3] bool bytes.
 * action_mode 0: the reference's one-hots / probabilities, actions [N][3][4], the symbol is the index of the row's first maximum;
 * 1: indices as fp32, actions [N][3], clamped to 0..3.  Every value is a small integer, so obs and rewards EQUAL the fp32 cast of
 * the reference's.  An environment whose episode ends (tstep >= episode_length) is reset inside the same launch and returns the
 * reset observation (nothing said yet: Eve sees zeros, Bob e_key | 0).  Reset draws: Philox stream (seed, episode), 32-bit word
 * 2 n + k of environment n — k = 0: goal = (word * L) >> 32 in 64-bit arithmetic; k = 1: key, the same map of its own word.  Both
 * validate on the host and name the fault: num_agents == 3, num_landmarks 2..4, N >= 1, non-null pointers, action_mode 0 or 1,
 * episode_length >= 1. */
int mappo_mpe_crypto_reset(int32_t *goal, int32_t *key, int32_t *comm, int32_t *tstep, int64_t *episode, float *obs_eve,
                           float *obs_bob, float *obs_alice, int32_t N, int32_t num_agents, int32_t num_landmarks, uint64_t seed,
                           mappo_stream_t stream);
int mappo_mpe_crypto_step(int32_t *goal, int32_t *key, int32_t *comm, int32_t *tstep, int64_t *episode, const float *actions,
                          int32_t action_mode, float *obs_eve, float *obs_bob, float *obs_alice, float *rewards, uint8_t *dones,
                          int32_t N, int32_t num_agents, int32_t num_landmarks, int32_t episode_length, uint64_t seed,
                          mappo_stream_t stream);
/* One launch per rollout EPISODE on the environment above, env steps included, for the SEPARATED runner (csrc/rollout_sep_img.h):
 * what T x (one mappo_rollout_step per agent + mappo_mpe_crypto_step with action_mode 1 + the agents' inserts) + one bootstrap
 * mappo_rollout_step per agent do, bit for bit.  agents: three mappo_comm_agent (Eve, Bob, Alice).  Per step t < T: agent m's actor
 * on its observation rows of step t (step 0: obs_buf slot 0), row n sampled with (agent's seed, counter + t (+ the agent's
 * *counter_dev), Philox index n) -> actions / logp slot t; the environments step on the sampled symbols (reset-on-done after
 * env_episode_length steps); each agent's observation -> its obs_buf slot t + 1, its share row (centralized: the three
 * observations side by side, 4 | 8 | 8 = 20; else its own observation) -> share_buf slot t + 1, its OWN reward -> rew_buf slot t,
 * 1 - done -> mask_buf slot t + 1.  Each critic on its share rows of step t <= T -> values, step T -> next_values.  The five state
 * arrays are stored back at the end, so the environment continues in either path.  Host checks, each named in the error: non-null
 * descriptors; num_landmarks 2..4; not recurrent; layer_N <= 1; actors in 4 / 8 / 8 and out 4; critics out 1 and in 20
 * (centralized) or the agent's own in_dim; the same layer_N and activation in all six networks; T, N, env_episode_length >= 1;
 * non-null pointers. */
int mappo_rollout_episode_crypto(const mappo_comm_agent *agents /*host, [3]*/, int32_t *goal, int32_t *key, int32_t *comm,
                                 int32_t *tstep, int64_t *episode, int32_t T, int32_t N, int32_t num_landmarks,
                                 int32_t env_episode_length, uint64_t env_seed, int32_t deterministic, uint64_t counter,
                                 int32_t centralized, mappo_stream_t stream);

/* GPU-vectorised MPE simple_world_comm (csrc/mpe_world_comm_env.hip, device functions in csrc/mpe_world_comm_core.h): N environments
 * of the fixed shape num_adversaries = 4, num_good_agents = 2, num_landmarks = 1 (num_agents = 6) — agents 0..3 the ADVERSARIES
 * (size 0.075, accel 3, max_speed 1), agent 0 their LEADER, agents 4, 5 the GOOD agents (size 0.045, accel 4, max_speed 1.3); five
 * landmarks in world order [landmark 0.2, food0, food1 0.03, forest0, forest1 0.3], none moves and only landmark 0 collides.  Every
 * agent moves, Discrete(5); the leader also says one of dim_c = 4 words, MultiDiscrete([[0, 4], [0, 3]]) — one launch per step.
 * Observation of agent m: own velocity 2, own position 2, the 5 landmarks relative to it 10, the five other agents relative to it
 * in world-agent order 10, then for an adversary the two good agents' velocities 4, its own in_forest flags 2 (+1 inside forest f,
 * else -1) and the leader's word of THIS step 4 (34 features); for a good agent its in_forest flags 2 and the other good agent's
 * velocity 2 (28).  Another agent's position, and a good one's velocity, is written as 0 unless it is visible to m: both inside the
 * same forest, or both inside no forest, or m is the leader.  Replaces MultiAgentEnv.step / _set_action (environment.py:117-256: the
 * MultiDiscrete split at :198-205, u = (a1 - a2, a3 - a4) * accel, the leader's c = its second head), World.step (core.py:207-322:
 * action force accel * u — accel a second time —, the soft-collision force between every pair of colliding entities of which one
 * can move, pairs a < b over the agents then landmark 0; damping 0.25; the max_speed clamp; dt 0.1; mass 1; state.c = action.c),
 * Scenario.reset_world / reward / observation (scenarios/simple_world_comm.py:100-112,141-199,225-288) + the vec-env's reset-on-done
 * (env_wrappers.py:146-152).  State is caller-owned device memory: agent_pos / agent_vel [N][6][2] and landmark_pos [N][5][2] in
 * float64, tstep [N] int32, episode [N] int64 (reset counter = Philox counter); the leader's word is not state, the step writes it
 * into the observations it returns.  obs: a HOST array of six device pointers, [N][34] x 4 then [N][28] x 2, fp32.  rewards [N][6]
 * fp32, ONE PER AGENT and never summed (world.collaborative is not set, environment.py:49-50,142): an adversary -0.1 x its distance
 * to the nearest good agent + 5 x (pairs of a good agent and ANY adversary within 0.12); a good agent -5 per adversary within 0.12,
 * -2 x the boundary penalty of |x| and of |y| (0 below 0.9, 10 (x - 0.9) below 1, else min(exp(2 x - 2), 10)), +2 per food item
 * within 0.075, +0.05 x its distance to the nearest food item; dones [N][6] bool bytes.  actions: a HOST array of device pointers —
 * action_mode 0: the reference's one-hots / probabilities, actions[0] [N][9] (the leader's move and word side by side) and
 * actions[1..5] [N][5]; 1: actions[0] = indices as fp32 [N][7] in the column order leader move, leader word, agents 1..5, clamped to
 * 0..4 (1/2/3/4 = +x/-x/+y/-y) and 0..3, actions[1..5] not read.  Physics in float64 with contraction off; the contact force and
 * the penalty go through the device's exp / log1p, so float obs and rewards match the fp32 cast of the reference's float64 values to
 * 1e-6 rather than to the bit; flags, hidden zeros, the word and dones are equal.  An environment whose episode ends (tstep >=
 * episode_length) is reset inside the same launch and returns the reset observation, the word in it zero; reset writes a zero word
 * too.  Reset draws: Philox stream (seed, episode), 64-bit uniform number 32 n + k of environment n — k = 2 a, 2 a + 1: position of
 * agent a in U(-1,1); k = 12 + 2 l, 13 + 2 l: position of landmark l in 0.8 U(-1,1); k = 22..31 unused; velocities start at zero.
 * Both validate on the host and name the fault: num_agents == 6 and num_landmarks == 1 (the only shape built), N >= 1, non-null
 * pointers (the arrays' entries included), action_mode 0 or 1, episode_length >= 1. */
int mappo_mpe_world_comm_reset(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                               float *const *obs /*host, [6]*/, int32_t N, int32_t num_agents, int32_t num_landmarks, uint64_t seed,
                               mappo_stream_t stream);
int mappo_mpe_world_comm_step(double *agent_pos, double *agent_vel, double *landmark_pos, int32_t *tstep, int64_t *episode,
                              const float *const *actions /*host, [6]*/, int32_t action_mode, float *const *obs /*host, [6]*/,
                              float *rewards, uint8_t *dones, int32_t N, int32_t num_agents, int32_t num_landmarks,
                              int32_t episode_length, uint64_t seed, mappo_stream_t stream);
/* One launch per rollout EPISODE on the environment above, env steps included, for the SEPARATED runner
 * (csrc/rollout_world_comm.h): what T x (mappo_rollout_step_md with the heads (5, 4) for the leader + one mappo_rollout_step per
 * other agent + mappo_mpe_world_comm_step with action_mode 1 + the agents' inserts) write into everything but the values, bit for
 * bit.  agents: six mappo_comm_agent (the leader, adversaries 1, 2, 3, then the two good agents).  Per step t < T: agent m's actor
 * on its observation rows of step t (step 0: obs_buf slot 0), row n sampled with (agent's seed, counter + t (+ the agent's
 * *counter_dev), Philox index n; the leader's head k: (k << 32) | n) -> actions / logp slot t, [T][N] and for the leader [T][N][2]
 * (move, word); the environments step in float64 on the sampled indices (reset-on-done after env_episode_length steps); each
 * agent's observation -> its obs_buf slot t + 1 (the word of step t in the adversaries' last four features, zeros where the
 * environment reset), its share row (centralized: the six observations side by side, 34 x 4 | 28 x 2 = 192; else its own
 * observation) -> share_buf slot t + 1, its OWN reward -> rew_buf slot t, 1 - done -> mask_buf slot t + 1.  The CRITICS DO NOT RUN
 * in this launch: values and next_values are neither read nor written; the caller runs each critic once afterwards on the agent's
 * share_buf viewed as [(T + 1) N][S] (slot T is the bootstrap value).  The critic descriptors are checked all the same, so that
 * what is refused here is what the sibling launches refuse.  The five state arrays are stored back at the end, so the environment
 * continues in either path.  Host checks, each named in the error: non-null descriptors; not recurrent; layer_N <= 1; actors in
 * 34 / out 9 (leader), in 34 / out 5 (x 3), in 28 / out 5 (x 2); critics out 1 and in 192 (centralized) or the agent's own in_dim;
 * the same layer_N and activation in all twelve networks; T, N, env_episode_length >= 1; non-null pointers.  A refused call
 * returns MAPPO_EINVAL and launches nothing. */
int mappo_rollout_episode_world_comm(const mappo_comm_agent *agents /*host, [6]*/, double *agent_pos, double *agent_vel,
                                     double *landmark_pos, int32_t *tstep, int64_t *episode, int32_t T, int32_t N,
                                     int32_t env_episode_length, uint64_t env_seed, int32_t deterministic, uint64_t counter,
                                     int32_t centralized, mappo_stream_t stream);

/* ---- benchmark utility: the synthetic SMAC-shaped vec-env of bench.py / scripts (mappo_amd/envs/synthetic.py), one launch per
 * step.  Not a reference interface (the reference's envs are CPU processes, onpolicy/envs/starcraft2/StarCraft2_Env.py): it only
 * produces data of the SMAC shapes with agents that die and episodes that end.  obs [N][M][D], share_obs [N][M][S] ~ N(0,1);
 * avail [N][M][A] in {0,1}; rewards [N]; dead (state) / dones [N][M] bool bytes; counter_dev [34] = {counter, 33 tickets}:
 * counter keys the Philox stream and is advanced by the launch itself (last workgroup to finish), tickets must start at 0. */
/* P consecutive steps in one launch (pools [P][N][M][D] ... [P][N][M]; step p uses counter + p, the launch advances the counter by P):
 * the env hands the pool out step by step as views, as SyntheticMPEEnv does with its per-episode block. */
int mappo_synth_smac_pool(float *obs, float *share_obs, float *avail, float *rewards, uint8_t *dead, uint8_t *dones, int32_t P,
                          int32_t N, int32_t M, int32_t D, int32_t S, int32_t A, float p_death, float p_term, uint64_t seed,
                          uint64_t *counter_dev /*[34]*/, mappo_stream_t stream);
int mappo_synth_smac_step(float *obs, float *share_obs, float *avail, float *rewards, uint8_t *dead, uint8_t *dones,
                          int32_t N, int32_t M, int32_t D, int32_t S, int32_t A, float p_death, float p_term,
                          uint64_t seed, uint64_t *counter_dev /*[34]*/, mappo_stream_t stream);

/* ---- measurement hook (bench.py): the NEXT launch of the entry point's dominant kernel carries the two hipEvent_t
 * handles (hipExtLaunchKernelGGL: start / stop of that dispatch on its own stream); the hook disarms after one use. */
#define MAPPO_PROF_GAE 0
#define MAPPO_PROF_PPO_LOSS 1
#define MAPPO_PROF_MLP_FWD 2
#define MAPPO_PROF_MLP_BWD 3
#define MAPPO_PROF_SLAB_REDUCE 4
#define MAPPO_PROF_ADAM 5
#define MAPPO_PROF_ACT 6
#define MAPPO_PROF_WIDE_L1 7 /* layer 1 of a wide-input update: its forward inside mappo_*_update / mappo_trunk_backward, its weight
                              * gradient inside mappo_wide_l1_backward (in_dim > 64) */
#define MAPPO_PROF_COUNT 8
int mappo_profile_arm(int32_t kernel_id, void *ev_start /*hipEvent_t*/, void *ev_stop /*hipEvent_t*/);

/* ---- self test: fp32 MFMA operand/accumulator lane maps (used by tests/, not by the product path) --- */
int mappo_selftest_mfma(const float *A /*[32][2]*/, const float *Bm /*[2][32]*/, float *D /*[32][32]*/,
                        mappo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MAPPO_HIP_H */
