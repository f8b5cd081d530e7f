"""TEST INFRASTRUCTURE ONLY (see oracle/__init__.py) — CPU restatement of the MAPPO hot path.

Every function cites the reference file:line it restates (paths relative to the reference
checkout, ``onpolicy/...``).  Arithmetic is float32 NumPy / torch-CPU exactly where the
reference uses them, so that results can be compared at 1e-5 relative (fp32) and bit-exact
(indices, masks).  The code is organised functionally (index math + gathers, explicit
per-step GRU) rather than as a transcription of the reference classes; the thin classes at
the bottom (BufferRef / PolicyRef / TrainerRef / run_iteration_ref) only wire the functions
together in the reference's order so that the whole iteration can be timed as the CPU baseline.

Parity: pinned by tests/golden/*.npz (outputs of the imported reference, generator script
tests/golden/generate_golden.py) — see tests/test_oracle_golden.py.
"""
from __future__ import annotations

import copy
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

F32 = np.float32


# --------------------------------------------------------------------------------------
# spaces (duck-typed by class name: onpolicy/utils/util.py:31-51)
# --------------------------------------------------------------------------------------
class Discrete:
    """Minimal stand-in for gym.spaces.Discrete (matched by class *name* in the reference)."""

    def __init__(self, n):
        self.n = int(n)


def obs_dim_of(space):
    """onpolicy/utils/util.py:31-38 + shared_buffer.py:39-43 (list spaces keep only [dim])."""
    name = space.__class__.__name__
    if name == "Box":
        shape = tuple(space.shape)
    elif name == "list":
        shape = space
    else:
        raise NotImplementedError(name)
    if isinstance(shape[-1], list):
        shape = shape[:1]
    return int(shape[0])


# --------------------------------------------------------------------------------------
# ValueNorm  (onpolicy/utils/valuenorm.py:8-78)
# --------------------------------------------------------------------------------------
class ValueNormRef:
    """Debiased EMA of mean / mean-square with beta=0.99999 (valuenorm.py:31-54)."""

    def __init__(self, beta=0.99999, epsilon=1e-5):
        self.beta, self.epsilon = beta, epsilon
        self.running_mean = torch.zeros(1)
        self.running_mean_sq = torch.zeros(1)
        self.debiasing_term = torch.tensor(0.0)

    # valuenorm.py:31-35
    def mean_var(self):
        d = self.debiasing_term.clamp(min=self.epsilon)
        mean = self.running_mean / d
        var = (self.running_mean_sq / d - mean ** 2).clamp(min=1e-2)
        return mean, var

    # valuenorm.py:37-54
    def update(self, x):
        x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x, dtype=torch.float32)
        bm = x.mean(dim=0)
        bsq = (x ** 2).mean(dim=0)
        w = self.beta
        self.running_mean.mul_(w).add_(bm * (1.0 - w))
        self.running_mean_sq.mul_(w).add_(bsq * (1.0 - w))
        self.debiasing_term.mul_(w).add_(1.0 * (1.0 - w))

    # valuenorm.py:56-65
    def normalize(self, x):
        x = torch.as_tensor(x, dtype=torch.float32)
        mean, var = self.mean_var()
        return (x - mean) / torch.sqrt(var)

    # valuenorm.py:67-78 (returns NumPy, like the reference)
    def denormalize(self, x):
        x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x, dtype=torch.float32)
        mean, var = self.mean_var()
        return (x * torch.sqrt(var) + mean).cpu().numpy()

    def state(self):
        return np.array([self.running_mean.item(), self.running_mean_sq.item(),
                         self.debiasing_term.item()], dtype=F32)

    def load_state(self, s):
        self.running_mean = torch.tensor([float(s[0])], dtype=torch.float32)
        self.running_mean_sq = torch.tensor([float(s[1])], dtype=torch.float32)
        self.debiasing_term = torch.tensor(float(s[2]), dtype=torch.float32)


# --------------------------------------------------------------------------------------
# compute_returns  (onpolicy/utils/shared_buffer.py:168-224)
# --------------------------------------------------------------------------------------
def compute_returns_ref(rewards, value_preds, masks, bad_masks, next_value, gamma, gae_lambda,
                        use_gae=True, use_proper_time_limits=False, denorm=None, returns=None):
    """All four flag branches of compute_returns.  Arrays are [T(+1), ...] float32; `value_preds`
    and `returns` are modified in place the way the reference does (slot T <- next_value in the
    GAE branches, returns[T] <- next_value in the discounted branches).  `denorm` is the
    ValueNorm denormaliser or None (shared_buffer.py:179,198,210: popart/valuenorm switch)."""
    T = rewards.shape[0]
    if returns is None:
        returns = np.zeros_like(value_preds)
    dn = (lambda x: denorm(x)) if denorm is not None else (lambda x: x)
    if use_gae:
        value_preds[-1] = next_value                      # :176 / :207
        gae = 0
        for t in range(T - 1, -1, -1):
            v_t, v_n = dn(value_preds[t]), dn(value_preds[t + 1])
            delta = rewards[t] + gamma * v_n * masks[t + 1] - v_t       # :181-183 / :210-212
            gae = delta + gamma * gae_lambda * masks[t + 1] * gae       # :184 / :213
            if use_proper_time_limits:
                gae = gae * bad_masks[t + 1]                            # :185
            returns[t] = gae + v_t                                      # :186 / :214
    else:
        returns[-1] = next_value                          # :194 / :222
        for t in range(T - 1, -1, -1):
            if use_proper_time_limits:                    # :196-204
                returns[t] = (returns[t + 1] * gamma * masks[t + 1] + rewards[t]) * bad_masks[t + 1] \
                    + (1 - bad_masks[t + 1]) * dn(value_preds[t])
            else:                                         # :223-224
                returns[t] = returns[t + 1] * gamma * masks[t + 1] + rewards[t]
    return returns


# --------------------------------------------------------------------------------------
# advantage normalisation  (onpolicy/algorithms/r_mappo/r_mappo.py:174-182)
# --------------------------------------------------------------------------------------
def normalized_advantages_ref(returns, value_preds, active_masks, denorm=None):
    v = denorm(value_preds[:-1]) if denorm is not None else value_preds[:-1]
    adv = returns[:-1] - v
    probe = adv.copy()
    probe[active_masks[:-1] == 0.0] = np.nan
    mean, std = np.nanmean(probe), np.nanstd(probe)
    return (adv - mean) / (std + 1e-5), mean, std


# --------------------------------------------------------------------------------------
# minibatch index math  (onpolicy/utils/shared_buffer.py:226-286, 288-383, 385-494)
# --------------------------------------------------------------------------------------
def feed_forward_rows(T, R, num_mini_batch, rand):
    """Flat source rows (t*R + r) of each minibatch; rand = torch.randperm(T*R) (:246-247)."""
    S = T * R
    assert S >= num_mini_batch
    mbs = S // num_mini_batch
    return [np.asarray(rand[k * mbs:(k + 1) * mbs], dtype=np.int64) for k in range(num_mini_batch)]


def recurrent_rows(T, R, num_mini_batch, L, rand):
    """Chunked-RNN minibatches (:385-494).  The reference re-orders to q=(r*T+t) (`_cast`,
    :10-11), cuts chunks [iL, iL+L) and stacks them time-major (L, mbs) (:438-474).  Returns
    per minibatch (rows[L*mbs] as flat t*R+r, h0_rows[mbs]); rand = torch.randperm(S // L)."""
    S = T * R
    chunks = S // L
    mbs = chunks // num_mini_batch
    out = []
    for k in range(num_mini_batch):
        c = np.asarray(rand[k * mbs:(k + 1) * mbs], dtype=np.int64)
        q = (c[None, :] * L + np.arange(L, dtype=np.int64)[:, None]).reshape(-1)   # time-major
        rows = (q % T) * R + q // T
        q0 = c * L
        h0 = (q0 % T) * R + q0 // T
        out.append((rows, h0))
    return out


def naive_recurrent_rows(T, R, num_mini_batch, perm):
    """Whole-episode sequences per (n,m) column (:288-383); perm = torch.randperm(R)."""
    assert R >= num_mini_batch
    n = R // num_mini_batch
    out = []
    for start in range(0, R, n):
        cols = np.asarray(perm[start:start + n], dtype=np.int64)
        if len(cols) < n:      # reference would index past perm and raise; never hit when R % nmb == 0
            break
        rows = (np.arange(T, dtype=np.int64)[:, None] * R + cols[None, :]).reshape(-1)
        out.append((rows, cols))
    return out


# --------------------------------------------------------------------------------------
# networks  (onpolicy/algorithms/utils/{mlp,rnn,act,distributions}.py, r_actor_critic.py)
# --------------------------------------------------------------------------------------
def _ortho(linear, gain):
    nn.init.orthogonal_(linear.weight.data, gain=gain)
    nn.init.constant_(linear.bias.data, 0)
    return linear


class _MLPStack(nn.Module):
    """mlp.py:6-28.  fc_h is the never-used template layer that still owns parameters."""

    def __init__(self, in_dim, hidden, layer_N, use_relu):
        super().__init__()
        gain = nn.init.calculate_gain("relu" if use_relu else "tanh")
        act = (lambda: nn.ReLU()) if use_relu else (lambda: nn.Tanh())
        self.fc1 = nn.Sequential(_ortho(nn.Linear(in_dim, hidden), gain), act(), nn.LayerNorm(hidden))
        self.fc_h = nn.Sequential(_ortho(nn.Linear(hidden, hidden), gain), act(), nn.LayerNorm(hidden))
        self.fc2 = nn.ModuleList([copy.deepcopy(self.fc_h) for _ in range(layer_N)])

    def forward(self, x):
        x = self.fc1(x)
        for blk in self.fc2:
            x = blk(x)
        return x


class _Trunk(nn.Module):
    """mlp.py:31-55."""

    def __init__(self, args, in_dim):
        super().__init__()
        self.use_fn = args.use_feature_normalization
        if self.use_fn:
            self.feature_norm = nn.LayerNorm(in_dim)
        self.mlp = _MLPStack(in_dim, args.hidden_size, args.layer_N, args.use_ReLU)

    def forward(self, x):
        if self.use_fn:
            x = self.feature_norm(x)
        return self.mlp(x)


def gru_cell_ref(gru: nn.GRU, x, h):
    """torch nn.GRU single layer cell, gate order (r, z, n)  (rnn.py:13)."""
    H = h.shape[-1]
    gi = x @ gru.weight_ih_l0.t() + gru.bias_ih_l0
    gh = h @ gru.weight_hh_l0.t() + gru.bias_hh_l0
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h


class _RNN(nn.Module):
    """rnn.py:7-80 with recurrent_N == 1.  The mask-segmented sequence run of the reference
    (rnn.py:30-77) equals multiplying h by mask_t before every step."""

    def __init__(self, hidden):
        super().__init__()
        self.rnn = nn.GRU(hidden, hidden, num_layers=1)
        for name, p in self.rnn.named_parameters():
            if "bias" in name:
                nn.init.constant_(p, 0)
            else:
                nn.init.orthogonal_(p)
        self.norm = nn.LayerNorm(hidden)

    def forward(self, x, hxs, masks):
        # hxs: [Nc, 1, H]; x: [Nc, H] (single step) or [L*Nc, H] (time-major sequence)
        Nc = hxs.shape[0]
        h = hxs[:, 0]
        if x.shape[0] == Nc:
            h = gru_cell_ref(self.rnn, x, h * masks)
            out = h
        else:
            L = x.shape[0] // Nc
            xs, ms = x.view(L, Nc, -1), masks.view(L, Nc, 1)
            outs = []
            for t in range(L):
                h = gru_cell_ref(self.rnn, xs[t], h * ms[t])
                outs.append(h)
            out = torch.cat(outs, 0)
        return self.norm(out), h.unsqueeze(1)


class _CategoricalHead(nn.Module):
    def __init__(self, hidden, n, gain):
        super().__init__()
        self.linear = _ortho(nn.Linear(hidden, n), gain)


class _ActLayer(nn.Module):
    """act.py Discrete branch (:78-81,154-160) + distributions.py:14-28,55-68."""

    def __init__(self, hidden, n, gain):
        super().__init__()
        self.action_out = _CategoricalHead(hidden, n, gain)

    def logits(self, x, avail):
        z = self.action_out.linear(x)
        if avail is not None:
            z = z.masked_fill(avail == 0, -1e10)      # in-place assignment in the reference
        return z

    @staticmethod
    def logp_entropy(z, actions):
        logp_all = z - torch.logsumexp(z, dim=-1, keepdim=True)
        p = torch.exp(logp_all)
        ent = -(p * torch.clamp(logp_all, min=torch.finfo(z.dtype).min)).sum(-1)
        logp = logp_all.gather(-1, actions.long().view(-1, 1))
        return logp, ent, p


class ActorRef(nn.Module):
    """r_actor_critic.py:11-107 (MLP trunk -> [GRU] -> categorical head)."""

    def __init__(self, args, obs_dim, n_actions):
        super().__init__()
        self.recurrent = bool(args.use_recurrent_policy or args.use_naive_recurrent_policy)
        self.use_policy_active_masks = args.use_policy_active_masks
        self.base = _Trunk(args, obs_dim)
        if self.recurrent:
            self.rnn = _RNN(args.hidden_size)
        self.act = _ActLayer(args.hidden_size, n_actions, args.gain)

    def features(self, obs, rnn_states, masks):
        x = self.base(obs)
        if self.recurrent:
            x, rnn_states = self.rnn(x, rnn_states, masks)
        return x, rnn_states

    def forward(self, obs, rnn_states, masks, avail=None, deterministic=False, generator=None):
        x, rnn_states = self.features(obs, rnn_states, masks)
        z = self.act.logits(x, avail)
        probs = torch.softmax(z, -1)
        if deterministic:
            actions = probs.argmax(-1, keepdim=True)          # distributions.py:27-28
        else:
            actions = torch.multinomial(probs, 1, generator=generator)
        logp, _, _ = self.act.logp_entropy(z, actions)
        return actions, logp, rnn_states

    def evaluate_actions(self, obs, rnn_states, action, masks, avail=None, active_masks=None):
        x, _ = self.features(obs, rnn_states, masks)
        z = self.act.logits(x, avail)
        logp, ent, _ = self.act.logp_entropy(z, action)
        if active_masks is not None and self.use_policy_active_masks:
            ent = (ent * active_masks.squeeze(-1)).sum() / active_masks.sum()     # act.py:157-158
        else:
            ent = ent.mean()
        return logp, ent, z


class CriticRef(nn.Module):
    """r_actor_critic.py:110-165."""

    def __init__(self, args, cent_obs_dim):
        super().__init__()
        self.recurrent = bool(args.use_recurrent_policy or args.use_naive_recurrent_policy)
        self.base = _Trunk(args, cent_obs_dim)
        if self.recurrent:
            self.rnn = _RNN(args.hidden_size)
        self.v_out = _ortho(nn.Linear(args.hidden_size, 1), 1.0)

    def forward(self, cent_obs, rnn_states, masks):
        x = self.base(cent_obs)
        if self.recurrent:
            x, rnn_states = self.rnn(x, rnn_states, masks)
        return self.v_out(x), rnn_states


# --------------------------------------------------------------------------------------
# fused loss: analytic forward + gradient  (r_mappo.py:52-89,124-141; util.py:23-29)
# --------------------------------------------------------------------------------------
def ppo_loss_fwd_bwd_ref(logits, avail, actions, old_logp, adv, active, values, v_old, ret,
                         vn_mean, vn_var, clip, entropy_coef, value_loss_coef, huber_delta,
                         use_huber=True, use_clipped_value=True, use_policy_active=True,
                         use_value_active=True, use_valuenorm=True):
    """float64 analytic evaluation of the actor objective (L_pi - c_H * H) and critic objective
    (c_V * L_V) and their gradients w.r.t. logits and values — SURVEY Appendix A formulas.
    `vn_mean/vn_var` are the ValueNorm statistics *after* update(ret) (r_mappo.py:65).
    Returns dict(policy_loss, dist_entropy, value_loss, ratio_mean, dlogits[B,A], dvalues[B])."""
    f = np.float64
    z = np.array(logits, dtype=f)
    B, A = z.shape
    if avail is not None:
        dead = np.asarray(avail) == 0
        z = np.where(dead, -1e10, z)
    else:
        dead = np.zeros_like(z, dtype=bool)
    a = np.asarray(actions).reshape(B).astype(np.int64)
    old = np.asarray(old_logp, dtype=f).reshape(B)
    advv = np.asarray(adv, dtype=f).reshape(B)
    act = np.asarray(active, dtype=f).reshape(B)
    zmax = z.max(-1, keepdims=True)
    lse = zmax + np.log(np.exp(z - zmax).sum(-1, keepdims=True))
    logp_all = z - lse
    p = np.exp(logp_all)
    logp = logp_all[np.arange(B), a]
    ent = -(p * np.maximum(logp_all, np.finfo(np.float32).min)).sum(-1)
    ratio = np.exp(logp - old)
    s1 = ratio * advv
    s2 = np.clip(ratio, 1 - clip, 1 + clip) * advv
    w_pi = act / act.sum() if use_policy_active else np.full(B, 1.0 / B)
    policy_loss = -(w_pi * np.minimum(s1, s2)).sum()
    dist_entropy = (w_pi * ent).sum()
    # d(actor objective)/d logp_a and / d z
    dlogp = np.where(s1 <= s2, -w_pi * advv * ratio, 0.0)
    onehot = np.zeros((B, A)); onehot[np.arange(B), a] = 1.0
    dz = dlogp[:, None] * (onehot - p)
    dz += -entropy_coef * w_pi[:, None] * (-p * (logp_all + ent[:, None]))
    dz = np.where(dead, 0.0, dz)
    # value loss
    v = np.asarray(values, dtype=f).reshape(B)
    vo = np.asarray(v_old, dtype=f).reshape(B)
    r = np.asarray(ret, dtype=f).reshape(B)
    tgt = (r - vn_mean) / np.sqrt(vn_var) if use_valuenorm else r
    vclip = vo + np.clip(v - vo, -clip, clip)
    e_o, e_c = tgt - v, tgt - vclip

    def loss_and_slope(e):
        if use_huber:
            small = np.abs(e) <= huber_delta
            return (np.where(small, e * e / 2, huber_delta * (np.abs(e) - huber_delta / 2)),
                    np.where(small, e, huber_delta * np.sign(e)))
        return e * e / 2, e

    l_o, g_o = loss_and_slope(e_o)
    l_c, g_c = loss_and_slope(e_c)
    inside = (np.abs(v - vo) <= clip).astype(f)
    if use_clipped_value:
        l = np.maximum(l_o, l_c)
        d_o, d_c = -g_o, -g_c * inside
        dv = np.where(l_o > l_c, d_o, np.where(l_c > l_o, d_c, 0.5 * (d_o + d_c)))
    else:
        l, dv = l_o, -g_o
    w_v = act / act.sum() if use_value_active else np.full(B, 1.0 / B)
    value_loss = (w_v * l).sum()
    dv = dv * w_v * value_loss_coef
    return dict(policy_loss=policy_loss, dist_entropy=dist_entropy, value_loss=value_loss,
                ratio_mean=ratio.mean(), dlogits=dz, dvalues=dv)


def huber_ref(e, d):
    """util.py:23-26."""
    a = (abs(e) <= d).float()
    b = (abs(e) > d).float()
    return a * e ** 2 / 2 + b * d * (abs(e) - d / 2)


# --------------------------------------------------------------------------------------
# grad clip + Adam on flat arrays  (r_mappo.py:143-148; torch Adam — SURVEY Appendix A)
# --------------------------------------------------------------------------------------
def clip_adam_ref(param, grad, exp_avg, exp_avg_sq, step, lr, max_norm, use_clip=True,
                  beta1=0.9, beta2=0.999, eps=1e-5, weight_decay=0.0):
    """float64 reference of clip_grad_norm_ + one torch.optim.Adam step on flat vectors.
    Returns (param, exp_avg, exp_avg_sq, pre-clip grad norm)."""
    g = np.asarray(grad, dtype=np.float64)
    norm = math.sqrt(float((g * g).sum()))
    if use_clip:
        coef = min(1.0, max_norm / (norm + 1e-6))
        g = g * coef
    p = np.asarray(param, dtype=np.float64)
    if weight_decay != 0.0:
        g = g + weight_decay * p
    m = beta1 * np.asarray(exp_avg, dtype=np.float64) + (1 - beta1) * g
    v = beta2 * np.asarray(exp_avg_sq, dtype=np.float64) + (1 - beta2) * g * g
    t = step + 1
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    p = p - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v, norm


# --------------------------------------------------------------------------------------
# wiring: buffer / policy / trainer / iteration  (CPU baseline + end-to-end oracle)
# --------------------------------------------------------------------------------------
def default_args(**kw):
    """Flag names/defaults of onpolicy/config.py:156-287 that the hot path reads."""
    d = dict(episode_length=200, n_rollout_threads=32, hidden_size=64, layer_N=1, recurrent_N=1,
             use_ReLU=True, use_popart=False, use_valuenorm=True, use_feature_normalization=True,
             use_orthogonal=True, gain=0.01, use_naive_recurrent_policy=False,
             use_recurrent_policy=False, data_chunk_length=10, lr=5e-4, critic_lr=5e-4,
             opti_eps=1e-5, weight_decay=0.0, ppo_epoch=15, use_clipped_value_loss=True,
             clip_param=0.2, num_mini_batch=1, entropy_coef=0.01, value_loss_coef=1.0,
             use_max_grad_norm=True, max_grad_norm=10.0, use_gae=True, gamma=0.99,
             gae_lambda=0.95, use_proper_time_limits=False, use_huber_loss=True,
             use_value_active_masks=True, use_policy_active_masks=True, huber_delta=10.0,
             stacked_frames=1, use_centralized_V=True)
    d.update(kw)
    return SimpleNamespace(**d)


class BufferRef:
    """onpolicy/utils/shared_buffer.py:24-166 (array set, insert, after_update)."""

    def __init__(self, args, num_agents, obs_dim, share_dim, n_actions):
        T, N, M, H = args.episode_length, args.n_rollout_threads, num_agents, args.hidden_size
        self.T, self.N, self.M = T, N, M
        self.args = args
        z = lambda *s: np.zeros(s, dtype=F32)
        o = lambda *s: np.ones(s, dtype=F32)
        self.share_obs, self.obs = z(T + 1, N, M, share_dim), z(T + 1, N, M, obs_dim)
        self.rnn_states = z(T + 1, N, M, args.recurrent_N, H)
        self.rnn_states_critic = z(T + 1, N, M, args.recurrent_N, H)
        self.value_preds, self.returns = z(T + 1, N, M, 1), z(T + 1, N, M, 1)
        self.available_actions = o(T + 1, N, M, n_actions)
        self.actions, self.action_log_probs, self.rewards = z(T, N, M, 1), z(T, N, M, 1), z(T, N, M, 1)
        self.masks, self.bad_masks, self.active_masks = o(T + 1, N, M, 1), o(T + 1, N, M, 1), o(T + 1, N, M, 1)
        self.step = 0

    def insert(self, share_obs, obs, rnn_a, rnn_c, actions, logp, values, rewards, masks,
               bad_masks=None, active_masks=None, available_actions=None):
        s = self.step                                      # shared_buffer.py:96-112
        self.share_obs[s + 1], self.obs[s + 1] = share_obs, obs
        self.rnn_states[s + 1], self.rnn_states_critic[s + 1] = rnn_a, rnn_c
        self.actions[s], self.action_log_probs[s] = actions, logp
        self.value_preds[s], self.rewards[s], self.masks[s + 1] = values, rewards, masks
        if bad_masks is not None:
            self.bad_masks[s + 1] = bad_masks
        if active_masks is not None:
            self.active_masks[s + 1] = active_masks
        if available_actions is not None:
            self.available_actions[s + 1] = available_actions
        self.step = (s + 1) % self.T

    def after_update(self):                                # shared_buffer.py:149-159
        for name in ("share_obs", "obs", "rnn_states", "rnn_states_critic", "masks", "bad_masks",
                     "active_masks", "available_actions"):
            arr = getattr(self, name)
            arr[0] = arr[-1]

    def compute_returns(self, next_value, vnorm):
        a = self.args
        dn = vnorm.denormalize if (vnorm is not None and a.use_valuenorm) else None
        compute_returns_ref(self.rewards, self.value_preds, self.masks, self.bad_masks, next_value,
                            a.gamma, a.gae_lambda, a.use_gae, a.use_proper_time_limits, dn, self.returns)

    def flat(self, name, with_last=False):
        arr = getattr(self, name)
        arr = arr if with_last or arr.shape[0] == self.T else arr[:-1]
        return arr.reshape(-1, *arr.shape[3:])

    def sample(self, rows, advantages, h0_rows=None):
        """The 12-tuple of the generators (shared_buffer.py:281-283) for given flat rows."""
        g = lambda n: self.flat(n)[rows]
        hr = rows if h0_rows is None else h0_rows
        return (g("share_obs"), g("obs"), self.flat("rnn_states")[hr], self.flat("rnn_states_critic")[hr],
                g("actions"), g("value_preds"), g("returns"), g("masks"), g("active_masks"),
                g("action_log_probs"), advantages.reshape(-1, 1)[rows], g("available_actions"))


class PolicyRef:
    """rMAPPOPolicy.py:17-37."""

    def __init__(self, args, obs_dim, share_dim, n_actions):
        self.actor = ActorRef(args, obs_dim, n_actions)
        self.critic = CriticRef(args, share_dim)
        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr=args.lr, eps=args.opti_eps,
                                                weight_decay=args.weight_decay)
        self.critic_optimizer = torch.optim.Adam(self.critic.parameters(), lr=args.critic_lr,
                                                 eps=args.opti_eps, weight_decay=args.weight_decay)


def ppo_losses_ref(args, logp, ent, values, old_logp, adv, active, v_old, tgt):
    """The loss expressions of r_mappo.py:52-141 on autograd tensors (any float dtype): evaluate_actions' log-probs and
    entropy, the critic's values and the value target (already normalised under use_valuenorm).  Honours every loss flag
    of `args`.  Returns (policy_loss, value_loss, imp_weights); the actor objective is policy_loss - entropy_coef * ent,
    the critic's value_loss * value_loss_coef."""
    imp = torch.exp(logp - old_logp)
    s1 = imp * adv
    s2 = torch.clamp(imp, 1.0 - args.clip_param, 1.0 + args.clip_param) * adv
    surr = torch.sum(torch.min(s1, s2), dim=-1, keepdim=True)
    if args.use_policy_active_masks:
        policy_loss = (-surr * active).sum() / active.sum()
    else:
        policy_loss = -surr.mean()
    v_clip = v_old + (values - v_old).clamp(-args.clip_param, args.clip_param)
    e_c, e_o = tgt - v_clip, tgt - values
    if args.use_huber_loss:
        l_c, l_o = huber_ref(e_c, args.huber_delta), huber_ref(e_o, args.huber_delta)
    else:
        l_c, l_o = e_c ** 2 / 2, e_o ** 2 / 2
    l = torch.max(l_o, l_c) if args.use_clipped_value_loss else l_o
    value_loss = (l * active).sum() / active.sum() if args.use_value_active_masks else l.mean()
    return policy_loss, value_loss, imp


def ppo_update_ref(args, policy, vnorm, sample, update_actor=True, dtype=torch.float32):
    """r_mappo.py:91-164 on torch-CPU autograd.  Returns the 6-tuple as floats + imp_weights.  `dtype` is that of the
    sample tensors; the caller converts the policy's networks to it (float64: a reference for the fp32 kernels).  The
    ValueNorm statistics stay float32, as in the reference."""
    t = lambda x: torch.as_tensor(x, dtype=dtype)
    (share_obs, obs, rnn_a, rnn_c, actions, v_old, ret, masks, active, old_logp, adv, avail) = \
        [None if x is None else t(x) for x in sample]
    logp, ent, _ = policy.actor.evaluate_actions(obs, rnn_a, actions, masks, avail, active)
    values, _ = policy.critic(share_obs, rnn_c, masks)
    if args.use_valuenorm:
        vnorm.update(ret)
        tgt = vnorm.normalize(ret).to(dtype)
    else:
        tgt = ret
    policy_loss, value_loss, imp = ppo_losses_ref(args, logp, ent, values, old_logp, adv, active, v_old, tgt)
    policy.actor_optimizer.zero_grad()
    if update_actor:
        (policy_loss - ent * args.entropy_coef).backward()
    if args.use_max_grad_norm:
        a_norm = float(nn.utils.clip_grad_norm_(policy.actor.parameters(), args.max_grad_norm))
    else:
        a_norm = math.sqrt(sum(float(p.grad.norm()) ** 2 for p in policy.actor.parameters() if p.grad is not None))
    policy.actor_optimizer.step()
    # critic (r_mappo.py:52-89)
    policy.critic_optimizer.zero_grad()
    (value_loss * args.value_loss_coef).backward()
    if args.use_max_grad_norm:
        c_norm = float(nn.utils.clip_grad_norm_(policy.critic.parameters(), args.max_grad_norm))
    else:
        c_norm = math.sqrt(sum(float(p.grad.norm()) ** 2 for p in policy.critic.parameters() if p.grad is not None))
    policy.critic_optimizer.step()
    return float(value_loss), c_norm, float(policy_loss), float(ent), a_norm, imp.detach()


def train_ref(args, policy, vnorm, buf: BufferRef, perms=None):
    """r_mappo.py:166-219.  `perms` optionally supplies the permutation per epoch (else
    torch.randperm, like the reference)."""
    dn = vnorm.denormalize if args.use_valuenorm else None
    adv, _, _ = normalized_advantages_ref(buf.returns, buf.value_preds, buf.active_masks, dn)
    T, R = buf.T, buf.N * buf.M
    info = dict(value_loss=0.0, policy_loss=0.0, dist_entropy=0.0, actor_grad_norm=0.0,
                critic_grad_norm=0.0, ratio=0.0)
    for e in range(args.ppo_epoch):
        if args.use_recurrent_policy:
            chunks = (T * R) // args.data_chunk_length
            rand = perms[e] if perms is not None else torch.randperm(chunks).numpy()
            batches = [buf.sample(rows, adv_cast(adv, rows), h0) for rows, h0 in
                       recurrent_rows(T, R, args.num_mini_batch, args.data_chunk_length, rand)]
        elif args.use_naive_recurrent_policy:
            perm = perms[e] if perms is not None else torch.randperm(R).numpy()
            batches = [buf.sample(rows, adv_cast(adv, rows), cols) for rows, cols in
                       naive_recurrent_rows(T, R, args.num_mini_batch, perm)]
        else:
            rand = perms[e] if perms is not None else torch.randperm(T * R).numpy()
            batches = [buf.sample(rows, adv_cast(adv, rows)) for rows in
                       feed_forward_rows(T, R, args.num_mini_batch, rand)]
        for sample in batches:
            vl, cn, pl, en, an, imp = ppo_update_ref(args, policy, vnorm, sample)
            info["value_loss"] += vl; info["policy_loss"] += pl; info["dist_entropy"] += en
            info["actor_grad_norm"] += an; info["critic_grad_norm"] += cn
            info["ratio"] += float(imp.mean())
    n = args.ppo_epoch * args.num_mini_batch
    return {k: v / n for k, v in info.items()}


def adv_cast(adv, rows):
    """identity helper: BufferRef.sample gathers advantages by flat row itself."""
    return adv


class SyntheticMPEEnvRef:
    """CPU twin of mappo_amd.envs.synthetic.SyntheticMPEEnv (SURVEY §8d synthetic inputs):
    obs ~ N(0,1), reward N(0,1) shared by the agents of a thread, all-done every T-th step."""

    def __init__(self, n_threads, n_agents, obs_dim, episode_length, seed=1):
        self.N, self.M, self.D, self.T = n_threads, n_agents, obs_dim, episode_length
        self.rng = np.random.default_rng(seed)
        self.t = 0

    def reset(self):
        self.t = 0
        return self.rng.standard_normal((self.N, self.M, self.D), dtype=F32)

    def step(self, actions_env):
        self.t += 1
        obs = self.rng.standard_normal((self.N, self.M, self.D), dtype=F32)
        rew = np.repeat(self.rng.standard_normal((self.N, 1, 1), dtype=F32), self.M, axis=1)
        done = np.full((self.N, self.M), self.t % self.T == 0)
        return obs, rew, done, None


class RunnerRef:
    """collect / insert / compute / train of onpolicy/runner/shared/{base,mpe}_runner.py
    (base_runner.py:110-125, mpe_runner.py:81-139) for the MLP/GRU MPE-style contract."""

    def __init__(self, args, env, num_agents, obs_dim, share_dim, n_actions, seed=1):
        torch.manual_seed(seed)
        self.args, self.env, self.M = args, env, num_agents
        self.policy = PolicyRef(args, obs_dim, share_dim, n_actions)
        self.vnorm = ValueNormRef() if args.use_valuenorm else None
        self.buffer = BufferRef(args, num_agents, obs_dim, share_dim, n_actions)
        self.n_actions = n_actions

    def _share(self, obs):
        N = obs.shape[0]
        return np.repeat(obs.reshape(N, 1, -1), self.M, axis=1)       # mpe_runner.py:133-135

    def warmup(self):
        obs = self.env.reset()
        self.buffer.share_obs[0], self.buffer.obs[0] = self._share(obs), obs

    @torch.no_grad()
    def collect(self, step):
        b, N = self.buffer, self.buffer.N
        cat = lambda x: torch.from_numpy(np.concatenate(x))
        actions, logp, rnn_a = self.policy.actor(cat(b.obs[step]), cat(b.rnn_states[step]), cat(b.masks[step]))
        values, rnn_c = self.policy.critic(cat(b.share_obs[step]), cat(b.rnn_states_critic[step]), cat(b.masks[step]))
        sp = lambda x: np.array(np.split(x.numpy(), N))
        return sp(values), sp(actions), sp(logp), sp(rnn_a), sp(rnn_c)

    def insert(self, obs, rewards, dones, values, actions, logp, rnn_a, rnn_c):
        rnn_a[dones] = 0.0
        rnn_c[dones] = 0.0
        masks = np.ones((self.buffer.N, self.M, 1), dtype=F32)
        masks[dones] = 0.0
        self.buffer.insert(self._share(obs), obs, rnn_a, rnn_c, actions.astype(F32), logp, values, rewards, masks)

    @torch.no_grad()
    def compute(self):
        b = self.buffer
        cat = lambda x: torch.from_numpy(np.concatenate(x))
        nv, _ = self.policy.critic(cat(b.share_obs[-1]), cat(b.rnn_states_critic[-1]), cat(b.masks[-1]))
        b.compute_returns(np.array(np.split(nv.numpy(), b.N)), self.vnorm)

    def run_iteration(self):
        timing = {}
        import time
        t0 = time.perf_counter()
        for step in range(self.args.episode_length):
            values, actions, logp, rnn_a, rnn_c = self.collect(step)
            onehot = np.eye(self.n_actions, dtype=F32)[actions[..., 0]]
            obs, rew, done, _ = self.env.step(onehot)
            self.insert(obs, rew, done, values, actions, logp, rnn_a, rnn_c)
        t1 = time.perf_counter()
        self.compute()
        t2 = time.perf_counter()
        info = train_ref(self.args, self.policy, self.vnorm, self.buffer)
        self.buffer.after_update()
        t3 = time.perf_counter()
        timing.update(collect=t1 - t0, gae=t2 - t1, train=t3 - t2, total=t3 - t0)
        return info, timing
