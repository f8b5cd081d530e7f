"""Host reference of the rollout sampling contract (include/mappo_hip.h, at mappo_actor_act), independent of the kernels:

  Philox4x32-10 written from its definition (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), vectorised
  in NumPy over the row index;  u = (word 0 >> 8) * 2^-24 with counter words {index lo, index hi, counter lo, counter hi} and
  key words {seed lo, seed hi};

  the policy in float64 through the oracle modules (oracle/mappo_oracle.py, cast to .double()): logits with unavailable
  actions at -1e10, log-softmax, probabilities and their running sum;

  the expected action (sampling: the first a with u < C_a; deterministic: the first maximum), the rows that sit within a
  margin of a decision boundary, and the checker that holds a kernel's (action, log-prob) against all of that.

A plain helper module: no fixtures, no pytest settings."""
import copy

import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)       # multipliers of Philox4x32
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85                             # Weyl increments of the key schedule


def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds.  ctr: 4 arrays (or scalars) of 32-bit words, key: 2 words; returns the 4 output words as
    uint64 arrays holding 32-bit values.  One round: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2,
    c' = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped by the Weyl constants between rounds."""
    c = [np.asarray(w, dtype=np.uint64) & M32 for w in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]                        # 32 x 32 -> 64 bit, exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return c


def philox_u32(seed, counter, index):
    """Word 0 of Philox4x32-10 with the kernels' word mapping: c0, c1 = index lo, hi; c2, c3 = counter lo, hi; k0, k1 = seed
    lo, hi.  seed / counter: Python ints (taken mod 2^64), index: integer array."""
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    idx = np.asarray(index, dtype=np.uint64)
    return philox4x32_10((idx & M32, idx >> np.uint64(32), counter & 0xFFFFFFFF, counter >> 32), (seed & 0xFFFFFFFF, seed >> 32))[0]


def uniform24(seed, counter, index):
    """The 24-bit uniform the kernels draw for row `index`: exact in float32 and in float64."""
    return (philox_u32(seed, counter, index) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


# ---- the policy in float64 / float32 on the CPU --------------------------------------------------------------------------------
def _t(x, dtype):
    return None if x is None else torch.as_tensor(np.asarray(x)).to(dtype)


def actor_eval(actor, obs, avail=None, h0=None, masks=None, dtype=torch.float64):
    """(masked logits [B][A], next hidden state [B][H] or None) of an oracle ActorRef evaluated in `dtype`."""
    net = copy.deepcopy(actor).to(dtype)
    with torch.no_grad():
        rec = net.recurrent
        x, h = net.features(_t(obs, dtype), _t(h0, dtype).unsqueeze(1) if rec else None, _t(masks, dtype).view(-1, 1) if rec else None)
        z = net.act.logits(x, _t(avail, dtype))
    return z.double().numpy(), (h[:, 0].double().numpy() if rec else None)


def critic_eval(critic, sobs, h0=None, masks=None, dtype=torch.float64):
    """(values [B], next hidden state or None) of an oracle CriticRef evaluated in `dtype`."""
    net = copy.deepcopy(critic).to(dtype)
    with torch.no_grad():
        rec = net.recurrent
        v, h = net(_t(sobs, dtype), _t(h0, dtype).unsqueeze(1) if rec else None, _t(masks, dtype).view(-1, 1) if rec else None)
    return v.double().numpy().reshape(-1), (h[:, 0].double().numpy() if rec else None)


def head_eval(actor, feats, avail=None, h0=None, masks=None, dtype=torch.float64):
    """actor_eval from trunk features instead of observations (the entry points that take featT)."""
    net = copy.deepcopy(actor).to(dtype)
    with torch.no_grad():
        x, h = net.rnn(_t(feats, dtype), _t(h0, dtype).unsqueeze(1), _t(masks, dtype).view(-1, 1))
        z = net.act.logits(x, _t(avail, dtype))
    return z.double().numpy(), h[:, 0].double().numpy()


def critic_head_eval(critic, feats, h0, masks, dtype=torch.float64):
    net = copy.deepcopy(critic).to(dtype)
    with torch.no_grad():
        x, h = net.rnn(_t(feats, dtype), _t(h0, dtype).unsqueeze(1), _t(masks, dtype).view(-1, 1))
        v = net.v_out(x)
    return v.double().numpy().reshape(-1), h[:, 0].double().numpy()


def err_and_tol(ref64, ref32):
    """err32 = max |float32 CPU evaluation - float64| of one output of one module, tol = 4 err32 + 2e-6."""
    err32 = float(np.abs(np.asarray(ref32, np.float64) - np.asarray(ref64, np.float64)).max())
    return err32, 4.0 * err32 + 2e-6


def log_softmax64(z):
    z = np.asarray(z, np.float64)
    s = z - z.max(axis=1, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=1, keepdims=True))


# ---- expected actions -------------------------------------------------------------------------------------------------------------
class Expected:
    """Per row: the expected action, whether the row is near a decision boundary, and the set of actions a kernel whose logits are
    within the tolerance may return (allowed[b][a]; exactly the expected one on a clear row)."""

    def __init__(self, action, near, allowed, logp_all, margin):
        self.action, self.near, self.allowed, self.logp_all, self.margin = action, near, allowed, logp_all, margin


def _avail_bool(avail, shape):
    return np.ones(shape, bool) if avail is None else (np.asarray(avail) != 0)


def expected_sample(z, avail, u, tol):
    """Inverse-CDF sampling: k = first a with u < C_a (C the float64 running sum of softmax(z); the last supported action if
    rounding leaves u >= C_last).  Near a boundary: min |u - C_a| < delta = 2 tol + 32 * 2^-23 over the interior boundaries of
    the available actions (every available action's C_a but the last one's, which is 1).  A near row may return any available
    action whose interval [C_(a-1), C_a] reaches into (u - delta, u + delta): the two neighbours of the boundary."""
    z = np.asarray(z, np.float64)
    B, A = z.shape
    av = _avail_bool(avail, z.shape)
    lp = log_softmax64(z)
    C = np.cumsum(np.exp(lp), axis=1)
    delta = 2.0 * tol + 32 * 2.0 ** -23
    u = np.asarray(u, np.float64).reshape(B, 1)
    last = A - 1 - np.argmax(av[:, ::-1], axis=1)                       # last available action
    hit = u < C
    k = np.where(hit.any(axis=1), np.argmax(hit, axis=1), last)
    k = np.minimum(k, last)
    interior = av.copy()
    interior[np.arange(B), last] = False
    dist = np.where(interior, np.abs(u - C), np.inf).min(axis=1)
    near = dist < delta
    lo = np.concatenate([np.zeros((B, 1)), C[:, :-1]], axis=1)
    allowed = av & (lo < u + delta) & (C > u - delta)
    allowed[np.arange(B), k] = True
    allowed[~near] = False
    allowed[~near, k[~near]] = True
    return Expected(k, near, allowed, lp, delta)


def expected_argmax(z, avail, tol):
    """Deterministic: the first maximum of the float64 logits; near a boundary when the top-two gap is < delta_z = 2 tol, and then
    either of the top actions (every one within delta_z of the maximum) is allowed."""
    z = np.asarray(z, np.float64)
    B, A = z.shape
    av = _avail_bool(avail, z.shape)
    lp = log_softmax64(z)
    delta_z = 2.0 * tol
    k = np.argmax(z, axis=1)
    if A > 1:
        top2 = np.sort(z, axis=1)[:, -2:]
        near = (top2[:, 1] - top2[:, 0]) < delta_z
    else:
        near = np.zeros(B, bool)
    allowed = av & (z > z.max(axis=1, keepdims=True) - delta_z)
    allowed[~near] = False
    allowed[~near, k[~near]] = True
    return Expected(k, near, allowed, lp, delta_z)


def check_actions(exp, avail, actions, logp, tol, what=""):
    """Hold a kernel's actions / log-probs [B] against `exp`.  Returns a list of failure strings (empty: all good):
    an unavailable action on any row; a clear row that is not exactly the expected action; a near-boundary row outside the
    boundary's neighbours; a log-prob further than tol from the float64 log-prob of the action actually returned."""
    actions = np.asarray(actions)
    logp = np.asarray(logp, np.float64)
    B, A = exp.logp_all.shape
    fails = []
    a_int = actions.astype(np.int64)
    if not (np.isfinite(actions).all() and (a_int == actions).all() and (a_int >= 0).all() and (a_int < A).all()):
        return [f"{what}: actions are not integers in [0, {A}): {actions[:8]}"]
    rows = np.arange(B)
    av = _avail_bool(avail, (B, A))
    dead = np.flatnonzero(~av[rows, a_int])
    if dead.size:
        fails.append(f"{what}: {dead.size} rows returned an unavailable action (first rows {dead[:5]}, actions {a_int[dead[:5]]})")
    clear = ~exp.near
    wrong = np.flatnonzero(clear & (a_int != exp.action))
    if wrong.size:
        fails.append(f"{what}: {wrong.size} of {int(clear.sum())} clear rows differ from the expected action (first rows {wrong[:5]}: "
                     f"got {a_int[wrong[:5]]}, expected {exp.action[wrong[:5]]})")
    out = np.flatnonzero(exp.near & ~exp.allowed[rows, a_int])
    if out.size:
        fails.append(f"{what}: {out.size} near-boundary rows returned an action that is no neighbour of the boundary (rows {out[:5]})")
    ok = av[rows, a_int]
    d = np.abs(logp - exp.logp_all[rows, a_int])
    d = np.where(ok, d, 0.0)
    if not np.isfinite(logp).all() or d.max() > tol:
        w = int(np.argmax(np.where(np.isfinite(d), d, np.inf)))
        fails.append(f"{what}: log-prob of the returned action off by {d.max():.3e} > tol {tol:.3e} (row {w}: {logp[w]!r} vs "
                     f"{exp.logp_all[w, a_int[w]]!r})")
    return fails


def max_logp_err(exp, actions, logp):
    a_int = np.asarray(actions).astype(np.int64)
    return float(np.abs(np.asarray(logp, np.float64) - exp.logp_all[np.arange(a_int.size), a_int]).max())
