"""Host mirror of the synthetic SMAC-shaped env kernels (mappo_amd/csrc/synth_env.hip: mappo_synth_smac_step, mappo_synth_smac_pool)
in NumPy, on top of rollout_ref.philox_u32.

The stream of one step, keyed by (seed, counter); W = D + S + A, total = N * M * W, element e = (agent ag = e // W, column k = e % W):
  element e of obs / share_obs    the normal of Philox words 2e, 2e + 1
  element e of avail (column a)   1 if a == 0 or the uniform of word 2e is <= 0.7f
  death of agent ag               the uniform of word 2 (total + ag)              <= p_death
  termination of env n            the uniform of word 2 (total + N M + n)         <= p_term
  reward of env n                 the normal of words 2 (total + N M + N + n), + 1
A uniform is ((word >> 8) + 1) * 2^-24, in (0, 1], exact in float32 and held exactly in float64 here; the comparisons run against
the float32 values of 0.7, p_death and p_term, as the kernel's do.  A normal is Box-Muller, sqrt(-2 log u1) cos(2 pi u2), in float64
from those exact uniforms.  dones = dead | terminated; a terminated env restarts with every agent alive.  A launch advances the
counter by 1 (step) or by P (pool: step p of a pool draws from counter + p).

A plain helper module: no fixtures, no pytest settings."""
import functools

import numpy as np

from rollout_ref import philox_u32

H = 2.0 ** -24                       # one step of the uniforms' grid
KINDS = ("normal", "avail", "death", "termination", "reward")


# The GPU tests' shapes (N, M, D, S, A), chosen for the number of 256-thread workgroups the launch takes, ceil(P N M W / 256), around
# the 32 groups of the counter advance's ticket scheme; W = D + S + A divides 256 in `one_full` only, so agents straddle workgroups.
STEP_SHAPES = dict(
    minimal=(1, 1, 1, 1, 1),              # total 3
    one_full=(2, 4, 16, 12, 4),           # total 256: exactly one full workgroup
    wg31=(30, 3, 30, 48, 9),              # 7830 elements
    wg32=(23, 4, 30, 48, 9),              # 8004
    wg33=(24, 4, 30, 48, 9),              # 8352: groups of 2, 1, 1, ...
    wg65=(38, 5, 30, 48, 9),              # 16530: groups of 3, 2, 2, ...
    over_cap=(1537, 8, 30, 48, 9),        # 1 069 752 elements, 4179 workgroups' worth on a grid capped at 4096: a second trip
)
# (shape, P): P = 1 on the step's small grids, P = 7 on shapes that give the same workgroup counts, P = 3 at the step's largest shape
# (12 537 workgroups' worth on a grid capped at 8192, the second trip made of st > 0 elements only)
POOL_SHAPES = dict(
    {k + "_p1": (v, 1) for k, v in STEP_SHAPES.items() if k != "over_cap"},
    minimal_p7=((1, 1, 1, 1, 1), 7),      # 21 elements
    wg31_p7=((13, 1, 30, 48, 9), 7),      # 7 x 1131 = 7917
    wg32_p7=((10, 4, 10, 13, 6), 7),      # 7 x 1160 = 8120
    wg33_p7=((41, 1, 10, 13, 6), 7),      # 7 x 1189 = 8323
    wg65_p7=((9, 3, 30, 48, 9), 7),       # 7 x 2349 = 16443
    over_cap_p3=((1537, 8, 30, 48, 9), 3),
)
WORKGROUPS = dict(minimal=1, one_full=1, wg31=31, wg32=32, wg33=33, wg65=65, over_cap=4179, minimal_p1=1, one_full_p1=1, wg31_p1=31,
                  wg32_p1=32, wg33_p1=33, wg65_p1=65, minimal_p7=1, wg31_p7=31, wg32_p7=32, wg33_p7=33, wg65_p7=65, over_cap_p3=12537)
# the cases' seeds (one beyond 32 bits, one beyond 63).  over_cap's is chosen so that the first launch of the stream (counter 1) holds
# an avail draw EXACTLY on the threshold 0.7f = 11744051 * 2^-24 (a chance of 2^-24 per draw): `<=` and `<` differ there
# (tests/test_synth_ref.py holds the seed to it)
SEEDS = dict(minimal=2 ** 40 + 5, one_full=7, wg31=31, wg32=2 ** 63 + 32, wg33=33, wg65=65, over_cap=114)
# the state-machine case: 12 steps from a state that already holds dead agents; the seed is the one tests/test_synth_ref.py holds to
# exercise every transition coverage() counts
STATE_CASE = dict(seed=11, N=37, M=4, D=5, S=7, A=3, p_death=0.3, p_term=0.2, steps=12)


def state_case_dead0():
    N, M = STATE_CASE["N"], STATE_CASE["M"]
    return (np.arange(N * M).reshape(N, M) % 5 == 0)


def workgroups(shape, P=1):
    N, M, D, S, A = shape
    return -(-(P * N * M * (D + S + A)) // 256)


def bases(N, M, D, S, A):
    """(W, total, base_agent, base_env, base_reward): the index spaces of one step's stream."""
    W = D + S + A
    total = N * M * W
    return W, total, total, total + N * M, total + N * M + N


def uniform(seed, counter, word):
    """The uniform in (0, 1] of Philox word index `word` (array), exact in float64."""
    return ((philox_u32(seed, counter, word) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * H


def normal(u1, u2):
    """Box-Muller in float64."""
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def normal_bound(u1, u2):
    """Per element, the largest change of normal(u1, u2) when either uniform moves to a neighbour on its 24-bit grid.  u1 only
    moves inside (0, 1] (every u1 has at least one such neighbour); the cosine is periodic, so u2 moves both ways."""
    return normal_and_bound(u1, u2)[1]


def normal_and_bound(u1, u2):
    """(normal(u1, u2), normal_bound(u1, u2)) from one radius r and one cosine c: a move of u2 changes r c by r |c' - c|, a move of
    u1 by |c| |r' - r|."""
    r, c = np.sqrt(-2.0 * np.log(u1)), np.cos(2.0 * np.pi * u2)
    b = r * np.maximum(np.abs(np.cos(2.0 * np.pi * (u2 + H)) - c), np.abs(np.cos(2.0 * np.pi * (u2 - H)) - c))
    for v in (np.where(u1 + H <= 1.0, u1 + H, u1), np.where(u1 - H > 0.0, u1 - H, u1)):       # a move out of (0, 1]: none
        b = np.maximum(b, np.abs(c) * np.abs(np.sqrt(-2.0 * np.log(v)) - r))
    return r * c, b


def normal_f32(u1, u2):
    """The kernel's formula evaluated in NumPy float32 (for comparison with the device's fast log / cos)."""
    u1, u2 = np.asarray(u1).astype(np.float32), np.asarray(u2).astype(np.float32)
    return np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(6.28318530718) * u2)


def stream_words(N, M, D, S, A):
    """Per kind of draw (KINDS), the array of Philox word indices that kind touches in one step: "normal" (obs / share_obs elements,
    two words each), "avail" (one word each; column 0 draws nothing), "death", "termination" (one word each), "reward" (two)."""
    W, total, b_ag, b_env, b_rew = bases(N, M, D, S, A)
    e = np.arange(total, dtype=np.int64)
    k = e % W
    en, ea = e[k < D + S], e[k > D + S]
    two = lambda i: np.concatenate([2 * i, 2 * i + 1])
    return dict(normal=two(en), avail=2 * ea, death=2 * (b_ag + np.arange(N * M, dtype=np.int64)),
                termination=2 * (b_env + np.arange(N, dtype=np.int64)), reward=two(b_rew + np.arange(N, dtype=np.int64)))


@functools.lru_cache(maxsize=8)
def draws(seed, counter, N, M, D, S, A):
    """Everything of one step that does not depend on the state or the probabilities (computed once per (seed, counter, shape),
    shared read-only among the tests): obs [N, M, D], share [N, M, S], rewards [N] (float64 normals); their per-element bounds
    obs_bound / share_bound / rewards_bound and first uniforms obs_u1 / share_u1 / rewards_u1; f32_ratio (the worst
    |normal_f32 - normal| / bound of the step); avail [N, M, A] float32; the raw uniforms u_death [N, M], u_term [N]."""
    W, total, b_ag, b_env, b_rew = bases(N, M, D, S, A)
    e = np.arange(total, dtype=np.int64).reshape(N, M, W)
    u1 = uniform(seed, counter, 2 * e)
    n1, n2 = u1[..., :D + S], uniform(seed, counter, 2 * e[..., :D + S] + 1)
    z, zb = normal_and_bound(n1, n2)
    avail = (u1[..., D + S:] <= float(np.float32(0.7))).astype(np.float32)
    avail[..., 0] = 1.0
    r = b_rew + np.arange(N, dtype=np.int64)
    r1, r2 = uniform(seed, counter, 2 * r), uniform(seed, counter, 2 * r + 1)
    rz, rb = normal_and_bound(r1, r2)
    f32 = max(float((np.abs(normal_f32(n1, n2) - z) / zb).max()), float((np.abs(normal_f32(r1, r2) - rz) / rb).max()))
    out = dict(obs=z[..., :D], share=z[..., D:], obs_bound=zb[..., :D], share_bound=zb[..., D:], obs_u1=n1[..., :D], share_u1=n1[..., D:],
               rewards=rz, rewards_bound=rb, rewards_u1=r1, f32_ratio=f32, avail=avail,
               u_death=uniform(seed, counter, 2 * (b_ag + np.arange(N * M, dtype=np.int64))).reshape(N, M),
               u_term=uniform(seed, counter, 2 * (b_env + np.arange(N, dtype=np.int64))))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _advance(d, p_death, p_term, dead):
    """The state machine of one step on the draws d -> (died, term, dones, dead_out)."""
    died = d["u_death"] <= float(np.float32(p_death))
    term = d["u_term"] <= float(np.float32(p_term))
    dead = dead | died
    return died, term, dead | term[:, None], dead & ~term[:, None]


def step(seed, counter, N, M, D, S, A, p_death, p_term, dead_in):
    """One launch of mappo_synth_smac_step.  dead_in: [N, M] bool / uint8.  Returns the entries of draws() plus dones / dead_out
    [N, M] bool, died / term (which draws fired) and `counter`, the counter after the launch."""
    o = dict(draws(int(seed), int(counter), N, M, D, S, A))
    o["died"], o["term"], o["dones"], o["dead_out"] = _advance(o, p_death, p_term, np.asarray(dead_in).astype(bool).reshape(N, M))
    o["counter"] = counter + 1
    return o


def pool(seed, counter, N, M, D, S, A, p_death, p_term, dead_in, P):
    """One launch of mappo_synth_smac_pool: obs [P, N, M, D], share, avail, rewards [P, N], dones [P, N, M] (and the bounds and u1 of
    the normals), step p drawn from counter + p with the state carried from step to step; dead_out after the P-th step; the counter
    advanced by P."""
    dead = np.asarray(dead_in).astype(bool).reshape(N, M)
    ds, dones = [draws(int(seed), int(counter) + p, N, M, D, S, A) for p in range(P)], []
    for d in ds:
        _, _, dn, dead = _advance(d, p_death, p_term, dead)
        dones.append(dn)
    o = {k: np.stack([d[k] for d in ds]) for k in ds[0] if k not in ("f32_ratio", "u_death", "u_term")}
    o.update(f32_ratio=max(d["f32_ratio"] for d in ds), dones=np.stack(dones), dead_out=dead, counter=counter + P)
    return o


def run(seed, counter, N, M, D, S, A, p_death, p_term, dead_in, steps):
    """`steps` calls of step(), the state carried along -> (list of the steps' dicts, counter after the last)."""
    out, dead = [], np.asarray(dead_in).astype(bool).reshape(N, M)
    for _ in range(steps):
        out.append(step(seed, counter, N, M, D, S, A, p_death, p_term, dead))
        dead, counter = out[-1]["dead_out"], out[-1]["counter"]
    return out, counter


def extreme_u1(outs):
    """Over a list of step() / pool() results: ((u1, position in the list, array name, flat index) of the normal with the smallest
    u1, the same for the largest u1) — the two ends where sqrt(-2 log u1) is most exposed."""
    lo = hi = None
    for i, o in enumerate(outs):
        for name in ("obs", "share", "rewards"):
            u = o[name + "_u1"].reshape(-1)
            j, k = int(u.argmin()), int(u.argmax())
            if lo is None or u[j] < lo[0]:
                lo = (float(u[j]), i, name, j)
            if hi is None or u[k] > hi[0]:
                hi = (float(u[k]), i, name, k)
    return lo, hi


def coverage(seed, counter, N, M, D, S, A, p_death, p_term, dead_in, steps):
    """Counts, over `steps` steps from dead_in, of the transitions of the state machine: a dict, one entry per transition."""
    c = dict(alive_to_dead=0, dead_stays_dead=0, dead_to_alive_by_termination=0, termination_with_nobody_dead=0,
             termination_and_death_same_step=0)
    dead = np.asarray(dead_in).astype(bool).reshape(N, M)
    for o in run(seed, counter, N, M, D, S, A, p_death, p_term, dead, steps)[0]:
        new = o["died"] & ~dead                                  # agents alive before the step whose death draw fired
        c["alive_to_dead"] += int((~dead & o["dead_out"]).sum())
        c["dead_stays_dead"] += int((dead & o["dead_out"]).sum())
        c["dead_to_alive_by_termination"] += int((dead & o["term"][:, None]).sum())
        c["termination_with_nobody_dead"] += int((o["term"] & ~(dead | o["died"]).any(1)).sum())
        c["termination_and_death_same_step"] += int((o["term"] & new.any(1)).sum())
        dead = o["dead_out"]
    return c
