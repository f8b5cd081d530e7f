"""Every rollout sampling path against a float64 policy and a host Philox (tests/rollout_ref.py).

All rollout kernels share one epilogue (categorical_act_mask, csrc/mlp_core.h): dead-action mask, softmax on the hardware exp2 / log2,
argmax or inverse-CDF sampling, log-prob.  Sampling is exactly reproducible on the host (the contract stated at mappo_actor_act in
include/mappo_hip.h), so each case says row by row which action a kernel must return:

    clear rows          exactly the expected action
    near-boundary rows  (u within delta of a CDF boundary / top-two logit gap below delta_z) one of the boundary's neighbours
    every row           an available action, and a log-prob within tol of the float64 log-prob of the action returned
    values, next hidden states within their own tol

tol = 4 err32 + 2e-6 with err32 the error of the same oracle module evaluated in float32 on the CPU against float64;
delta = 2 tol + 32 * 2^-23, delta_z = 2 tol.  Near-boundary rows are at most 2 % of a case (checked on the CPU, from the
reference and the host Philox alone).  Each case runs three ways: sampling with seed 2^33 + 12345, counter 2^32 + 7 and a non-NULL
counter_dev holding 2^32 + 3; the same with counter_dev NULL; deterministic.

MATRIX is a covering design of the kernel instances behind mappo_actor_act, mappo_rollout_step, mappo_rollout_episode(_spread),
mappo_gru_forward (head_mode 2), mappo_gru_step_dual, mappo_recurrent_step_dual and mappo_recurrent_rollout_step;
test_rollout_matrix_covers_every_instance checks that on the CPU through a Python mirror of the host dispatch.
mappo_rollout_episode and mappo_rollout_episode_spread take no available actions (their ABI has none), so their cases run unmasked.
The simple_spread episode draws its observations inside the launch: its reference is evaluated on the buffer's own obs_buf[t]
after the run, and its near-boundary share is asserted there instead of in the CPU test."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

import rollout_ref as R
from oracle import mappo_oracle as O
from test_gpu_kernels import dev, _flat_from_module, _randomize, ops   # noqa: F401  (ops: the module-level fixture)

SEED, COUNTER, COUNTER_DEV = 2 ** 33 + 12345, 2 ** 32 + 7, 2 ** 32 + 3
MODES = (("sample+counter_dev", False, COUNTER_DEV), ("sample", False, None), ("deterministic", True, None))
NEAR_CAP = 0.02
INPUT_SEED = 1000                 # chosen on the CPU so that test_rollout_matrix_near_boundary_share holds for every case
HID, NUM_CU = 64, 256
T, F = True, False


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- the matrix ----------------------------------------------------------------------------------------------------------------
# ep: entry point; D / S: actor / critic in_dim; N, M: threads x agents (M = 0: B = N contiguous rows); TT: episode steps;
# cen: centralized critic rows; ins: fused insert; edge: an exact edge case (see _edge_*)
Case = namedtuple("Case", "ep D S A relu LN fn N M TT cen ins edge", defaults=(0, 0, F, F, None))


def act(D, A, relu, LN, fn, B, edge=None):
    return Case("act", D, 0, A, relu, LN, fn, B, edge=edge)


MATRIX = [
    # mappo_actor_act, narrow: mlp_forward_kernel<RELU, LN, 1, XW> — 12 instances; D in {1, 7, 32, 33, 64}, A in {1, 5, 8, 9, 16, 17, 32}
    act(1, 1, T, 0, F, 1), act(7, 5, F, 0, T, 47), act(32, 8, T, 1, F, 130), act(7, 9, F, 1, T, 130), act(32, 16, T, 2, T, 47),
    act(1, 17, F, 2, T, 130), act(33, 32, T, 0, T, 130), act(64, 5, F, 0, F, 47), act(33, 17, T, 1, T, 47), act(64, 9, F, 1, T, 1),
    act(64, 32, T, 2, T, 130), act(33, 8, F, 2, F, 47),
    act(18, 5, T, 1, T, 256 * 4 * 32 + 40),              # grid capped at 256 workgroups: a wave walks a second tile; ragged last tile
    # ... wide: split-K (<= 256 16-row tiles) and streamed
    act(65, 5, T, 1, T, 37), act(130, 17, F, 0, T, 300), act(512, 32, T, 2, F, 37), act(512, 9, F, 1, T, 300),
    act(70, 9, T, 1, T, 4100 + 9),
    # mappo_rollout_step, narrow rollout_step_kernel<RELU, LN>: strided (n, m) rows (centralized and not), contiguous rows, B > 8192
    Case("step", 18, 54, 5, T, 1, T, 37, 3, cen=T, ins=T), Case("step", 18, 18, 9, F, 0, T, 37, 3),
    Case("step", 7, 33, 17, T, 0, F, 47), Case("step", 64, 64, 32, F, 2, F, 130), Case("step", 33, 7, 8, T, 2, T, 47),
    Case("step", 20, 60, 16, F, 1, T, 5, 3, cen=T, ins=T), Case("step", 18, 54, 5, T, 1, T, 8192 + 69),
    # ... wide_rollout_step_kernel
    Case("step", 130, 70, 9, F, 0, T, 37), Case("step", 176, 322, 18, T, 2, F, 300),
    # ... wide_rollout_full_kernel: 256 / 512 on both networks, with and without the fused insert; 16 405 rows = 1 026 tiles on 1 024 waves
    Case("step", 256, 256, 5, T, 1, T, 3281, 5, ins=T), Case("step", 256, 256, 17, F, 0, T, 9, 3),
    Case("step", 512, 512, 9, T, 1, F, 37, 7, ins=T), Case("step", 512, 512, 32, T, 2, T, 300, 5),
    # mappo_rollout_episode: rollout_episode_kernel<RELU, LN>; T = 3, N M = 3 * 37 + 5 and one size with >= 2 items per wave
    Case("episode", 18, 36, 5, T, 1, T, 58, 2, 3, cen=T), Case("episode", 7, 7, 17, F, 0, T, 116, 1, 3),
    Case("episode", 30, 60, 32, T, 2, F, 58, 2, 3, cen=T), Case("episode", 33, 33, 9, F, 1, F, 29, 4, 3),
    Case("episode", 12, 24, 8, T, 0, T, 58, 2, 3, cen=T), Case("episode", 16, 16, 16, F, 2, T, 116, 1, 3),
    Case("episode", 18, 54, 5, T, 1, T, 1100, 3, 3, cen=T),
    # mappo_gru_forward head_mode 2, L = 1 (gru_step3_kernel<2>); Nc = 16 * 513: the grid is capped at 512 workgroups
    Case("gru_fwd", 12, 0, 5, T, 1, T, 5), Case("gru_fwd", 12, 0, 17, T, 1, T, 37), Case("gru_fwd", 12, 0, 32, T, 1, T, 5),
    Case("gru_fwd", 12, 0, 5, T, 1, T, 16 * 513),
    # mappo_gru_step_dual: Nc past the 256-workgroup cap per network
    Case("gru_dual", 12, 20, 5, T, 1, T, 16 * 257 + 3), Case("gru_dual", 12, 20, 17, T, 1, T, 16 * 257 + 3),
    Case("gru_dual", 12, 20, 32, T, 1, T, 16 * 257 + 3),
    # mappo_recurrent_step_dual: gru_step3f_dual_kernel<TR, TLN> (4 instances) and the wide split-K form
    Case("rec_dual", 30, 48, 9, T, 1, T, 116), Case("rec_dual", 7, 64, 17, F, 1, T, 47), Case("rec_dual", 30, 48, 32, T, 0, F, 47),
    Case("rec_dual", 7, 64, 5, F, 0, T, 116), Case("rec_dual", 176, 322, 18, T, 1, T, 300), Case("rec_dual", 130, 70, 5, F, 0, T, 37),
    # mappo_recurrent_rollout_step: the row mask comes from `dones`
    Case("rec_roll", 30, 48, 9, T, 1, T, 37, 3), Case("rec_roll", 176, 322, 18, T, 1, T, 9, 10),
]


def _id(c):
    s = f"{c.ep}-D{c.D}" + (f"-S{c.S}" if c.S else "") + f"-A{c.A}-{'relu' if c.relu else 'tanh'}-LN{c.LN}-N{c.N}" + (f"-M{c.M}" if c.M else "")
    return s + ("-cen" if c.cen else "") + ("-ins" if c.ins else "") + (f"-{c.edge}" if c.edge else "")


IDS = [f"{i:02d}-{_id(c)}" for i, c in enumerate(MATRIX)]

# exact edge cases on one narrow, one wide and one recurrent entry point
EDGES = [Case(ep, D, S, A, T, 1, T, 130, edge=e)
         for ep, D, S in (("act", 18, 0), ("act", 130, 0), ("rec_dual", 30, 48))
         for e, A in (("flat", 9), ("flat", 32), ("single", 5), ("a31", 32), ("a16", 17))]
EDGE_IDS = [_id(c) for c in EDGES]


def rows_of(c):
    return c.N * c.M if c.M else c.N


# ---- Python mirror of the host dispatch -------------------------------------------------------------------------------------------
def act_instance(c):
    """launch_forward<1> (csrc/mlp.hip): wide inputs split-K up to WIDE_SK_MAX_TILES = 256 16-row tiles (mlp_launch.h;
    wide16_launch_forward_sk) else streamed (wide16_launch_forward); narrow mlp_forward_kernel<RELU, LN, 1, XW>, XW by in_dim."""
    if c.D > 64:
        return ("wide_sk" if _cdiv(c.N, 16) <= 256 else "wide_streamed",)
    return ("narrow", c.relu, c.LN, 1 if c.D > 32 else 0)


def act_walks(c):
    """launch_forward (csrc/mlp.hip): 32-row tiles, up to 4 waves per workgroup (fit_waves can only lower that), at most NUM_CU workgroups."""
    n_tiles = _cdiv(c.N, 32)
    nw = 4 if n_tiles >= 4 else (2 if n_tiles >= 2 else 1)
    return n_tiles > min(_cdiv(n_tiles, nw), NUM_CU) * nw


def step_instance(c):
    """mappo_rollout_step (csrc/mlp_step.hip): wide -> wide_rollout_full_kernel for 256 / 512 on both networks and at most two
    tiles per wave (full_step / fuse_ins: fused insert only for uncentralized rows with agent stride in_dim), else
    wide_rollout_step_kernel; narrow -> rollout_step_kernel<RELU, LN>, at most NUM_CU / 2 workgroups of <= 4 waves x 16 rows per network."""
    B = rows_of(c)
    if c.D > 64:
        full = c.D == c.S and c.D in (256, 512) and _cdiv(B, 16) <= 2 * 8 * (NUM_CU // 2)
        return ("full", c.D, bool(c.ins and not c.cen)) if full else ("wide",)
    return ("narrow", c.relu, c.LN)


def step_tiles_per_wave(c):
    n_tiles = _cdiv(rows_of(c), 16)
    if c.D > 64:
        return _cdiv(n_tiles, min(_cdiv(n_tiles, 8), NUM_CU // 2) * 8)            # mappo_rollout_step, wide branch: n_groups / nb
    nw = 4 if n_tiles >= 4 else (2 if n_tiles >= 2 else 1)
    return _cdiv(n_tiles, min(_cdiv(n_tiles, nw), NUM_CU // 2) * nw)


def episode_items_per_wave(c):
    """mappo_rollout_episode (csrc/mlp_step.hip): (step, tile) items dealt over 4 NUM_CU waves, split by item cost 150 : 134."""
    n_tiles, n_net = _cdiv(c.N * c.M, 16), 4 * NUM_CU
    items_a, items_c = c.TT * n_tiles, (c.TT + 1) * n_tiles
    best, wa = None, 1
    for a in range(1, n_net):
        l = max(_cdiv(items_a, a) * 150, _cdiv(items_c, n_net - a) * 134)
        if best is None or l < best:
            best, wa = l, a
    return _cdiv(items_a, min(wa, items_a))


def gru_instance(c):
    """gru.hip: mappo_gru_forward L = 1, head_mode 2 -> gru_step3_kernel<2>, min(tiles, 2 NUM_CU) workgroups (:314-320);
    mappo_gru_step_dual min(tiles, NUM_CU) per network (:364-366); mappo_recurrent_step_dual / mappo_recurrent_rollout_step: wide when
    both in_dim > 64 (:391-394, :447-450), else gru_step3f_dual(_ins)_kernel<TR, TLN> (:409-412, :470-473)."""
    if c.ep in ("rec_dual", "rec_roll"):
        return (c.ep, "wide") if min(c.D, c.S) > 64 else (c.ep, c.relu, c.LN)
    return (c.ep,)


def test_rollout_matrix_covers_every_instance():
    by = lambda ep: [c for c in MATRIX if c.ep == ep]
    a = by("act")
    assert {act_instance(c) for c in a} == {("narrow", r, ln, xw) for r in (T, F) for ln in (0, 1, 2) for xw in (0, 1)} | \
        {("wide_sk",), ("wide_streamed",)}
    narrow = [c for c in a if c.D <= 64]
    assert {c.D for c in narrow} >= {1, 7, 32, 33, 64} and {c.A for c in narrow} >= {1, 5, 8, 9, 16, 17, 32}
    assert {c.N for c in narrow} >= {1, 47, 130} and any(act_walks(c) and c.N % 32 for c in narrow)
    sk = [c for c in a if act_instance(c) == ("wide_sk",)]
    assert {c.D for c in sk} >= {65, 130, 512} and {c.N for c in sk} >= {37, 300}
    s = by("step")
    assert {step_instance(c) for c in s} == {("narrow", r, ln) for r in (T, F) for ln in (0, 1, 2)} | {("wide",)} | \
        {("full", d, i) for d in (256, 512) for i in (T, F)}
    sn = [c for c in s if c.D <= 64]
    assert {(c.M > 0, c.cen) for c in sn} == {(T, T), (T, F), (F, F)} and any(step_tiles_per_wave(c) >= 2 and rows_of(c) > 8192 for c in sn)
    assert {(c.D, c.S) for c in s if step_instance(c) == ("wide",)} >= {(130, 70), (176, 322)}
    assert any(step_instance(c)[0] == "full" and step_tiles_per_wave(c) == 2 for c in s)
    e = by("episode")
    assert {(c.relu, c.LN) for c in e} == {(r, ln) for r in (T, F) for ln in (0, 1, 2)} and all(c.TT == 3 for c in e)
    assert any(c.N * c.M == 3 * 37 + 5 for c in e) and any(episode_items_per_wave(c) >= 2 for c in e) and {c.cen for c in e} == {T, F}
    g = by("gru_fwd")
    assert {c.A for c in g} >= {5, 17, 32} and {c.N for c in g} >= {5, 37} and any(_cdiv(c.N, 16) > 2 * NUM_CU for c in g)
    d = by("gru_dual")
    assert {c.A for c in d} >= {5, 17, 32} and all(c.N == 16 * 257 + 3 and _cdiv(c.N, 16) > NUM_CU for c in d)
    r = by("rec_dual")
    assert {gru_instance(c) for c in r} == {("rec_dual", tr, ln) for tr in (T, F) for ln in (0, 1)} | {("rec_dual", "wide")}
    assert {(c.D, c.S) for c in r} >= {(30, 48), (7, 64), (176, 322), (130, 70)}
    assert {gru_instance(c)[1] == "wide" for c in by("rec_roll")} == {T, F}
    assert {c.ep for c in MATRIX} == {"act", "step", "episode", "gru_fwd", "gru_dual", "rec_dual", "rec_roll"}
    # the exact edge cases: a narrow, a wide and a recurrent entry point
    assert {act_instance(c)[0] if c.ep == "act" else c.ep for c in EDGES} == {"narrow", "wide_sk", "rec_dual"}


# ---- inputs and the float64 reference -----------------------------------------------------------------------------------------------
def _avail(rng, B, A):
    """About 30 % dead actions, at least one available per row, every 7th row with a single available action."""
    av = (rng.random((B, A)) > 0.3).astype(np.float32)
    av[np.arange(B), rng.integers(0, A, B)] = 1.0
    single = np.arange(0, B, 7)
    av[single] = 0.0
    av[single, rng.integers(0, A, single.size)] = 1.0
    return av


def _edge(c, rng, actor, B):
    """Exact edge cases.  flat: zero head weights and a constant bias, so all logits are bit-equal; single: one available action per
    row; a31 / a16: only the last action of A = 32 (bit 31 of the dead mask) / of A = 17 (the second head block)."""
    if c.edge == "flat":
        with torch.no_grad():
            actor.act.action_out.linear.weight.zero_()
            actor.act.action_out.linear.bias.fill_(0.375)
        return _avail(rng, B, c.A)
    av = np.zeros((B, c.A), np.float32)
    av[np.arange(B), rng.integers(0, c.A, B) if c.edge == "single" else c.A - 1] = 1.0
    return av


@functools.lru_cache(maxsize=None)
def _inputs(c):
    """Networks (head weights x 40 through _randomize), rows, masks and the float64 / float32 CPU evaluations of case `c`.
    z: masked float64 logits [steps * B][A] with row index idx and step t; v: float64 values; ha / hc: next states."""
    f = np.float32
    B, A = rows_of(c), c.A
    key = INPUT_SEED + sum(ord(ch) for ch in c.ep) + 31 * c.D + 7 * c.S + 3 * A + B + (len(c.edge) if c.edge else 0)
    torch.manual_seed(key)
    rng = np.random.default_rng(key)
    rec = c.ep in ("gru_fwd", "gru_dual", "rec_dual", "rec_roll")
    a = O.default_args(use_ReLU=c.relu, layer_N=c.LN, use_feature_normalization=c.fn, use_recurrent_policy=rec)
    actor = O.ActorRef(a, c.D, A)
    critic = O.CriticRef(a, c.S) if c.S else None
    _randomize(actor, key + 3)
    if critic is not None:
        _randomize(critic, key + 4)
    x = dict(c=c, a=a, actor=actor, critic=critic, B=B, steps=1)
    no_avail = c.ep == "episode"
    avail = None if no_avail else (_edge(c, rng, actor, B) if c.edge else _avail(rng, B, A))
    x["avail"] = avail
    n = lambda *s: rng.standard_normal(s).astype(f)
    if rec:
        x["ha0"], x["hc0"] = n(B, HID) * 0.5, n(B, HID) * 0.5
        if c.ep == "rec_roll":
            dones = rng.random((c.N, c.M)) < 0.4
            dones[::3] = True                                                 # env done: every agent's state is zeroed
            x["dones"] = dones
            x["masks"] = np.repeat(1.0 - dones.all(axis=1).astype(f), c.M)
            assert 0 < x["masks"].sum() < B
        else:
            x["masks"] = (rng.random(B) > 0.3).astype(f)
            x["masks"][0] = 0.0
    if c.ep in ("gru_fwd", "gru_dual"):
        # the entry points take trunk features: the float32 trunk output on the host is the kernels' input and the reference's
        with torch.no_grad():
            x["fa"] = actor.base(torch.from_numpy(n(B, c.D))).numpy()
            ev = lambda dt: R.head_eval(actor, x["fa"], avail, x["ha0"], x["masks"], dt)
            if critic is not None:
                x["fc"] = critic.base(torch.from_numpy(n(B, c.S))).numpy()
                evc = lambda dt: R.critic_head_eval(critic, x["fc"], x["hc0"], x["masks"], dt)
    elif c.ep == "episode":
        Tn, N, M, D = c.TT, c.N, c.M, c.D
        x["steps"] = Tn
        x["pool"] = n(Tn, N, M * D + 1)                                      # env output of every step, thread stride M D + 1
        x["obs0"] = n(N, M, D)
        env = x["pool"][:, :, :M * D].reshape(Tn, N, M, D)
        rows_a = np.concatenate([x["obs0"][None], env[:Tn - 1]]).reshape(Tn * B, D)
        allr = np.concatenate([x["obs0"][None], env])                       # [T + 1][N][M][D]
        rows_c = (np.repeat(allr.reshape(Tn + 1, N, 1, M * D), M, axis=2) if c.cen else allr).reshape((Tn + 1) * B, c.S)
        x["dones"] = rng.random((Tn, N, M)) < 0.3
        ev = lambda dt: R.actor_eval(actor, rows_a, None, dtype=dt)
        evc = lambda dt: R.critic_eval(critic, rows_c, dtype=dt)
    else:
        if c.M and c.ep == "step":
            x["blk"] = n(c.N, c.M * c.D + 1)                                # strided (n, m) view: thread stride M D + 1
            obs = x["blk"][:, :c.M * c.D].reshape(B, c.D)
            sobs = np.repeat(x["blk"][:, :c.M * c.D], c.M, axis=0) if c.cen else obs
            x["dones_ins"] = rng.random((c.N, c.M)) < 0.5
        else:
            obs, sobs = n(B, c.D), (n(B, c.S) if c.S else None)
        x["obs"], x["sobs"] = np.ascontiguousarray(obs), (np.ascontiguousarray(sobs) if sobs is not None else None)
        ev = lambda dt: R.actor_eval(actor, x["obs"], avail, x.get("ha0"), x.get("masks"), dt)
        if critic is not None:
            evc = lambda dt: R.critic_eval(critic, x["sobs"], x.get("hc0"), x.get("masks"), dt)
    (z, ha), (z32, ha32) = ev(torch.float64), ev(torch.float32)
    x["z"], x["ha"] = z, ha
    x["err32"], x["tol"] = R.err_and_tol(z, z32)
    if ha is not None:
        x["err32_ha"], x["tol_ha"] = R.err_and_tol(ha, ha32)
    if critic is not None:
        (v, hc), (v32, hc32) = evc(torch.float64), evc(torch.float32)
        x["v"], x["hc"] = v, hc
        x["err32_v"], x["tol_v"] = R.err_and_tol(v, v32)
        if hc is not None:
            x["err32_hc"], x["tol_hc"] = R.err_and_tol(hc, hc32)
    x["idx"] = np.tile(np.arange(B), x["steps"])
    x["t"] = np.repeat(np.arange(x["steps"]), B)
    x["avail_rows"] = None if avail is None else np.tile(avail, (x["steps"], 1))
    return x


def _uniforms(counter_dev, idx, t):
    ctr = COUNTER + (counter_dev or 0)
    u = np.empty(idx.size)
    for s in np.unique(t):
        u[t == s] = R.uniform24(SEED, ctr + int(s), idx[t == s])
    return u


def _expected(x, det, counter_dev, z=None, avail=None, tol=None):
    z = x["z"] if z is None else z
    avail = x["avail_rows"] if avail is None else avail
    tol = x["tol"] if tol is None else tol
    if det:
        return R.expected_argmax(z, avail, tol)
    return R.expected_sample(z, avail, _uniforms(counter_dev, x["idx"], x["t"]), tol)


def test_rollout_matrix_near_boundary_share():
    """A condition on the inputs, from the reference and the host Philox alone: in every case and mode at most 2 % of the rows sit
    within delta of a CDF boundary (delta_z of a logit tie); masks and edges are what the docstrings say.  The flat edge cases
    (bit-equal logits, float64 CDF k / n) additionally keep every u further than 32 * 2^-23 from every k / n, so the fp32 running sum
    of the kernels cannot move a row across: those cases are then compared exactly."""
    for c in MATRIX + EDGES:
        x = _inputs(c)
        if x["avail"] is not None and not c.edge:
            assert (x["avail"].sum(1) >= 1).all()
        if x["avail"] is not None and not c.edge and c.A > 1 and x["B"] >= 30:
            assert 0.2 < 1 - x["avail"].mean() and (x["avail"].sum(1) >= 1).all() and (x["avail"].sum(1) == 1).any()
        for name, det, cdev in MODES:
            if not c.edge:
                e = _expected(x, det, cdev)
                assert e.near.mean() <= NEAR_CAP, f"{_id(c)} {name}: {e.near.sum()} of {e.near.size} rows near a boundary (tol {x['tol']:.2e})"
            if c.edge == "flat" and not det:
                n_av = x["avail"].sum(1)
                u = _uniforms(cdev, x["idx"], x["t"])
                frac = u * n_av
                assert np.abs(frac - np.round(frac)).min() / n_av.max() > 32 * 2.0 ** -23, f"{_id(c)} {name}: a draw sits on k / n"
    # the counter word is part of the stream: the three counters of a case's modes / steps give different draws
    i = np.arange(64)
    assert not np.array_equal(R.uniform24(SEED, COUNTER, i), R.uniform24(SEED, COUNTER + COUNTER_DEV, i))
    assert not np.array_equal(R.uniform24(SEED, COUNTER, i), R.uniform24(SEED, COUNTER + 1, i))
    assert not np.array_equal(R.uniform24(SEED, COUNTER, i), R.uniform24(SEED & 0xFFFFFFFF, COUNTER, i))       # seed above 2^32
    assert not np.array_equal(R.uniform24(SEED, COUNTER, i), R.uniform24(SEED, COUNTER & 0xFFFFFFFF, i))       # counter above 2^32


def test_host_philox_known_answers():
    """Philox4x32-10 known-answer vectors (Random123 kat_vectors: zero, all-ones and pi-digit counter / key), and the kernels' word
    mapping of (seed, counter, index) onto them."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{int(w):08x}" for w in R.philox4x32_10(ctr, key)) == want
        seed, counter, index = key[0] | key[1] << 32, ctr[2] | ctr[3] << 32, ctr[0] | ctr[1] << 32
        got = R.philox_u32(seed, counter, np.array([index], dtype=np.uint64))
        assert f"{int(got[0]):08x}" == want[:8]
        assert R.uniform24(seed, counter, np.array([index], dtype=np.uint64))[0] == (int(want[:8], 16) >> 8) / 2.0 ** 24
    # vectorised over the index: lane i equals the scalar call
    v = R.philox_u32(SEED, COUNTER, np.arange(5))
    assert [int(R.philox_u32(SEED, COUNTER, np.array([i]))[0]) for i in range(5)] == [int(w) for w in v]


# ---- the GPU side -------------------------------------------------------------------------------------------------------------------
def _nan(*s):
    return torch.full(s, float("nan"), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _upload(ops, x):
    """Flat parameters and device inputs of a case (once per test)."""
    c = x["c"]
    rec = x["actor"].recurrent
    g = dict(da=ops.net_desc(c.D, c.A, c.LN, c.relu, c.fn, recurrent=rec))
    g["pa"] = _flat_from_module(ops, x["actor"], g["da"], "act.action_out.linear")[0]
    if x["critic"] is not None:
        g["dc"] = ops.net_desc(c.S, 1, c.LN, c.relu, c.fn, recurrent=rec)
        g["pc"] = _flat_from_module(ops, x["critic"], g["dc"], "v_out")[0]
    g["avail"] = dev(x["avail"]) if x["avail"] is not None else None
    for k in ("obs", "sobs", "ha0", "hc0", "masks", "blk", "pool", "obs0"):
        if x.get(k) is not None:
            g[k] = dev(x[k])
    for k in ("fa", "fc"):
        if k in x:
            g[k] = dev(x[k].T)                                              # feature-major [64][Nc]
    return g


def _run(ops, x, g, det, cdev):
    """One launch of the case's entry point; returns the outputs as NumPy arrays (row order of x['z'])."""
    c, B = x["c"], x["B"]
    cd = torch.tensor([cdev], dtype=torch.int64, device="cuda") if cdev is not None else None
    actions, logp = _nan(x["steps"], B), _nan(x["steps"], B)
    out = {}
    if c.ep == "act":
        ops.actor_act(g["pa"], g["da"], g["obs"], g["avail"], B, det, SEED, COUNTER, actions.view(B), logp.view(B), counter_dev=cd)
    elif c.ep == "step":
        values = _nan(B)
        ins = None
        if c.M:
            obs = g["blk"][:, :c.M * c.D].view(c.N, c.M, c.D)
            o = (obs, obs.stride(0), obs.stride(1))
            s = (obs, obs.stride(0), 0 if c.cen else obs.stride(1))
            if c.ins:
                rew = torch.randn(c.N, 1, device="cuda").expand(c.N, c.M)
                dn = dev(x["dones_ins"], torch.bool)
                ins = dict(obs_dst=_nan(c.N, c.M, c.D), share_dst=_nan(c.N, c.M, c.S), rewards=(rew, rew.stride(0), rew.stride(1)),
                           dones=(dn, dn.stride(0), dn.stride(1)), rew_dst=_nan(c.N, c.M, 1), mask_dst=_nan(c.N, c.M, 1), centralized=c.cen)
        else:
            o, s = (g["obs"], 0, 0), (g["sobs"], 0, 0)
        ops.rollout_step(g["pa"], g["da"], g["pc"], g["dc"], o, s, c.M, B, g["avail"], det, SEED, COUNTER, cd, actions.view(B), logp.view(B),
                         values, ins)
        out["v"] = _np(values)
        if ins is not None:                                                  # the fused insert rode along: the slots hold the rows read
            np.testing.assert_array_equal(_np(ins["obs_dst"]).reshape(B, c.D), x["obs"])
            np.testing.assert_array_equal(_np(ins["share_dst"]).reshape(B, c.S), x["sobs"])
            np.testing.assert_array_equal(_np(ins["mask_dst"]).reshape(c.N, c.M), 1.0 - x["dones_ins"])
    elif c.ep == "episode":
        Tn, N, M, D, S = c.TT, c.N, c.M, c.D, c.S
        env = g["pool"][:, :, :M * D].view(Tn, N, M, D)
        rew = torch.randn(Tn, N, 1, device="cuda").expand(Tn, N, M)
        dn = dev(x["dones"], torch.bool)
        obs_buf, share_buf = _nan(Tn + 1, B, D), _nan(Tn + 1, B, S)
        obs_buf[0] = g["obs0"].view(B, D)
        share_buf[0] = g["obs0"].view(N, 1, M * D).expand(N, M, M * D).reshape(B, S) if c.cen else g["obs0"].view(B, D)
        rew_buf, mask_buf, values, nxt = _nan(Tn, B), _nan(Tn + 1, B), _nan(Tn, B), _nan(B)
        ops.rollout_episode(g["pa"], g["da"], g["pc"], g["dc"], env, rew, dn, det, SEED, COUNTER, cd, obs_buf, share_buf, rew_buf, mask_buf,
                            actions, logp, values, nxt, c.cen)
        out["v"] = np.concatenate([_np(values).reshape(-1), _np(nxt)])
        np.testing.assert_array_equal(_np(obs_buf[1:]), _np(env).reshape(Tn, B, D))
    elif c.ep == "gru_fwd":
        hl = _nan(B, HID)
        ops.gru_forward(g["pa"], g["da"], g["fa"], g["ha0"], None, g["masks"], None, 1, B, h_last=hl, head_mode=2, avail=g["avail"],
                        deterministic=det, seed=SEED, counter=COUNTER, counter_dev=cd, actions=actions.view(B), logp=logp.view(B))
        out["ha"] = _np(hl)
    elif c.ep in ("gru_dual", "rec_dual"):
        hla, hlc, values = _nan(B, HID), _nan(B, HID), _nan(B)
        fn, xa, xc = (ops.gru_step_dual, g["fa"], g["fc"]) if c.ep == "gru_dual" else (ops.recurrent_step_dual, g["obs"], g["sobs"])
        fn(g["pa"], g["da"], xa, g["ha0"], hla, g["pc"], g["dc"], xc, g["hc0"], hlc, g["masks"], B, g["avail"], det, SEED, COUNTER, cd,
           actions.view(B), logp.view(B), values)
        out.update(v=_np(values), ha=_np(hla), hc=_np(hlc))
    elif c.ep == "rec_roll":
        N, M = c.N, c.M
        hla, hlc, values = _nan(B, HID), _nan(B, HID), _nan(B)
        rew = torch.randn(N, 1, device="cuda").expand(N, M)
        dn = dev(x["dones"], torch.bool)
        slot = dict(obs=_nan(B, c.D), share_obs=_nan(B, c.S), available_actions=_nan(B, c.A), rewards=_nan(B), masks=_nan(B), bad_masks=_nan(B),
                    active_masks=_nan(B), rnn_states=_nan(B, HID), rnn_states_critic=_nan(B, HID))
        ops.recurrent_rollout_step(g["pa"], g["da"], g["pc"], g["dc"], g["obs"].view(N, M, c.D), g["sobs"].view(N, M, c.S),
                                   g["avail"].view(N, M, c.A), rew, dn, None, g["ha0"], g["hc0"], hla, hlc, det, SEED, COUNTER, cd,
                                   actions.view(B), logp.view(B), values, slot)
        out.update(v=_np(values), ha=_np(hla), hc=_np(hlc))
        np.testing.assert_array_equal(_np(slot["masks"]), x["masks"])          # the mask the kernel derived from `dones`
    else:
        raise AssertionError(c.ep)
    torch.cuda.synchronize()
    out["actions"], out["logp"] = _np(actions).reshape(-1), _np(logp).reshape(-1)
    return out


def _check(x, out, name, det, cdev, what):
    """All assertions of one mode; returns (failures, summary line)."""
    e = _expected(x, det, cdev)
    fails = R.check_actions(e, x["avail_rows"], out["actions"], out["logp"], x["tol"], f"{what} {name}")
    line = (f"{what} | {name} | rows {e.near.size} | err32 {x['err32']:.2e} tol {x['tol']:.2e} | near {int(e.near.sum())} | "
            f"logp err {R.max_logp_err(e, np.nan_to_num(out['actions']).clip(0, x['c'].A - 1), out['logp']):.2e}")
    for k, nm in (("v", "values"), ("ha", "actor next state"), ("hc", "critic next state")):
        if k in out:
            err = float(np.abs(out[k].astype(np.float64) - x[k]).max()) if np.isfinite(out[k]).all() else float("inf")
            line += f" | {nm} err32 {x['err32_' + k]:.2e} tol {x['tol_' + k]:.2e} err {err:.2e}"
            if not err <= x["tol_" + k]:
                fails.append(f"{what} {name}: {nm} off by {err:.3e} > tol {x['tol_' + k]:.3e} (err32 {x['err32_' + k]:.3e})")
    return fails, line


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(MATRIX)), ids=IDS)
def test_rollout_matrix_vs_float64_and_host_philox(ops, monkeypatch, idx):
    """See the module docstring.  Every mode's err32, tol, near-boundary count and measured errors are printed and carried in the
    assertion message.  Measured on an MI355X, all cases passing, no path needed more than the factor 4 (per group over its runs =
    cases x 3 modes: largest err32, largest tol, near-boundary rows, largest log-prob error, largest error / tol over log-probs,
    values and next states):
        actor_act narrow     39 runs  err32 6.4e-07  tol 4.5e-06  near 5 of 101 085  logp 8.3e-07  0.19
        actor_act wide       15       7.2e-07        4.9e-06      1 of 14 349        6.9e-07       0.15
        rollout_step narrow  21       5.6e-07        4.3e-06      3 of 26 166        5.7e-07       0.31
        rollout_step wide     6       8.7e-07        5.5e-06      0 of 1 011         9.9e-07       0.26
        rollout_step full    12       1.1e-06        6.5e-06      2 of 54 573        1.6e-06       0.25
        rollout_episode      21       6.5e-07        4.6e-06      3 of 35 964        7.4e-07       0.25
        episode_spread        3       4.9e-07        3.9e-06      0 of 1 332         3.9e-07       0.16
        gru_forward          12       3.9e-07        3.6e-06      1 of 24 765        4.2e-07       0.13
        gru_step_dual         9       6.7e-07        4.7e-06      7 of 37 035        5.8e-07       0.17
        recurrent_step_dual  18       8.1e-07        5.3e-06      1 of 1 989         6.9e-07       0.20
        recurrent_rollout     6       6.8e-07        4.7e-06      0 of 603           6.3e-07       0.18"""
    for k in ("MAPPO_WIDE_FULL_STEP", "MAPPO_WIDE_NO_SK", "MAPPO_WIDE_SK_TILES", "MAPPO_EPISODE_WAVES", "MAPPO_EPISODE_NET_WAVES",
              "MAPPO_EPISODE_INS_WAVES", "MAPPO_EPISODE_COST_A"):
        monkeypatch.delenv(k, raising=False)
    c = MATRIX[idx]
    x = _inputs(c)
    g = _upload(ops, x)
    fails, lines = [], []
    for name, det, cdev in MODES:
        f_, line = _check(x, _run(ops, x, g, det, cdev), name, det, cdev, IDS[idx])
        fails += f_
        lines.append(line)
    print("\n" + "\n".join(lines))
    assert not fails, "\n".join(fails + lines)


@pytest.mark.gpu
@pytest.mark.parametrize("c", EDGES, ids=EDGE_IDS)
def test_rollout_exact_edge_cases(ops, c):
    """No tolerance on the action.  flat (bit-equal logits): deterministic returns the first available action, sampling the
    floor(u n)-th of the n available ones, log-prob within 1e-6 of -log n.  single / a31 / a16: the one available action, |log-prob|
    <= 1e-6."""
    x = _inputs(c)
    g = _upload(ops, x)
    av = x["avail"] != 0
    n_av = av.sum(1)
    B = x["B"]
    for name, det, cdev in MODES:
        out = _run(ops, x, g, det, cdev)
        a = out["actions"].astype(np.int64)
        assert (out["actions"] == a).all() and (a >= 0).all() and (a < c.A).all() and av[np.arange(B), a].all(), f"{name}: unavailable action"
        if c.edge == "flat":
            j = np.zeros(B, np.int64) if det else np.floor(_uniforms(cdev, x["idx"], x["t"]) * n_av).astype(np.int64)
            want = np.array([np.flatnonzero(av[b])[j[b]] for b in range(B)])
        else:
            want = np.argmax(av, axis=1)
        np.testing.assert_array_equal(a, want, err_msg=f"{_id(c)} {name}")
        np.testing.assert_allclose(out["logp"], -np.log(n_av), rtol=0, atol=1e-6, err_msg=f"{_id(c)} {name}")


@pytest.mark.gpu
def test_rollout_episode_spread_actions_follow_the_policy(ops):
    """mappo_rollout_episode_spread, M = L = 3, N = 37, T = 4, env_episode_length 3 (a reset falls inside): for every t, actions[t] is
    the expected action of the float64 policy on the buffer's own obs_buf[t] with u from (seed, counter + t, n M + m); log-probs and
    values[t] / next_values against the float64 networks on obs_buf[t] / share_buf[t].  Ties the recorded actions to the policy
    without relying on the env."""
    Mn, L, N, Tn, env_T, A = 3, 3, 37, 4, 3, 5
    D = 4 + 2 * L + 4 * (Mn - 1)
    S, B = Mn * D, N * Mn
    torch.manual_seed(77)
    a = O.default_args()
    actor, critic = O.ActorRef(a, D, A), O.CriticRef(a, S)
    _randomize(actor, 5); _randomize(critic, 6)
    da, dc = ops.net_desc(D, A), ops.net_desc(S, 1)
    pa, pc = _flat_from_module(ops, actor, da, "act.action_out.linear")[0], _flat_from_module(ops, critic, dc, "v_out")[0]
    f64 = dict(dtype=torch.float64, device="cuda")
    fails, lines = [], []
    for name, det, cdev in MODES:
        pos, vel, lpos = torch.zeros(N, Mn, 2, **f64), torch.zeros(N, Mn, 2, **f64), torch.zeros(N, L, 2, **f64)
        tstep, episode = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int64, device="cuda")
        obs0 = _nan(N, Mn, D)
        ops.mpe_spread_reset(pos, vel, lpos, tstep, episode, obs0, N, Mn, L, 9)
        obs_buf, share_buf = _nan(Tn + 1, B, D), _nan(Tn + 1, B, S)
        obs_buf[0] = obs0.view(B, D)
        share_buf[0] = obs0.view(N, 1, S).expand(N, Mn, S).reshape(B, S)
        rew_buf, mask_buf, actions, logp, values, nxt = _nan(Tn, B), _nan(Tn + 1, B), _nan(Tn, B), _nan(Tn, B), _nan(Tn, B), _nan(B)
        cd = torch.tensor([cdev], dtype=torch.int64, device="cuda") if cdev is not None else None
        ops.rollout_episode_spread(pa, da, pc, dc, Tn, N, Mn, L, env_T, 9, pos, vel, lpos, tstep, episode, det, SEED, COUNTER, cd, obs_buf,
                                   share_buf, rew_buf, mask_buf, actions, logp, values, nxt, True)
        torch.cuda.synchronize()
        ob, sb = _np(obs_buf), _np(share_buf)
        assert np.isfinite(ob).all() and np.isfinite(sb).all()
        assert float(_np(mask_buf)[1:].min()) == 0.0 and float(_np(mask_buf)[1:].max()) == 1.0          # a reset fell inside
        np.testing.assert_array_equal(sb.reshape(Tn + 1, N, Mn, S), np.repeat(ob.reshape(Tn + 1, N, 1, S), Mn, axis=2))
        rows_a, rows_c = ob[:Tn].reshape(Tn * B, D), sb.reshape((Tn + 1) * B, S)
        (z, _), (z32, _) = R.actor_eval(actor, rows_a), R.actor_eval(actor, rows_a, dtype=torch.float32)
        (v, _), (v32, _) = R.critic_eval(critic, rows_c), R.critic_eval(critic, rows_c, dtype=torch.float32)
        x = dict(c=Case("spread", D, S, A, T, 1, T, N, Mn, Tn, cen=T), z=z, v=v, avail_rows=None, idx=np.tile(np.arange(B), Tn),
                 t=np.repeat(np.arange(Tn), B))
        x["err32"], x["tol"] = R.err_and_tol(z, z32)
        x["err32_v"], x["tol_v"] = R.err_and_tol(v, v32)
        e = _expected(x, det, cdev)
        assert e.near.mean() <= NEAR_CAP, f"{name}: {e.near.sum()} of {e.near.size} rows near a boundary"
        out = dict(actions=_np(actions).reshape(-1), logp=_np(logp).reshape(-1), v=np.concatenate([_np(values).reshape(-1), _np(nxt)]))
        f_, line = _check(x, out, name, det, cdev, "spread-episode")
        fails += f_
        lines.append(line)
    print("\n" + "\n".join(lines))
    assert not fails, "\n".join(fails + lines)
