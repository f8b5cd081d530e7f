"""The fused PPO update launches at edge batch sizes and in the input forms that test_gpu_update_matrix.py does not use.

One pair of networks per kernel family (NETS: upd16 / upd16d, the pair kernel upd2 / upd2d, upd16x, the K-chunked wide kernel) and
two multi-head actors (MD_NETS: mappo_actor_update_md / mappo_actor_critic_update_md); test_edge_networks_cover_every_family
checks through the dispatch mirror of test_gpu_update_matrix.py that they reach every family MATRIX reaches.

  1. test_edge_batches: B in EDGE_B, rows None and gathered, every pair, zero- and NaN-filled buffers; single launches, the dual
     launch (in_dim <= 64) and the unfused sequence against float64 autograd; the NaN run checks the write contract.
     test_active_patterns: a full tile that is entirely inactive, and a batch whose only active row is the 1-row tail tile.
     test_edge_batches_cover_the_tile_walks restates the tile walks (mlp_upd16.h, mlp_upd2.h, mlp_upd.h) and says which B reaches what.
  2. test_avail_none: avail == NULL against the float64 reference without available_actions; bit-identical to an all-ones avail.
  3. test_misaligned_x: obs / share_obs that start 1, 2, 3 floats into an allocation (rows None, so every full tile gathers).
  4. test_accumulate_partials*: cfg.accumulate_partials adds onto the buffer; the rows a network does not own in the dual launch.
  5. test_caller_chosen_grid: n_blocks.

Inputs: every row at least 1e-4 from the ReLU and loss kinks (_draw redraws unsafe rows, never drops one; at least one active row);
cpu_case takes the first seed at which the oracle's own float32 evaluation meets the statistics' bounds (2 of the 128 cases of
test_edge_batches move to seed 1: multi-head policy losses of 1e-2 that are sums of signed terms of magnitude 1).
Tolerances are the project's: gradients within 1e-4 of the float64 tensor's largest entry (exactly zero where that tensor is
zero), statistics rtol 1e-5 / atol 1e-7 (multi-head: 2e-6 relative), two launch forms of one operation 2e-6 / (1e-6, 1e-9).

Measured on the MI355X, worst case over the file (gradients: err / max|ref|, bound 1e-4; statistics: fraction of their bound):

    family   form      gradient   statistic        family   form      gradient   statistic
    upd16    single    2.1e-06    0.38             upd16x   single    2.7e-05    0.06
    upd16    dual      2.1e-06    0.38             upd16x   unfused   2.2e-06    0.06
    upd16    unfused   2.6e-06    0.23             wide     single    5.0e-06    0.13
    upd2     single    3.2e-06    0.17             wide     unfused   7.0e-06    0.40
    upd2     dual      3.0e-06    0.17             md       single    1.2e-06    0.44
    upd2     unfused   2.9e-06    0.35             md       dual      1.2e-06    0.44

The misaligned launches are bit-identical to the aligned ones in every family; accumulated partials meet 1e-12 (|p0| + |fresh|).
No case exposed a fault in the kernels or their dispatch."""
import types

import numpy as np
import pytest
import torch

import md_ref
from oracle import mappo_oracle as O
from test_gpu_kernels import close, close_rel_max, dev, _flat_from_module, _randomize, _relu_margin, _loss_margin
from test_gpu_multidiscrete import _md_reference
from test_gpu_update_matrix import (FLAGS, MATRIX, NUM_CU, TS, UPD16_WAVES, _check_grads, _check_partials, _check_written, _reference,
                                    dual_family, dual_slabs, single_family, upd16_split)

# (actor in_dim, critic in_dim, actions | heads, layer_N, ReLU, feature norm)
NETS = {
    "upd16": (18, 54, 5, 1, True, True),
    "upd16-tanh": (40, 12, 12, 0, False, False),
    "upd2": (36, 54, 5, 1, True, True),                # the actor on the pair kernel, the critic on upd16; dual: upd2d
    "upd2-tanh": (33, 20, 32, 2, False, True),
    "upd16x": (130, 70, 5, 1, True, True),
    "wide": (130, 100, 18, 2, True, True),
}
MD_NETS = {
    "md-5x10": (21, 42, (5, 10), 1, True, True),
    "md-3x3x3x3": (21, 42, (3, 3, 3, 3), 1, False, True),
}
ALL_NETS = dict(NETS, **MD_NETS)
EDGE_B = [1, 15, 16, 17, 31, 32, 33, 129]
NAN = float("nan")


def _families(net):
    D, S, A, LN = net[:4]
    A = sum(A) if isinstance(A, tuple) else A
    fams = {single_family(D, A, LN, True), single_family(S, 1, LN, False)}
    if D <= 64 and S <= 64:
        fams.add(dual_family(D, S, A, LN))
    return fams


def test_edge_networks_cover_every_family():
    """NETS reaches the families MATRIX reaches; the two multi-head actors take the 16-sample-tile kernel, alone and in the dual launch."""
    want = set()
    for D, S, A, LN, *_ in MATRIX:
        want |= _families((D, S, A, LN))
    got = set().union(*(_families(n) for n in NETS.values()))
    assert got == want == {"upd16", "upd16x", "upd2", "wide", "upd16d", "upd2d"}, (got, want)
    assert single_family(36, 5, 1, True) == "upd2" and single_family(54, 1, 1, False) == "upd16"
    for n in MD_NETS.values():
        assert _families(n) == {"upd16", "upd16d"} and len(n[2]) > 1
    assert any(not n[5] for n in NETS.values()) and {n[4] for n in NETS.values()} == {True, False}


# ---- the tile walks, restated --------------------------------------------------------------------------------------------
def walk16(B, nb, n_waves=UPD16_WAVES):
    """update16_body: wave `wave` of workgroup `bid` walks tile0 = wave * nb + bid, then + nb * n_waves; 16-row tiles.
    {(bid, wave): [valid rows of each tile it walks]}."""
    n_tiles = (B + 15) // 16
    return {(bid, w): [min(16, B - 16 * t) for t in range(w * nb + bid, n_tiles, nb * n_waves)] for bid in range(nb) for w in range(n_waves)}


def walk2(B, nb, n_pairs):
    """update2_body: pair `pair` of workgroup `bid` walks tile0 = pair * nb + bid, then + nb * n_pairs; 32-row tiles."""
    n_tiles = (B + TS - 1) // TS
    return {(bid, p): [min(TS, B - TS * t) for t in range(p * nb + bid, n_tiles, nb * n_pairs)] for bid in range(nb) for p in range(n_pairs)}


def walk_wide(B, nb, n_waves):
    """mlp_update_kernel: workgroup `bid` walks block tiles tb = bid, bid + nb, ... < ceil(n_tiles / n_waves); its wave takes tile
    tb * n_waves + wave, which may lie beyond the batch (0 valid rows: the loop is uniform over the workgroup)."""
    n_tiles = (B + TS - 1) // TS
    n_btiles = (n_tiles + n_waves - 1) // n_waves
    return {(bid, w): [max(0, min(TS, B - TS * (tb * n_waves + w))) for tb in range(bid, n_btiles, nb)] for bid in range(nb) for w in range(n_waves)}


def single_grid(B, n_blocks=0):
    nb = min((B + TS - 1) // TS, NUM_CU)                 # mappo_mlp_backward_slabs
    return min(n_blocks, nb) if n_blocks > 0 else nb


def _wg_tiles(walk, bid):
    return sum(len([v for v in t if v > 0]) for (b, _), t in walk.items() if b == bid)


def _reached(bs):
    """The walk properties that the batch sizes `bs` reach, as a set of names."""
    got = set()
    for B in bs:
        nb = single_grid(B)
        nA, nC = upd16_split(18, 54, 5, 1, B)
        for name, w in (("s16", walk16(B, nb)), ("d16", walk16(B, nA)), ("d16", walk16(B, nC))):
            tiles = [t for t in w.values() if t]
            if tiles == [[1]]:
                got.add("16: the only tile has 1 row")
            if tiles == [[15]]:
                got.add("16: the only tile has 15 rows")
            if tiles == [[16]]:
                got.add("16: exactly one full tile")
            if sorted(tiles) == [[1], [16]]:
                got.add("16: a full tile, then a 1-row tile")
            if len(tiles) == 1 and len(w) == UPD16_WAVES:
                got.add("16: one wave with a tile, seven without")
            if name == "s16" and nb == 2 and _wg_tiles(w, 0) != _wg_tiles(w, 1):
                got.add("16: two workgroups, unequal tile counts")
            if name == "s16" and nb > 2 and max(_wg_tiles(w, b) for b in range(nb)) >= 2 and \
                    any(not w[(b, k)] and w[(b, k - 1)] for b in range(nb) for k in range(1, UPD16_WAVES)):
                got.add("16: more than two workgroups of several tiles, a wave without a tile beside one with")
        for n_pairs in (1, 2, 4):
            for nbp in (nb, min(nb, NUM_CU // 2)):
                tiles = [t for t in walk2(B, nbp, n_pairs).values() if t]
                if tiles == [[1]]:
                    got.add("32: the only tile has 1 row")
                if tiles == [[15]]:
                    got.add("32: the only tile has 15 rows")
                if tiles == [[TS]]:
                    got.add("32: exactly one full tile")
                if sorted(tiles) == [[1], [TS]]:
                    got.add("32: a full tile, then a 1-row tile")
        for nw in (1, 2, 4):
            w = walk_wide(B, nb, nw)
            if nw > 1 and any(0 in t for t in w.values()) and any(1 in t for t in w.values()):
                got.add("wide: a 1-row tile beside tiles beyond the batch in one workgroup")
            if nw > 1 and any(not t for t in w.values()) and nb > 1:
                got.add("wide: a workgroup without a block tile")
    return got


WALKS = {"16: the only tile has 1 row", "16: the only tile has 15 rows", "16: exactly one full tile", "16: a full tile, then a 1-row tile",
         "16: one wave with a tile, seven without", "16: two workgroups, unequal tile counts",
         "16: more than two workgroups of several tiles, a wave without a tile beside one with",
         "32: the only tile has 1 row", "32: the only tile has 15 rows", "32: exactly one full tile", "32: a full tile, then a 1-row tile",
         "wide: a 1-row tile beside tiles beyond the batch in one workgroup", "wide: a workgroup without a block tile"}


def test_edge_batches_cover_the_tile_walks():
    """EDGE_B reaches every walk property in WALKS, and each of B = 1, 15, 16, 17, 32, 33, 129 is the only one to reach some property
    (31 is the ragged single 32-row tile next to 15: it adds no property of its own and is kept as the issue lists it).

    A default grid never gives a wave a second tile below B = 32 768: nb = min(ceil(B / 32), 256) workgroups of 8 waves (4 pairs at
    most) hold 4 B rows.  What B = 129 adds is a launch of several workgroups with several tiles each in which waves without a tile
    sit beside waves with one.  Waves that walk two and three tiles, beside waves that walk none in the same launch, come from the
    caller-chosen grid (test_caller_chosen_grid: B = 333 on 1 and 3 workgroups); that is asserted here, too."""
    assert _reached(EDGE_B) == WALKS, WALKS - _reached(EDGE_B)
    for B in (1, 15, 16, 17, 32, 33, 129):
        assert _reached([b for b in EDGE_B if b != B]) != WALKS, f"B = {B} covers nothing of its own"
    for B in EDGE_B:
        for w in (walk16(B, single_grid(B)), walk2(B, single_grid(B), 1), walk16(B, min(upd16_split(18, 54, 5, 1, B)))):
            assert max(len(t) for t in w.values()) == 1
    w1, w3 = walk16(333, single_grid(333, 1)), walk16(333, single_grid(333, 3))
    assert sorted({len(t) for t in w1.values()}) == [2, 3] and sorted({len(t) for t in w3.values()}) == [0, 1]
    assert max(len(t) for t in walk2(333, 1, 4).values()) == 3 and single_grid(333) == 11 and single_grid(333, 16) == 11


# ---- cases ---------------------------------------------------------------------------------------------------------------
def _margin(a, actor, critic, heads, relu, obs, sobs, actions, avail, active, old_logp, v_old, ret, vn):
    """Distance of every row to the nearest kink (test_gpu_kernels._relu_margin / _loss_margin; multi-head: every head's ratio)."""
    f = np.float32
    n = obs.shape[0]
    A = actor.act.action_out.linear.out_features
    ones = np.ones((n, A), f)
    if heads is None:
        m = _loss_margin(a, actor, critic, obs, sobs, actions, ones if avail is None else avail, active, old_logp, v_old, ret, vn)
    else:
        import copy
        ad = copy.deepcopy(actor).double()
        with torch.no_grad():
            z = ad.act.logits(ad.features(torch.from_numpy(obs).double(), None, None)[0], None)
            lp, _ = md_ref.evaluate_heads(z, heads, torch.from_numpy(actions).double())
            lp0 = ad.evaluate_actions(torch.from_numpy(obs).double(), None, torch.zeros(n, 1).double(), None, torch.from_numpy(ones).double(),
                                      torch.from_numpy(active).double().view(-1, 1))[0].numpy().reshape(-1)
        r = torch.exp(lp - torch.from_numpy(old_logp).double())
        c = a.clip_param
        m = torch.minimum((r - (1 - c)).abs(), (r - (1 + c)).abs()).min(1).values.numpy()
        # the critic's kinks: _loss_margin with a ratio of exactly 1 on its (single-head) actor side
        m = np.minimum(m, _loss_margin(a, actor, critic, obs, sobs, np.zeros(n, f), ones, active, lp0.astype(np.float64), v_old, ret, vn))
    if relu:
        m = np.minimum(m, np.minimum(_relu_margin(actor, torch.from_numpy(obs)), _relu_margin(critic, torch.from_numpy(sobs))))
    return m


def _draw(a, actor, critic, rng, n_rows, rows, D, S, A, heads, relu, pattern, with_avail, safe):
    """Loss inputs as test_gpu_update_matrix._safe_inputs draws them, for any n_rows >= 1: unsafe rows are redrawn until none is
    left (20 rounds at most), never deactivated or dropped.  `pattern` sets the active mask by minibatch position."""
    f = np.float32
    B = rows.size
    obs = rng.standard_normal((n_rows, D)).astype(f)
    sobs = rng.standard_normal((n_rows, S)).astype(f)
    if heads is None:
        actions = rng.integers(0, A, n_rows).astype(f)
        avail = (rng.random((n_rows, A)) > 0.3).astype(f)
        avail[np.arange(n_rows), actions.astype(int)] = 1.0
        if B >= 15:                                   # rows whose only available action is the one taken: probability 1, entropy 0
            for pos in (1, 7):
                avail[rows[pos]] = 0.0
                avail[rows[pos], int(actions[rows[pos]])] = 1.0
        if not with_avail:
            avail = None
        logn = np.log(A)
        draw_old = lambda k: (-np.abs(rng.standard_normal(k)) * 0.3 - logn).astype(f)
    else:
        actions = np.stack([rng.integers(0, d, n_rows) for d in heads], 1).astype(f)
        avail = None
        logn = np.log(np.asarray(heads, f))
        draw_old = lambda k: (-np.abs(rng.standard_normal((k, len(heads)))) * 0.3 - logn).astype(f)
    old_logp = draw_old(n_rows)
    adv = rng.standard_normal(n_rows).astype(f)
    active = (rng.random(n_rows) > 0.25).astype(f)
    if pattern == "tile_off":                         # minibatch rows 16..31: a tile that must contribute exactly nothing
        active[rows] = 1.0
        active[rows[16:32]] = 0.0
    elif pattern == "last_only":                      # the 1-row tail tile carries the whole loss
        active[rows] = 0.0
        active[rows[-1]] = 1.0
    elif active[rows].sum() == 0:
        active[rows[-1]] = 1.0
    ret = (rng.standard_normal(n_rows) * 3).astype(f)
    ret[rng.random(n_rows) > 0.9] *= 20
    noise = (rng.standard_normal(n_rows) * 0.25).astype(f)
    vn = O.ValueNormRef()
    vn.update(ret[:50].reshape(-1, 1)); vn.update(ret[rows].reshape(-1, 1))
    for _ in range(20):
        with torch.no_grad():
            v_now = critic(torch.from_numpy(sobs), None, None)[0].numpy().reshape(-1)
        v_old = (v_now + noise).astype(f)
        if not safe:
            break
        bad = np.flatnonzero(_margin(a, actor, critic, heads, relu, obs, sobs, actions, avail, active, old_logp, v_old, ret, vn) < 1e-4)
        if bad.size == 0:
            break
        obs[bad] = rng.standard_normal((bad.size, D))
        sobs[bad] = rng.standard_normal((bad.size, S))
        old_logp[bad] = draw_old(bad.size)
        noise[bad] = rng.standard_normal(bad.size) * 0.25
    else:
        raise AssertionError("could not draw inputs away from the kinks")
    assert active[rows].sum() >= 1
    return dict(obs=obs, sobs=sobs, avail=avail, actions=actions, old=old_logp, adv=adv, active=active, ret=ret, vold=v_old), vn


def _stat_bounds(c):
    """The bound of each of (value_loss, policy_loss, dist_entropy, ratio) against the float64 reference."""
    return [2e-6 * abs(r) + 1e-8 if c.heads else 1e-5 * abs(r) + 1e-7 for r in c.ref[0]]


def _stats32(c):
    """The four statistics from the oracle networks evaluated in float32 on the CPU: the reference's own error in the kernels'
    number format."""
    x, r = c.x, c.rows.astype(np.int64)
    t = lambda v: torch.from_numpy(v[r])
    with torch.no_grad():
        act, adv = t(x["active"]).view(-1, 1), t(x["adv"]).view(-1, 1)
        vals = c.critic(t(x["sobs"]), None, None)[0]
        ret_t = t(x["ret"]).view(-1, 1)
        tgt = c.vn.normalize(ret_t) if c.a.use_valuenorm else ret_t
        if c.heads is None:
            lp, ent, _ = c.actor.evaluate_actions(t(x["obs"]), None, t(x["actions"]).view(-1, 1), None,
                                                  None if x["avail"] is None else t(x["avail"]), act)
            pl, vl, imp = O.ppo_losses_ref(c.a, lp, ent, vals, t(x["old"]).view(-1, 1), adv, act, t(x["vold"]).view(-1, 1), tgt)
            return [vl.item(), pl.item(), ent.item(), imp.mean().item()]
        z = c.actor.act.logits(c.actor.features(t(x["obs"]), None, None)[0], None)
        pl, ent, ratio, _ = md_ref.policy_terms(z, c.heads, t(x["actions"]), t(x["old"]), adv, act, c.a.clip_param, c.a.use_policy_active_masks)
        dummy = torch.zeros_like(ret_t)
        _, vl, _ = O.ppo_losses_ref(c.a, dummy, dummy.sum(), vals, dummy, adv, act, t(x["vold"]).view(-1, 1), tgt)
        return [vl.item(), pl.item(), ent.item(), ratio.item()]


def cpu_case(name, B, with_rows, **kw):
    """_cpu_case with the first seed in 0..9 at which the oracle ALONE meets the case's conditions: besides the kink margins and
    the active row of _draw, the float32 evaluation of the oracle (_stats32) is within the statistics' bounds of its float64
    evaluation.  Where it is not, a statistic is a cancelling sum (a policy loss of signed terms of magnitude 1 that sum to 1e-2)
    that no float32 implementation meets at a relative bound; the draw then says nothing about the kernels.  Nothing a kernel
    returns enters the choice."""
    for seed in range(10):
        c = _cpu_case(name, B, with_rows, seed=seed, **kw)
        if c.ref is None or all(abs(s - r) <= b for s, r, b in zip(_stats32(c), c.ref[0], _stat_bounds(c))):
            c.seed = seed
            return c
    raise AssertionError("no seed at which the float32 oracle meets the statistics' bounds")


def _cpu_case(name, B, with_rows, pattern=None, with_avail=True, flags="default", safe=True, seed=0):
    """Networks, inputs and the float64 reference of one case (`name`: a key of ALL_NETS, or a network tuple); needs no GPU."""
    D, S, A, LN, relu, fn = ALL_NETS[name] if isinstance(name, str) else name
    name = name if isinstance(name, str) else "x".join(map(str, name[:4]))
    heads = A if isinstance(A, tuple) else None
    A = sum(heads) if heads else A
    torch.manual_seed(B + D + S)
    rng = np.random.default_rng([B, D, A, int(with_rows), seed, {None: 0, "tile_off": 1, "last_only": 2}[pattern], int(with_avail)])
    a = O.default_args(use_ReLU=relu, layer_N=LN, use_feature_normalization=fn, **FLAGS[flags])
    actor, critic = O.ActorRef(a, D, A), O.CriticRef(a, S)
    _randomize(actor, D + 3); _randomize(critic, S + 4)
    n_rows = B + 64 if with_rows else B
    rows = rng.permutation(n_rows)[:B].astype(np.int32) if with_rows else np.arange(B, dtype=np.int32)
    x, vn = _draw(a, actor, critic, rng, n_rows, rows, D, S, A, heads, relu, pattern, with_avail, safe)
    c = types.SimpleNamespace(name=name, D=D, S=S, A=A, LN=LN, relu=relu, fn=fn, heads=heads, B=B, a=a, actor=actor, critic=critic,
                              rows=rows, with_rows=with_rows, x=x, vn=vn, ref=None)
    if safe:
        r64 = rows.astype(np.int64)
        if heads is None:
            c.ref = _reference(a, actor, critic, r64, x["obs"], x["sobs"], x["avail"], x["actions"], x["old"], x["adv"], x["active"],
                               x["vold"], x["ret"], vn)[:3]
        else:
            c.ref = _md_reference(a, actor, critic, heads, r64, x["obs"], x["sobs"], x["actions"], x["old"], x["adv"], x["active"],
                                  x["vold"], x["ret"], vn)
        assert all(np.isfinite(v) for v in c.ref[0])
    return c


@pytest.fixture(scope="module")
def ops(gpu_device):
    from mappo_amd import ops as _ops
    return _ops


def gpu_case(ops, *args, **kw):
    c = cpu_case(*args, **kw)
    c.ops = ops
    c.da, c.dc = ops.net_desc(c.D, c.A, c.LN, c.relu, c.fn), ops.net_desc(c.S, 1, c.LN, c.relu, c.fn)
    c.pa, c.la, c.Pa = _flat_from_module(ops, c.actor, c.da, "act.action_out.linear")
    c.pc, c.lc, c.Pc = _flat_from_module(ops, c.critic, c.dc, "v_out")
    c.d_rows = dev(c.rows, torch.int32) if c.with_rows else None
    c.g = {k: (None if v is None else dev(v)) for k, v in c.x.items()}
    c.g["vn"] = dev(c.vn.state()) if c.a.use_valuenorm else None
    c.mom = torch.zeros(4, dtype=torch.float64, device="cuda")
    ops.minibatch_moments(c.g["ret"], c.g["active"], c.d_rows, c.B, c.mom)
    c.cfg = ops.ppo_cfg(c.a)
    c.col_c = ((c.Pa + 255) // 256) * 256
    c.P = c.col_c + ((c.Pc + 255) // 256) * 256 + 256            # a spare 256 columns after the critic's range: must stay untouched
    c.ranges = [(0, c.Pa), (c.col_c, c.Pc)]
    c.ns = ops.mlp_backward_slabs(c.B)
    c.dual = c.D <= 64 and c.S <= 64
    if c.dual:
        c.nd = ops.dual_update_slabs(c.da, c.dc, c.B)
        assert c.nd == dual_slabs(c.D, c.S, c.A, c.LN, c.B)      # the Python mirror of the dispatch agrees with the library
    return c


def _partials(ops, fill):
    return torch.full((ops.update_partials("cuda").numel(),), fill, dtype=torch.float64, device="cuda")


def _buffers(c, n, fill):
    slabs = torch.full((n + 3, c.P), fill, device="cuda")
    for d, (c0, Pn) in zip((c.D, c.S), c.ranges):
        if d > 64:
            slabs[:n, c0:c0 + Pn] = 0.0          # wide inputs: the caller zeroes its column range (mappo_wide_l1_backward writes fewer rows)
    return slabs, _partials(c.ops, fill), _partials(c.ops, fill)


def launch(c, form, fill=0.0, cfg=None, avail="own", obs=None, sobs=None, n_blocks=0, bufs=None):
    """One fused update, `form` "single" (actor_update + critic_update) or "dual": (slabs, actor partials, critic partials, rows)."""
    ops, g, B = c.ops, c.g, c.B
    cfg = cfg or c.cfg
    obs, sobs = g["obs"] if obs is None else obs, g["sobs"] if sobs is None else sobs
    av = g["avail"] if isinstance(avail, str) else avail
    n_full = c.ns if form == "single" else c.nd
    slabs, p_a, p_c = bufs or _buffers(c, n_full, fill)
    if form == "single":
        n = min(n_blocks, n_full) if n_blocks > 0 else n_full
        if c.heads is None:
            ops.actor_update(c.pa, c.da, obs, c.d_rows, B, av, g["actions"], g["old"], g["adv"], g["active"], c.mom, cfg, slabs, c.P, 0, p_a, n_blocks)
        else:
            ops.actor_update_md(c.pa, c.da, obs, c.d_rows, B, c.heads, g["actions"], g["old"], g["adv"], g["active"], c.mom, cfg, slabs, c.P, 0,
                                p_a, n_blocks)
        ops.critic_update(c.pc, c.dc, sobs, c.d_rows, B, g["vold"], g["ret"], g["active"], g["vn"], c.mom, cfg, slabs, c.P, c.col_c, p_c, n_blocks)
    else:
        n = n_full
        if c.heads is None:
            ops.actor_critic_update(c.pa, c.da, obs, c.pc, c.dc, sobs, c.d_rows, B, av, g["actions"], g["old"], g["adv"], g["active"], g["vold"],
                                    g["ret"], g["vn"], c.mom, cfg, slabs, c.P, 0, c.col_c, p_a, p_c)
        else:
            ops.actor_critic_update_md(c.pa, c.da, obs, c.pc, c.dc, sobs, c.d_rows, B, c.heads, g["actions"], g["old"], g["adv"], g["active"],
                                       g["vold"], g["ret"], g["vn"], c.mom, cfg, slabs, c.P, 0, c.col_c, p_a, p_c)
    return slabs, p_a, p_c, n


def reduce(c, out):
    """(the six statistics, the reduced gradient) of a launch."""
    slabs, p_a, p_c, n = out
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    c.ops.update_stats(p_a, n, p_c, n, c.mom, c.cfg, stats)
    grad = torch.zeros(c.P, device="cuda")
    c.ops.slab_reduce(slabs, n, c.P, c.P, grad)
    return stats.cpu().numpy(), grad.cpu().numpy()


def unfused(c, avail="own"):
    """mlp_forward -> ppo_loss_fwd_bwd -> mlp_backward (Discrete)."""
    ops, g, B = c.ops, c.g, c.B
    av = g["avail"] if isinstance(avail, str) else avail
    logits, values = torch.zeros(B, c.A, device="cuda"), torch.zeros(B, device="cuda")
    ops.mlp_forward(c.pa, c.da, g["obs"], c.d_rows, B, logits)
    ops.mlp_forward(c.pc, c.dc, g["sobs"], c.d_rows, B, values)
    dl, dv = torch.zeros(B, c.A, device="cuda"), torch.zeros(B, device="cuda")
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    ops.ppo_loss_fwd_bwd(logits, values, c.d_rows, av, g["actions"], g["old"], g["adv"], g["active"], g["vold"], g["ret"], g["vn"], c.mom, dl, dv,
                         stats, c.cfg)
    slabs = torch.zeros(c.ns, c.P, device="cuda")
    ops.mlp_backward(c.pa, c.da, g["obs"], c.d_rows, B, dl, slabs, c.P, 0)
    ops.mlp_backward(c.pc, c.dc, g["sobs"], c.d_rows, B, dv.view(B, 1), slabs, c.P, c.col_c)
    grad = torch.zeros(c.P, device="cuda")
    ops.slab_reduce(slabs, c.ns, c.P, c.P, grad)
    return stats.cpu().numpy(), grad.cpu().numpy()


WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


def vs_reference(c, stats, grad, what):
    """Statistics and every parameter gradient against float64 autograd; the ratios go to WORST (printed by each test)."""
    ref_stats, ga, gc = c.ref
    fam = c.name.split("-")[0] + " " + what.split(",")[0]
    for i, name in enumerate(("value_loss", "policy_loss", "dist_entropy", "ratio")):
        bound = _stat_bounds(c)[i]
        _note((fam, "stat"), abs(stats[i] - ref_stats[i]) / bound)
        assert abs(stats[i] - ref_stats[i]) <= bound, f"{c.name} B={c.B} {what}: {name} {stats[i]!r} vs {ref_stats[i]!r}"
    for layout, col0, ref, net in ((c.la, 0, ga, "actor"), (c.lc, c.col_c, gc, "critic")):
        for key, off, shape in layout:
            got = grad[col0 + off: col0 + off + int(np.prod(shape))].reshape(shape)
            if not np.abs(ref[key]).max():
                assert not np.abs(got).max(), f"{c.name} B={c.B} {what}: {net} {key} is exactly zero in float64"
            else:
                _note((fam, "grad"), np.abs(got - ref[key]).max() / np.abs(ref[key]).max())
    _check_grads(grad, c.la, c.lc, c.col_c, ga, gc, f"{c.name} B={c.B} {what}")


def _print_worst():
    for (fam, kind), v in sorted(WORST.items()):
        print(f"WORST {fam:24s} {kind}: {v:.3e}")


def run_forms(c, nan=True, avail="own"):
    """The launch forms of one case against the reference; `nan`: again on NaN-filled buffers, with the write contract."""
    res = {}
    forms = ["single"] + (["dual"] if c.dual else [])
    for form in forms:
        out = launch(c, form, 0.0, avail=avail)
        st, gr = reduce(c, out)
        vs_reference(c, st, gr, form)
        res[form] = (out, st, gr)
        if nan:
            outn = launch(c, form, NAN, avail=avail)
            n = outn[3]
            _check_written(outn[0].cpu().numpy(), n, c.ranges, f"{c.name} B={c.B} {form}")
            _check_partials(outn[1], n, f"{form}, actor"); _check_partials(outn[2], n, f"{form}, critic")
            stn, grn = reduce(c, outn)
            close(stn, st, 0, 0, f"{form} stats: NaN-filled vs zero-filled buffers")
            for c0, Pn in c.ranges:
                close_rel_max(grn[c0:c0 + Pn], gr[c0:c0 + Pn], 1e-6, f"{form} grad: NaN-filled vs zero-filled slabs")
    if c.dual:
        close(res["dual"][1], res["single"][1], 1e-6, 1e-9, "stats dual vs separate launches")
        close_rel_max(res["dual"][2], res["single"][2], 2e-6, "grad dual vs separate launches")
    if c.heads is None:
        st, gr = unfused(c, avail)
        assert np.array_equal(res["single"][1][4:], st[4:])
        vs_reference(c, st, gr, "unfused")
        res["unfused"] = (None, st, gr)
    return res


# ---- 1. edge batch sizes ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_rows", [False, True], ids=["flat", "rows"])
@pytest.mark.parametrize("B", EDGE_B)
@pytest.mark.parametrize("name", list(ALL_NETS))
def test_edge_batches(ops, name, B, with_rows):
    run_forms(gpu_case(ops, name, B, with_rows))
    _print_worst()


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["tile_off", "last_only"])
@pytest.mark.parametrize("B", [33, 17])
@pytest.mark.parametrize("name", list(ALL_NETS))
def test_active_patterns(ops, name, B, pattern):
    """Policy and value masks on (the default flags): minibatch rows 16..31 inactive (B = 33: a full 16-row tile and half of the
    32-row one; B = 17: the tail tile), or only the last row active (the 1-row tail tile carries the whole loss)."""
    c = gpu_case(ops, name, B, B == 17, pattern=pattern)
    assert c.a.use_policy_active_masks and c.a.use_value_active_masks
    act = c.x["active"][c.rows]
    assert (act.sum() == 1 and act[-1] == 1) if pattern == "last_only" else (act[16:32].sum() == 0 and act.sum() == B - len(act[16:32]))
    run_forms(c)
    _print_worst()


# ---- 2. avail == NULL ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [53, 16])
@pytest.mark.parametrize("name", list(NETS))
def test_avail_none(ops, name, B):
    """What every MPE run passes.  Each launch form against float64 autograd without available_actions, and bit-identical to the
    same form given an all-ones avail (unfused: equal statistics and gradient)."""
    c = gpu_case(ops, name, B, False, with_avail=False)
    assert c.g["avail"] is None
    r0 = run_forms(c, nan=False, avail=None)
    ones = torch.ones(B, c.A, device="cuda")
    for form, (out, st, gr) in r0.items():
        if form == "unfused":
            st1, gr1 = unfused(c, ones)
        else:
            out1 = launch(c, form, 0.0, avail=ones)
            assert torch.equal(out[0], out1[0]) and torch.equal(out[1], out1[1]) and torch.equal(out[2], out1[2]), f"{form}: slabs / partials"
            st1, gr1 = reduce(c, out1)
        assert np.array_equal(st, st1) and np.array_equal(gr, gr1), f"{form}: NULL vs all-ones avail"
    _print_worst()


# ---- 3. x that is only 4-byte aligned ----------------------------------------------------------------------------------------
def _shifted(x, off):
    """A contiguous copy of x that starts `off` floats into its allocation."""
    big = torch.empty(x.numel() + 8, device="cuda")
    v = big[off: off + x.numel()].view(x.shape)
    v.copy_(x)
    assert big.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("B", [48, 53])
@pytest.mark.parametrize("name", list(ALL_NETS))
def test_misaligned_x(ops, name, B):
    """rows None and an x whose every row is 4-byte aligned only: prefetch16 / prefetch_half gather their full tiles, too.
    Every family, single and dual, turned out bit-identical to the aligned launch (the flat loads hand each lane the values it
    would have gathered, and the wide kernels have one load path): that is asserted, on top of the two bounds."""
    c = gpu_case(ops, name, B, False)
    assert c.g["obs"].data_ptr() % 16 == 0 and c.g["sobs"].data_ptr() % 16 == 0
    for form in ["single"] + (["dual"] if c.dual else []):
        out = launch(c, form)
        st, gr = reduce(c, out)
        same = True
        for off in (1, 2, 3):
            obs, sobs = _shifted(c.g["obs"], off), _shifted(c.g["sobs"], off)
            assert obs.data_ptr() % 16 != 0 and sobs.data_ptr() % 16 != 0
            outm = launch(c, form, obs=obs, sobs=sobs)
            stm, grm = reduce(c, outm)
            vs_reference(c, stm, grm, f"{form}, x + {off} floats")
            close_rel_max(grm, gr, 2e-6, f"{c.name} {form}: x + {off} floats vs aligned, gradient")
            close(stm, st, 1e-6, 1e-9, f"{c.name} {form}: x + {off} floats vs aligned, statistics")
            same = same and all(torch.equal(u, v) for u, v in zip(outm[:3], out[:3]))
        assert same, f"{name} {form}: the misaligned launch is not bit-identical to the aligned one"
    _print_worst()


# ---- 4. accumulating partials --------------------------------------------------------------------------------------------------
def _p0(ops):
    n = ops.update_partials("cuda").numel() // 4
    r, k = np.meshgrid(np.arange(n), np.arange(4), indexing="ij")
    return torch.as_tensor(0.37 * (4 * r + k + 1) - 3.0, dtype=torch.float64).reshape(-1).cuda()


def _acc_close(got, p0, fresh, k, what):
    """got == p0 + k fresh within 1e-12 (|p0| + |fresh|) per element: fewer than 40 double additions of 2^-53 each per entry."""
    got, p0, fresh = (t.cpu().numpy() for t in (got, p0, fresh))
    err, tol = np.abs(got - (p0 + k * fresh)), 1e-12 * (np.abs(p0) + np.abs(fresh))
    assert (err <= tol).all(), f"{what}: off by {(err / tol).max():.3g} of the bound"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ALL_NETS))
def test_accumulate_partials(ops, name):
    """cfg.accumulate_partials (every PPO epoch but the last): the launch's partial rows become p0 + fresh, the rows beyond keep p0,
    slabs are those of the fresh launch; a second accumulating launch gives p0 + 2 fresh."""
    B = 53
    c = gpu_case(ops, name, B, True)
    acc = ops.ppo_cfg(c.a, accumulate_partials=True)
    assert acc.accumulate_partials == 1 and c.cfg.accumulate_partials == 0
    p0 = _p0(ops)
    assert torch.isfinite(p0).all() and len(set(p0.cpu().numpy().tolist())) == p0.numel() and (p0 != 0).all()
    for form in ["single"] + (["dual"] if c.dual else []):
        fresh = launch(c, form)
        st, gr = reduce(c, fresh)
        vs_reference(c, st, gr, form)
        n = fresh[3]
        bufs = _buffers(c, n, 0.0)
        bufs[1].copy_(p0); bufs[2].copy_(p0)
        for k in (1, 2):
            out = launch(c, form, cfg=acc, bufs=bufs)
            assert torch.equal(out[0], fresh[0]), f"{form}: slabs with accumulate_partials"
            for i, net in ((1, "actor"), (2, "critic")):
                _acc_close(out[i][:4 * n], p0[:4 * n], fresh[i][:4 * n], k, f"{name} {form} {net} launch {k}")
                assert torch.equal(out[i][4 * n:], p0[4 * n:]), f"{form} {net}: partial rows beyond the launch's changed"
        assert (fresh[1][:4 * n].view(-1, 4)[:, :3] != 0).any() and (fresh[2][:4 * n].view(-1, 4)[:, 0] != 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name,net,B", [("nA<nC", (18, 54, 5, 1, True, True), 16500), ("nA>nC", (60, 5, 16, 0, False, True), 12000)])
def test_accumulate_partials_unequal_dual_shares(ops, name, net, B):
    """The dual 16-sample-tile launch with unequal shares (MATRIX's shapes): the narrower network's rows [min(nA, nC), max(nA, nC)) are
    written by the other network's workgroups — slab columns 0 in both modes, partials 0 without the flag, untouched with it."""
    D, S, A, LN = net[:4]
    nA, nC = upd16_split(D, S, A, LN, B)
    assert dual_family(D, S, A, LN) == "upd16d" and ((nA < nC) if name == "nA<nC" else (nA > nC))
    c = gpu_case(ops, net, B, True, safe=False)          # no reference here: plain random inputs
    lo, hi = min(nA, nC), max(nA, nC)
    assert c.nd == hi
    narrow = 1 if nA < nC else 2                         # index into (slabs, actor partials, critic partials)
    c0, Pn = c.ranges[narrow - 1]
    acc = ops.ppo_cfg(c.a, accumulate_partials=True)
    p0 = _p0(ops)
    fresh = launch(c, "dual", NAN)
    _check_written(fresh[0].cpu().numpy(), hi, c.ranges, f"dual {name}")
    assert not fresh[0][lo:hi, c0:c0 + Pn].abs().max().item() and fresh[0][:lo, c0:c0 + Pn].abs().max().item() > 0
    assert not fresh[narrow][4 * lo: 4 * hi].abs().max().item(), "flag off: the rows the narrower network does not own become 0"
    _check_partials(fresh[1], hi, "actor"); _check_partials(fresh[2], hi, "critic")
    bufs = (torch.full((hi + 3, c.P), NAN, device="cuda"), p0.clone(), p0.clone())
    out = launch(c, "dual", cfg=acc, bufs=bufs)
    assert torch.equal(out[0][:hi].nan_to_num(7.0), fresh[0][:hi].nan_to_num(7.0)) and not out[0][lo:hi, c0:c0 + Pn].abs().max().item()
    assert torch.equal(out[narrow][4 * lo:], p0[4 * lo:]), "flag on: the rows the narrower network does not own keep p0"
    wide = 3 - narrow
    _acc_close(out[narrow][:4 * lo], p0[:4 * lo], fresh[narrow][:4 * lo], 1, f"{name}: narrower network")
    _acc_close(out[wide][:4 * hi], p0[:4 * hi], fresh[wide][:4 * hi], 1, f"{name}: the other network")
    assert torch.equal(out[wide][4 * hi:], p0[4 * hi:])


# ---- 5. caller-chosen grid -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["upd16", "upd2-tanh"])
def test_caller_chosen_grid(ops, name):
    """n_blocks (the grid of --concurrent_update): exactly min(n_blocks, slabs(B)) slab and partial rows are written; the result
    matches float64 autograd and the default grid; more workgroups than CUs is MAPPO_EINVAL before any launch."""
    from mappo_amd import _lib
    B = 333
    c = gpu_case(ops, name, B, True)
    ns = c.ns
    assert ns == 11
    st0, gr0 = reduce(c, launch(c, "single"))
    vs_reference(c, st0, gr0, "single")
    for nb in (1, 3, ns, ns + 5):
        out = launch(c, "single", NAN, n_blocks=nb)
        n = out[3]
        assert n == min(nb, ns)
        _check_written(out[0].cpu().numpy(), n, c.ranges, f"{name} n_blocks={nb}")
        _check_partials(out[1], n, f"actor_update n_blocks={nb}"); _check_partials(out[2], n, f"critic_update n_blocks={nb}")
        st, gr = reduce(c, out)
        vs_reference(c, st, gr, f"single, n_blocks={nb}")
        close(st, st0, 1e-6, 1e-9, f"{name} n_blocks={nb} vs the default grid, statistics")
        for c0, Pn in c.ranges:
            close_rel_max(gr[c0:c0 + Pn], gr0[c0:c0 + Pn], 2e-6, f"{name} n_blocks={nb} vs the default grid, gradient")
    slabs, p_a, p_c = _buffers(c, ns, NAN)
    for who in ("actor_update", "critic_update"):
        with pytest.raises(_lib.MappoHipError, match=r"code -1.*n_blocks 257 > 256"):
            if who == "actor_update":
                ops.actor_update(c.pa, c.da, c.g["obs"], c.d_rows, B, c.g["avail"], c.g["actions"], c.g["old"], c.g["adv"], c.g["active"], c.mom,
                                 c.cfg, slabs, c.P, 0, p_a, 257)
            else:
                ops.critic_update(c.pc, c.dc, c.g["sobs"], c.d_rows, B, c.g["vold"], c.g["ret"], c.g["active"], c.g["vn"], c.mom, c.cfg, slabs,
                                  c.P, c.col_c, p_c, 257)
        msg = _lib.load().mappo_last_error()
        assert who.encode() in msg and b"n_blocks 257" in msg
    torch.cuda.synchronize()
    assert torch.isnan(slabs).all() and torch.isnan(p_a).all() and torch.isnan(p_c).all(), "a rejected call launched something"
    _print_worst()
