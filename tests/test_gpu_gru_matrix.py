"""Every path of the recurrent PPO update chain against float64 autograd.

One update of a recurrent network (mappo_amd/recurrent.py: _update_recurrent.one_net) is
    mappo_mlp_features_seq | mappo_mlp_features -> mappo_gru16_forward_loss -> mappo_gru16_backward -> mappo_gru16_wgrad
    -> mappo_trunk_backward_seq | mappo_trunk_backward
and the host dispatch (csrc/gru_train16.hip: seq_waves, seq_split, *_grid, mappo_mlp_features_seq) chooses among

    forward   split recurrence (gru16s_fwd_kernel + gru16_head_kernel<HEAD, NBH>) | unsplit gru16_fwd_kernel<HEAD, NBH, XBLK>
    backward  gru16s_bwd_kernel<DXBLK> | gru16_bwd4_kernel<DXBLK> (<= 4 waves) | gru16_bwd_kernel<DXBLK>
    wgrad     gru16_wgrad_kernel<XBLK>
    features  gru16_features_kernel<RELU, LN, KB1> with 1 / 4 / 8 waves | the wide blocked forward | feature-major mappo_mlp_features

MATRIX is a covering design of those instances; test_gru_matrix_covers_every_instance checks that on the CPU through a Python
mirror of the dispatch, environment overrides included (the host functions read them on every launch, so monkeypatch.setenv
selects a path in-process).  Each case calls the ops wrappers as one_net does, for an actor and a critic, and compares the four
loss statistics, every parameter's gradient and the trunk features with float64 autograd through the oracle networks
(O.ActorRef / O.CriticRef with use_recurrent_policy, O.ppo_losses_ref).  Cases marked `nan` fill slabs, partials, scratch and
feature arrays with NaN and check the write contract stated in include/mappo_hip.h.

test_recurrent_update_shape_change_on_one_trainer: one trainer, two minibatch shapes in a row (the kernels' grids shrink)."""
import copy
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import mappo_oracle as O
from test_gpu_e2e import M, make_args, set_vn   # noqa: F401  (M: the trainer-level fixture)
from test_gpu_kernels import close, close_rel_max, dev, _flat_from_module, _randomize, _relu_margin
from test_gpu_update_matrix import FLAGS

# ---- Python mirror of the dispatch (mappo_amd/csrc/gru_train16.hip, host section) ---------------------------------------
NUM_CU, G16_WAVES, HID = 256, 8, 64


def _tiles(Nc):
    return (Nc + 15) // 16


def seq_waves(Nc, env):
    n_ct = _tiles(Nc)
    w = (n_ct + NUM_CU - 1) // NUM_CU
    w = min(n_ct, 4) if w < 4 else w
    if "MAPPO_GRU16_WAVES" in env:
        w = int(env["MAPPO_GRU16_WAVES"])
    return max(1, min(w, G16_WAVES))


def seq_split(Nc, bwd, env):
    thr = int(env.get("MAPPO_GRU16_SPLIT_TILES_BWD" if bwd else "MAPPO_GRU16_SPLIT_TILES", 1024))
    return _tiles(Nc) <= thr


def split_grid(Nc, env):
    return min(_tiles(Nc), int(env.get("MAPPO_GRU16_SPLIT_GRID", 2 * NUM_CU)))


def head_grid(L, Nc):
    return min((L * _tiles(Nc) + 3) // 4, NUM_CU)


def seq_grid(Nc, env):
    nw = seq_waves(Nc, env)
    return min((_tiles(Nc) + nw - 1) // nw, NUM_CU)


def wg_grid(L, Nc):
    return min((L * _tiles(Nc) + 1) // 2, NUM_CU)


def gru16_slabs(L, Nc, env):
    """mappo_gru16_slabs."""
    return max(seq_grid(Nc, env), wg_grid(L, Nc))


def forward_grid(L, Nc, env):
    """Workgroups that write loss partials (and the head / rnn.norm slab columns)."""
    return head_grid(L, Nc) if seq_split(Nc, False, env) else seq_grid(Nc, env)


def mlp_backward_slabs(B):
    return min((B + 31) // 32, NUM_CU)


def feature_path(D, LN, Nc):
    """The trunk-feature form one_net chooses: 'narrow' / 'wide' (blocked, mappo_mlp_features_seq) or 'fm' (feature-major)."""
    if LN <= 1 and 4 <= D <= 64:
        return "narrow"
    if LN <= 1 and 64 < D <= 512 and Nc % 16 == 0:
        return "wide"
    return "fm"


def fm_reason(D, LN, Nc):
    return "layer_N" if LN > 1 else ("D<4" if D < 4 else ("wide_ragged" if D > 64 and Nc % 16 else None))


def feat16_launch(L, Nc, env):
    """(waves, workgroups, tiles) of gru16_features_kernel."""
    n_tiles = L * _tiles(Nc)
    nw = 8 if n_tiles >= 8 * NUM_CU else (4 if n_tiles >= 4 else 1)
    return nw, min((n_tiles + nw - 1) // nw, int(env.get("MAPPO_FEAT16_GRID", NUM_CU))), n_tiles


# ---- the matrix ------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "D S A LN relu fn L Nc rows flags env nan fm")
U = {"MAPPO_GRU16_SPLIT_TILES": "0", "MAPPO_GRU16_SPLIT_TILES_BWD": "0"}         # unsplit forward and backward
U8 = dict(U, MAPPO_GRU16_WAVES="8")                                                 # ... with 8 waves (production: n_ct > 1024)
T, F = True, False

# actor in_dim D, critic in_dim S, actions A, layer_N, ReLU, feature norm, L, Nc, gathered rows / h0_rows (else NULL), flag set,
# path overrides, NaN fill, feature-major forced where the blocked form would be chosen
MATRIX = [
    # split recurrence (default up to 1 024 tiles): every gru16_features_kernel<RELU, LN, KB1>, both head widths, every flag set
    Case(4, 20, 2, 1, T, T, 3, 17, T, "default", {}, T, F),                    # KB1 1, 2; one full and one 1-sequence tile
    Case(40, 64, 9, 1, T, F, 10, 37, T, "huber_off", {}, F, F),                # KB1 3, 4; feature norm off, layer_N 1
    Case(12, 30, 16, 0, T, T, 1, 16, F, "vclip_off", {}, F, F),                # L = 1, Nc = 16: one tile, 1-wave features kernel
    Case(33, 50, 17, 0, T, F, 10, 70, T, "pmask_off", {}, T, F),               # head wider than 16; feature norm off, layer_N 0
    Case(16, 17, 5, 1, F, T, 3, 1, T, "vmask_off", {}, F, F),                  # Nc = 1
    Case(48, 49, 32, 1, F, T, 10, 133, F, "vn_off", {}, F, F),
    Case(5, 32, 9, 0, F, T, 3, 37, T, "hyper", {}, F, F),
    Case(36, 60, 5, 0, F, T, 10, 17, T, "default", {"MAPPO_GRU16_SPLIT_GRID": "1", "MAPPO_FEAT16_GRID": "2"}, F, F),   # tile loops
    # ... feature-major x / d x: layer_N 2, in_dim < 4, wide with a ragged tile; wide blocked with a head wider than 16
    Case(20, 44, 5, 2, T, T, 10, 37, T, "default", {}, T, F),
    Case(3, 2, 20, 1, F, T, 3, 70, T, "huber_off", {}, F, F),
    Case(130, 322, 17, 1, T, T, 3, 32, T, "vclip_off", {}, T, F),
    Case(130, 70, 9, 0, T, T, 3, 37, F, "pmask_off", {}, F, F),
    Case(18, 54, 5, 1, T, T, 2, 9607, T, "default", {}, F, F),                 # steady state: 601 tiles > 512 workgroups
    # unsplit kernels with <= 4 waves (gru16_bwd4_kernel) ...
    Case(18, 54, 9, 1, T, T, 10, 37, T, "default", U, T, F),
    Case(20, 12, 32, 1, T, T, 3, 70, T, "huber_off", U, F, F),                 # NBH = 2
    Case(30, 48, 5, 2, F, T, 10, 37, F, "vclip_off", U, T, F),                 # XBLK = DXBLK = false
    Case(2, 3, 17, 0, T, T, 3, 17, T, "pmask_off", U, F, F),                   # ... with NBH = 2
    Case(25, 40, 10, 1, F, T, 1, 133, F, "hyper", U, F, F),                    # L = 1
    Case(9, 7, 3, 1, T, T, 3, 1, F, "default", U, F, F),                       # Nc = 1
    Case(130, 66, 5, 1, T, T, 3, 32, T, "default", U, F, F),                   # wide blocked
    # ... and with 8 (gru16_bwd_kernel); n_ct = 9 >= waves
    Case(44, 16, 16, 0, F, F, 10, 133, T, "vmask_off", U8, T, F),
    Case(64, 8, 2, 1, T, T, 10, 133, T, "vn_off", U8, T, T),
    Case(54, 18, 5, 1, T, T, 2, 33005, T, "default", {}, F, F),                # steady state: unsplit by default, 2 063 tiles > 256 x 8
]
IDS = [f"{i:02d}-D{c.D}-S{c.S}-A{c.A}-LN{c.LN}-{'relu' if c.relu else 'tanh'}-L{c.L}-Nc{c.Nc}-{c.flags}"
       f"{'-unsplit' if c.env.get('MAPPO_GRU16_SPLIT_TILES') == '0' else ''}{'-nan' if c.nan else ''}" for i, c in enumerate(MATRIX)]


def _net_instances(c, actor):
    """What one network of a case launches, by the mirror."""
    d = c.D if actor else c.S
    path = feature_path(d, c.LN, c.Nc)
    blocked = path != "fm" and not c.fm
    head = ("a<=16" if c.A <= 16 else "a>16") if actor else "critic"
    sf, sb = seq_split(c.Nc, False, c.env), seq_split(c.Nc, True, c.env)
    bwd = "split" if sb else ("bwd4" if seq_waves(c.Nc, c.env) <= 4 else "bwd")
    inst = dict(fwd=("split" if sf else "unsplit", head, blocked), bwd=(bwd, blocked), wgrad=blocked, feat=None, fm=None,
                split=sf)
    if blocked and path == "narrow":
        inst["feat"] = (c.relu, c.LN, (d + 15) // 16)
    elif blocked:
        inst["feat"] = "wide"
    else:
        inst["fm"] = fm_reason(d, c.LN, c.Nc) or "forced"
    return inst


def test_gru_matrix_covers_every_instance():
    """The case list reaches every forward / backward / wgrad / features instance, the three reasons for feature-major features,
    every flag set on the split and the unsplit kernels for both heads, every looping grid and the listed edges."""
    fwd, bwd, wgrad, feat, feat_waves, nofn, fmr, flags = set(), set(), set(), set(), set(), set(), set(), set()
    for c in MATRIX:
        B = c.L * c.Nc
        assert gru16_slabs(c.L, c.Nc, c.env) >= max(mlp_backward_slabs(B), head_grid(c.L, c.Nc), forward_grid(c.L, c.Nc, c.env))
        if "MAPPO_GRU16_WAVES" in c.env:
            assert _tiles(c.Nc) >= int(c.env["MAPPO_GRU16_WAVES"])              # the geometry production has
        assert seq_split(c.Nc, False, c.env) == seq_split(c.Nc, True, c.env)    # as in production: one threshold
        for actor in (True, False):
            i = _net_instances(c, actor)
            fwd.add(i["fwd"]); bwd.add(i["bwd"]); wgrad.add(i["wgrad"])
            flags.add((c.flags, i["split"]))                                # (every case runs both heads)
            if i["feat"] == "wide":
                feat.add("wide")
            elif i["feat"]:
                feat.add(i["feat"]); feat_waves.add(feat16_launch(c.L, c.Nc, c.env)[0])
                if not c.fn:
                    nofn.add(c.LN)
            else:
                fmr.add(i["fm"])
    assert fwd == {(s, h, b) for s in ("split", "unsplit") for h in ("a<=16", "a>16", "critic") for b in (T, F)}, fwd
    assert bwd == {(k, b) for k in ("split", "bwd4", "bwd") for b in (T, F)}, bwd
    assert wgrad == {T, F}
    assert feat == {(r, ln, kb) for r in (T, F) for ln in (0, 1) for kb in (1, 2, 3, 4)} | {"wide"}, feat
    assert feat_waves >= {1, 4} and nofn == {0, 1}
    assert fmr >= {"layer_N", "D<4", "wide_ragged"}, fmr
    assert flags >= {(f, s) for f in FLAGS for s in (T, F)}, flags
    # looping grids: split recurrence, unsplit sequence kernels, head, wgrad, features (by size and by override)
    assert any(seq_split(c.Nc, F, c.env) and not c.env and _tiles(c.Nc) > 512 for c in MATRIX)
    assert any(not seq_split(c.Nc, F, c.env) and not c.env and _tiles(c.Nc) > 2048 for c in MATRIX)
    assert any(c.L * _tiles(c.Nc) > 1024 for c in MATRIX) and any(c.L * _tiles(c.Nc) > 512 for c in MATRIX)
    assert any(seq_split(c.Nc, F, c.env) and _tiles(c.Nc) > split_grid(c.Nc, c.env) and c.Nc < 100 for c in MATRIX)
    assert any(nw * nb < nt for nw, nb, nt in (feat16_launch(c.L, c.Nc, c.env) for c in MATRIX if c.Nc < 100))
    # edges
    assert any(c.L == 1 and seq_split(c.Nc, F, c.env) for c in MATRIX) and any(c.L == 1 and not seq_split(c.Nc, F, c.env) for c in MATRIX)
    assert any(c.Nc == 1 and seq_split(c.Nc, F, c.env) for c in MATRIX) and any(c.Nc == 1 and not seq_split(c.Nc, F, c.env) for c in MATRIX)
    assert any(c.Nc % 16 == 0 for c in MATRIX) and any(c.Nc >= 17 for c in MATRIX)          # (>= 17: a tile with no active row)
    assert any(feature_path(c.D, c.LN, c.Nc) == "wide" and c.A > 16 for c in MATRIX)
    assert {c.rows for c in MATRIX} == {T, F} and {(c.rows, seq_split(c.Nc, F, c.env)) for c in MATRIX} == {(r, s) for r in (T, F) for s in (T, F)}
    # NaN fill: every forward / backward path, and an unsplit one whose forward grid differs from the split one (so the
    # partial-row count proves that the override took effect)
    nan_f = {_net_instances(c, a)["fwd"][0::2] for c in MATRIX if c.nan for a in (T, F)}
    nan_b = {_net_instances(c, a)["bwd"] for c in MATRIX if c.nan for a in (T, F)}
    assert nan_f == {(s, b) for s in ("split", "unsplit") for b in (T, F)} and nan_b == bwd
    assert any(c.nan and not seq_split(c.Nc, F, c.env) and head_grid(c.L, c.Nc) != seq_grid(c.Nc, c.env) for c in MATRIX)
    assert any(c.nan and max(c.D, c.S) > 64 for c in MATRIX)


# ---- inputs and the float64 reference ----------------------------------------------------------------------------------
def _kink_margin(a, lp, vals, old_logp, v_old, tgt):
    """_loss_margin of test_gpu_kernels.py on log-probs / values already evaluated (here: by the recurrent float64 forward)."""
    c = a.clip_param
    imp = torch.exp(lp - old_logp)
    m_ratio = torch.minimum((imp - (1 - c)).abs(), (imp - (1 + c)).abs())
    if not a.use_clipped_value_loss:
        return m_ratio.view(-1).numpy()
    d = vals - v_old
    vclip = v_old + d.clamp(-c, c)
    loss = (lambda e: O.huber_ref(e, a.huber_delta)) if a.use_huber_loss else (lambda e: e * e / 2)
    gap = (loss(tgt - vals) - loss(tgt - vclip)).abs()
    m_max = torch.where(d.abs() > c, gap, torch.full_like(gap, np.inf))
    return torch.minimum(torch.minimum(m_ratio, (d.abs() - c).abs()), m_max).view(-1).numpy()


@functools.lru_cache(maxsize=None)
def _inputs(idx):
    """Networks and loss inputs of case `idx`, every minibatch row at least 1e-4 away from the ReLU zero crossings of the trunks
    and from the ratio / value-clip kinks (evaluated with the recurrent float64 forward).  Offending rows are redrawn, not
    deactivated (old_logp and the v_old noise for a loss kink, the observation for a ReLU margin — which moves the later steps of
    that sequence, hence the rounds).  Masks: random at 0.8, step 0 of sequence 0 masked, the last sequence masked at every step;
    the first tile has no active row (Nc >= 17)."""
    c = MATRIX[idx]
    f = np.float32
    L, Nc, D, S, A = c.L, c.Nc, c.D, c.S, c.A
    B = L * Nc
    torch.manual_seed(B + D + S)
    rng = np.random.default_rng(B * 7 + A + idx)
    a = O.default_args(use_ReLU=c.relu, layer_N=c.LN, use_feature_normalization=c.fn, use_recurrent_policy=True, **FLAGS[c.flags])
    actor, critic = O.ActorRef(a, D, A), O.CriticRef(a, S)
    _randomize(actor, D + 3); _randomize(critic, S + 4)
    n_rows, n_h = (B + 64, Nc + 7) if c.rows else (B, Nc)
    rows = rng.permutation(n_rows)[:B].astype(np.int64) if c.rows else np.arange(B)
    h0_rows = rng.permutation(n_h)[:Nc].astype(np.int64) if c.rows else np.arange(Nc)
    obs = rng.standard_normal((n_rows, D)).astype(f)
    sobs = rng.standard_normal((n_rows, S)).astype(f)
    avail = (rng.random((n_rows, A)) > 0.3).astype(f)
    actions = rng.integers(0, A, n_rows).astype(f)
    avail[np.arange(n_rows), actions.astype(int)] = 1.0
    old_logp = (-np.abs(rng.standard_normal(n_rows)) * 0.3 - np.log(A)).astype(f)
    adv = rng.standard_normal(n_rows).astype(f)
    active = (rng.random(n_rows) > 0.25).astype(f)
    ret = (rng.standard_normal(n_rows) * 3).astype(f)
    ret[rng.random(n_rows) > 0.9] *= 20
    noise = (rng.standard_normal(n_rows) * 0.25).astype(f)
    masks = (rng.random(n_rows) > 0.2).astype(f)
    h0a, h0c = (rng.standard_normal((n_h, HID)) * 0.5).astype(f), (rng.standard_normal((n_h, HID)) * 0.5).astype(f)
    steps = np.arange(L)
    masks[rows[0]] = 0.0
    if Nc >= 2:
        masks[rows[steps * Nc + Nc - 1]] = 0.0
    if Nc >= 17:
        active[rows[(steps[:, None] * Nc + np.arange(16)[None, :]).ravel()]] = 0.0
    active[rows[B - 1]] = 1.0
    vn = O.ValueNormRef()
    vn.update(ret[:50].reshape(-1, 1)); vn.update(ret[rows].reshape(-1, 1))
    ad, cd = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    t = lambda x: torch.from_numpy(x[rows]).double()
    th = lambda x: torch.from_numpy(x[h0_rows]).double().unsqueeze(1)
    v_old = np.zeros(n_rows, f)
    tgt = vn.normalize(t(ret).view(-1, 1).float()).double() if a.use_valuenorm else t(ret).view(-1, 1)
    for _ in range(20):
        with torch.no_grad():
            lp, _, _ = ad.evaluate_actions(t(obs), th(h0a), t(actions).view(-1, 1), t(masks).view(-1, 1), t(avail), t(active).view(-1, 1))
            vals = cd(t(sobs), th(h0c), t(masks).view(-1, 1))[0]
        v_old[rows] = (vals.view(-1).numpy() + noise[rows]).astype(f)
        bad_l = np.flatnonzero(_kink_margin(a, lp, vals, t(old_logp).view(-1, 1), t(v_old).view(-1, 1), tgt) < 1e-4)
        bad_a = np.flatnonzero(_relu_margin(ad, t(obs)) < 1e-4) if c.relu else bad_l[:0]
        bad_c = np.flatnonzero(_relu_margin(cd, t(sobs)) < 1e-4) if c.relu else bad_l[:0]
        n_bad = np.union1d(np.union1d(bad_l, bad_a), bad_c).size
        if n_bad == 0:
            return dict(a=a, actor=actor, critic=critic, ad=ad, cd=cd, rows=rows, h0_rows=h0_rows, obs=obs, sobs=sobs, avail=avail,
                        actions=actions, old_logp=old_logp, adv=adv, active=active, ret=ret, v_old=v_old, masks=masks, h0a=h0a,
                        h0c=h0c, vn=vn, tgt=tgt)
        assert n_bad < 0.1 * B, f"case {idx}: {n_bad} of {B} rows within 1e-4 of a kink"
        old_logp[rows[bad_l]] = -np.abs(rng.standard_normal(bad_l.size)) * 0.3 - np.log(A)
        noise[rows[bad_l]] = rng.standard_normal(bad_l.size) * 0.25
        obs[rows[bad_a]] = rng.standard_normal((bad_a.size, D))
        sobs[rows[bad_c]] = rng.standard_normal((bad_c.size, S))
    raise AssertionError(f"case {idx}: could not draw inputs away from the kinks")


def test_gru_matrix_inputs_stay_clear_of_kinks():
    """The float64 reference alone: every case finds inputs 1e-4 away from every kink within the redraw cap (no GPU)."""
    seen = set()
    for idx, c in enumerate(MATRIX):
        x = _inputs(idx)
        rows, L, Nc = x["rows"], c.L, c.Nc
        tm = lambda v: v[rows].reshape(L, Nc)                                  # time-major [t][sequence]
        masks, active = tm(x["masks"]), tm(x["active"])
        assert masks[0, 0] == 0 and active.sum() > 0
        seen.add(("mask 0 at t = 0", seq_split(Nc, F, c.env)))
        if Nc >= 2:
            assert not masks[:, Nc - 1].any()
            seen.add(("all-zero masks", seq_split(Nc, F, c.env)))
        if Nc >= 17:
            assert not active[:, :16].any() and active[:, 16:].any()
            seen.add(("tile without active row", seq_split(Nc, F, c.env)))
        if L > 1 and Nc > 2:
            assert masks[:, 1:Nc - 1].any() and not masks[:, :Nc - 1].all()   # the other sequences: ones and zeros
    # the edges that _inputs builds exist in the arrays, on the split and on the unsplit kernels
    assert seen == {(e, s) for e in ("mask 0 at t = 0", "all-zero masks", "tile without active row") for s in (T, F)}, seen


@functools.lru_cache(maxsize=None)
def _reference(idx):
    """float64 autograd through the oracle networks on the gathered, time-major rows: (value_loss, policy_loss, entropy, ratio
    mean), every parameter's gradient per network, the trunk features and target - value."""
    x = _inputs(idx)
    a, rows, h0_rows = x["a"], x["rows"], x["h0_rows"]
    ad, cd = copy.deepcopy(x["ad"]), copy.deepcopy(x["cd"])
    t = lambda v: torch.from_numpy(v[rows]).double()
    th = lambda v: torch.from_numpy(v[h0_rows]).double().unsqueeze(1)
    act, msk = t(x["active"]).view(-1, 1), t(x["masks"]).view(-1, 1)
    lp, ent, _ = ad.evaluate_actions(t(x["obs"]), th(x["h0a"]), t(x["actions"]).view(-1, 1), msk, t(x["avail"]), act)
    vals = cd(t(x["sobs"]), th(x["h0c"]), msk)[0]
    pl, vl, imp = O.ppo_losses_ref(a, lp, ent, vals, t(x["old_logp"]).view(-1, 1), t(x["adv"]).view(-1, 1), act,
                                   t(x["v_old"]).view(-1, 1), x["tgt"])
    (pl - a.entropy_coef * ent).backward()
    (vl * a.value_loss_coef).backward()
    with torch.no_grad():
        fa, fc = ad.base(t(x["obs"])).numpy(), cd.base(t(x["sobs"])).numpy()
    ga = {k: p.grad.numpy() for k, p in ad.named_parameters() if p.grad is not None}
    gc = {k: p.grad.numpy() for k, p in cd.named_parameters() if p.grad is not None}
    return [vl.item(), pl.item(), ent.item(), imp.mean().item()], ga, gc, fa, fc, (x["tgt"] - vals).detach().numpy()


# ---- the GPU side -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops(gpu_device):
    from mappo_amd import ops as _ops
    return _ops


GUARD = 4096                       # floats behind every work array: must still hold the fill afterwards
GRAD_TOL = 2e-4                    # of max|ref| per parameter: the bound of test_ppo_update_recurrent_golden for these kernels


def _group(key):
    return "gru" if key.startswith("rnn.rnn") else ("norm+head" if key.startswith(("rnn.norm", "act.", "v_out")) else "trunk")


def _unblock(feat, L, Nc):
    """Blocked [L][n_ct][4 b][4 q][16 n][4 i] (feature 16 b + 4 q + i of sequence 16 j + n) -> [L * Nc][64]; padding lanes dropped."""
    n_ct = _tiles(Nc)
    return feat.view(L, n_ct, 4, 4, 16, 4).permute(0, 1, 4, 2, 3, 5).reshape(L, n_ct * 16, HID)[:, :Nc].reshape(L * Nc, HID)


def _one_net(ops, c, actor, params, desc, x, g, h0, cfg, mom, fill, slabs, P, col0, part):
    """The launches of _update_recurrent.one_net on work arrays filled with `fill`; returns the trunk features [B][64]."""
    L, Nc = c.L, c.Nc
    B = L * Nc
    blocked = feature_path(desc.in_dim, c.LN, Nc) != "fm" and not c.fm
    comp, n_scr = ops.gru16_blocked_floats(L, Nc), ops.gru16_scratch_floats(L, Nc)
    assert comp == L * _tiles(Nc) * 1024 and n_scr == 6 * comp
    arr = lambda n: torch.full((n + GUARD,), fill, device="cuda")
    scr_all = arr(n_scr)
    scratch = scr_all[:n_scr]
    feat_all = arr(comp if blocked else HID * B)
    dx_all = None if blocked else arr(HID * B)
    if blocked:
        feat, dxT = feat_all[:comp], None
        ops.mlp_features_seq(params, desc, x, g["rows"], L, Nc, feat)
    else:
        feat, dxT = feat_all[:HID * B].view(HID, B), dx_all[:HID * B].view(HID, B)
        ops.mlp_features(params, desc, x, g["rows"], B, feat)
    head = 1 if actor else 2
    ops.gru16_forward_loss(params, desc, feat, blocked, h0, g["h0_rows"], g["masks"], g["rows"], L, Nc, head,
                           g["avail"] if actor else None, g["actions"] if actor else None, g["old"] if actor else None,
                           g["adv"] if actor else None, g["active"], None if actor else g["vold"], None if actor else g["ret"],
                           None if actor else g["vn"], mom, cfg, scratch, slabs, P, col0, part)
    ops.gru16_backward(params, desc, g["masks"], g["rows"], L, Nc, scratch, dxT)
    ops.gru16_wgrad(desc, feat, blocked, scratch, L, Nc, slabs, P, col0)
    if blocked:
        ops.trunk_backward_seq(params, desc, x, g["rows"], L, Nc, scratch[5 * comp:6 * comp], slabs, P, col0)
    else:
        ops.trunk_backward(params, desc, x, g["rows"], B, dxT, slabs, P, col0)
    torch.cuda.synchronize()
    if fill != fill:
        for nm, t_, n in (("scratch", scr_all, n_scr), ("features", feat_all, feat.numel()), ("d x", dx_all, HID * B)):
            assert t_ is None or bool(torch.isnan(t_[n:]).all()), f"{nm}: written beyond its size"
    return (_unblock(feat, L, Nc) if blocked else feat.t()).double().cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(MATRIX)), ids=IDS)
def test_gru_update_matrix_vs_float64_autograd(ops, monkeypatch, idx):
    """Statistics at the tolerances of test_update_matrix_vs_float64_autograd, trunk features at those of
    test_mlp_forward_vs_oracle, every parameter's gradient within 2e-4 of max|ref| (the bound of
    test_ppo_update_recurrent_golden for these kernels; the worst measured ratio per parameter group is printed).
    Measured on an MI355X over the 23 cases: worst ratio 3.7e-5 (actor trunk of the 2-wide feature-major case), every GRU and
    rnn.norm / head group below 2e-6, so no case needed a wider bound; trunk features within 9.2e-6 absolute.
    The zero-filled run can only bound the partial rows from above (nothing beyond the forward grid); that exactly the forward
    grid's rows are written — which is what shows that a path override took effect — is checked on the NaN-filled cases, and the
    coverage test demands an unsplit one among them whose sequence grid differs from its head grid."""
    c = MATRIX[idx]
    for k in ("MAPPO_GRU16_SPLIT_TILES", "MAPPO_GRU16_SPLIT_TILES_BWD", "MAPPO_GRU16_WAVES", "MAPPO_GRU16_SPLIT_GRID", "MAPPO_FEAT16_GRID"):
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    x = _inputs(idx)
    ref_stats, ga, gc, fa, fc, err = _reference(idx)
    a, L, Nc = x["a"], c.L, c.Nc
    B = L * Nc
    if c.flags == "hyper":
        assert (np.abs(err) > a.huber_delta).any() and (np.abs(err) <= a.huber_delta).any()    # both Huber branches
    da, dc = ops.net_desc(c.D, c.A, c.LN, c.relu, c.fn, recurrent=True), ops.net_desc(c.S, 1, c.LN, c.relu, c.fn, recurrent=True)
    pa, la, Pa = _flat_from_module(ops, x["actor"], da, "act.action_out.linear")
    pc, lc, Pc = _flat_from_module(ops, x["critic"], dc, "v_out")
    g = dict(obs=dev(x["obs"]), sobs=dev(x["sobs"]), avail=dev(x["avail"]), actions=dev(x["actions"]), old=dev(x["old_logp"]),
             adv=dev(x["adv"]), active=dev(x["active"]), ret=dev(x["ret"]), vold=dev(x["v_old"]), masks=dev(x["masks"]),
             vn=dev(x["vn"].state()) if a.use_valuenorm else None,
             rows=dev(x["rows"], torch.int32) if c.rows else None, h0_rows=dev(x["h0_rows"], torch.int32) if c.rows else None)
    h0a, h0c = dev(x["h0a"]), dev(x["h0c"])
    mom = torch.zeros(4, dtype=torch.float64, device="cuda")
    ops.minibatch_moments(g["ret"], g["active"], g["rows"], B, mom)
    cfg = ops.ppo_cfg(a)
    n_bwd, n_fwd = gru16_slabs(L, Nc, c.env), forward_grid(L, Nc, c.env)
    assert ops.gru16_slabs(L, Nc) == n_bwd and ops.mlp_backward_slabs(B) == mlp_backward_slabs(B)     # mirror == library, overrides included
    n_sl = max(n_bwd, mlp_backward_slabs(B))
    col_c = ((Pa + 255) // 256) * 256
    P = col_c + ((Pc + 255) // 256) * 256 + 256                  # a spare 256 columns right of the critic's range
    owned = np.zeros(P, dtype=bool)
    owned[:Pa] = True; owned[col_c:col_c + Pc] = True

    def run(fill):
        slabs = torch.full((n_sl + 3, P), fill, device="cuda")
        part_a = torch.full((1024,), fill, dtype=torch.float64, device="cuda")
        part_c = torch.full((1024,), fill, dtype=torch.float64, device="cuda")
        f_a = _one_net(ops, c, True, pa, da, g["obs"], g, h0a, cfg, mom, fill, slabs, P, 0, part_a)
        f_c = _one_net(ops, c, False, pc, dc, g["sobs"], g, h0c, cfg, mom, fill, slabs, P, col_c, part_c)
        stats = torch.zeros(6, dtype=torch.float64, device="cuda")
        ops.update_stats(part_a, n_fwd, part_c, n_fwd, mom, cfg, stats)
        return slabs.cpu().numpy(), part_a.cpu().numpy().reshape(-1, 4), part_c.cpu().numpy().reshape(-1, 4), stats.cpu().numpy(), f_a, f_c

    s, p_a, p_c, stats, f_a, f_c = run(0.0)
    # nothing outside the networks' columns, nothing at or above mappo_gru16_slabs, no partial row beyond the forward grid
    assert not s[:, ~owned].any() and not s[n_bwd:].any(), "wrote outside its columns / rows"
    assert not p_a[n_fwd:].any() and not p_c[n_fwd:].any(), "wrote loss partials beyond the forward grid"
    # trunk features alone (tolerance of test_mlp_forward_vs_oracle for O(1) outputs)
    print(f"\n{IDS[idx]}: features max|err| actor {np.abs(f_a - fa).max():.2e} critic {np.abs(f_c - fc).max():.2e}")
    close(f_a, fa, 1e-5, 2e-5, "actor trunk features"); close(f_c, fc, 1e-5, 2e-5, "critic trunk features")
    print(f"{IDS[idx]}: stats {stats[:4]} ref {ref_stats}")
    close(stats[:4], ref_stats, 1e-5, 1e-7, "stats vs float64 autograd")
    grad = s.astype(np.float64).sum(0)
    worst, fails = {}, []
    for net, layout, c0, gref in (("actor", la, 0, ga), ("critic", lc, col_c, gc)):
        for key, off, shape in layout:
            got, want = grad[c0 + off: c0 + off + int(np.prod(shape))].reshape(shape), gref[key]
            r = np.abs(got - want).max() / max(np.abs(want).max(), 1e-12)
            worst[(net, _group(key))] = max(worst.get((net, _group(key)), 0.0), r)
            if not r <= GRAD_TOL:
                fails.append(f"{net} {key}: {r:.3e}")
    print(f"{IDS[idx]}: grad max err / max|ref| " + ", ".join(f"{n} {k} {v:.2e}" for (n, k), v in sorted(worst.items())))
    assert not fails, f"gradient beyond {GRAD_TOL} of max|ref|: {fails}"

    if c.nan:
        sn, pn_a, pn_c, stats_n, _, _ = run(float("nan"))
        fin = np.isfinite(sn)
        assert not fin[:, ~owned].any(), "wrote outside [col0, col0 + param_count)"
        assert not fin[n_bwd:].any(), "wrote a slab row at or above mappo_gru16_slabs"
        inside = fin[:, owned]
        assert (inside[1:] <= inside[:-1]).all(), "a column's written rows are not a prefix"
        assert inside[0].all(), "a parameter's column was never written"
        for p in (pn_a, pn_c):
            assert np.isfinite(p[:n_fwd]).all() and np.isnan(p[n_fwd:]).all(), \
                f"partial rows written: {np.flatnonzero(np.isfinite(p).any(1))}, forward grid {n_fwd}"
        close(stats_n, stats, 0, 0, "stats: NaN-filled vs zero-filled buffers")
        grad_n = np.nansum(sn.astype(np.float64), axis=0)
        for c0, Pn in ((0, Pa), (col_c, Pc)):
            close_rel_max(grad_n[c0:c0 + Pn], grad[c0:c0 + Pn], 1e-6, "grad: NaN-filled vs zero-filled arrays")


# ---- trainer level: two minibatch shapes on one trainer ------------------------------------------------------------------
def _rec_sample(L, Nc, D, S, A, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    B = L * Nc
    avail = (rng.random((B, A)) > 0.3).astype(f)
    actions = rng.integers(0, A, (B, 1)).astype(f)
    avail[np.arange(B), actions[:, 0].astype(int)] = 1.0
    n = lambda *s: rng.standard_normal(s).astype(f)
    return (n(B, S), n(B, D), n(Nc, 1, HID) * 0.5, n(Nc, 1, HID) * 0.5, actions, n(B, 1) * 0.3, n(B, 1) * 2,
            (rng.random((B, 1)) > 0.2).astype(f), (rng.random((B, 1)) > 0.2).astype(f), (-np.abs(n(B, 1)) * 0.3 - np.log(A)).astype(f),
            n(B, 1), avail)


@pytest.mark.gpu
@pytest.mark.parametrize("Nc1,Nc2", [(2000, 1000), (600, 100)])
def test_recurrent_update_shape_change_on_one_trainer(M, Nc1, Nc2):
    """R_MAPPO.ppo_update with a sample of (L = 10, Nc1), then one of (L = 10, Nc2 < Nc1), against a fresh trainer that gets only
    the second: the six statistics and the flat gradient must be equal bit for bit.  Every kernel of the recurrent chain writes
    one slab / partial row per workgroup of its own grid and the reductions sum a fixed row count, so a row written for the first
    shape must not reach the second's sums.  (2000, 1000): 256 slab rows both times, the head kernel's grid shrinks from 256 to 158;
    (600, 100): slab rows 190 -> 35, partial rows 95 -> 18 of the 35 that mappo_update_stats sums.  Learning rates are zero so the
    weights stay put; the ValueNorm state is reset before each call.

    _update_recurrent keeps its slabs and loss partials per (L, Nc) for this reason.  With the partials shared by all shapes and
    the slabs shared per row count both pairs failed on an MI355X (second call on the used trainer / fresh trainer):
      (2000, 1000)  value loss 1.7961 / 1.1247, policy loss 0.4036 / 0.2619, entropy 2.1149 / 1.3024, ratio 2.9777 / 1.8305,
                    critic gradient norm 2.9807 / 2.7049, actor gradient norm 0.10390 / 0.09516, flat_grad off by 0.313 of its maximum
      (600, 100)    value loss 2.2836 / 1.0788, policy loss 0.6133 / 0.1924, entropy 2.6785 / 1.3062, ratio 3.8128 / 1.8292;
                    gradient norms and flat_grad equal (another row count: another slab array)."""
    L, D, S, A = 10, 12, 20, 5
    a = make_args(M, use_recurrent_policy=True, data_chunk_length=L, lr=0.0, critic_lr=0.0, perm_device="cpu", hidden_size=HID)
    torch.manual_seed(5)
    pol0 = M.R_MAPPOPolicy(a, [D], [S], M.Discrete(A))
    sd_a, sd_c = copy.deepcopy(pol0.actor.state_dict()), copy.deepcopy(pol0.critic.state_dict())
    vn0 = np.array([0.1, 2.0, 0.5], np.float32)
    s1, s2 = _rec_sample(L, Nc1, D, S, A, 11), _rec_sample(L, Nc2, D, S, A, 12)

    def trainer():
        pol = M.R_MAPPOPolicy(a, [D], [S], M.Discrete(A))
        pol.actor.load_state_dict(sd_a); pol.critic.load_state_dict(sd_c)
        return pol, M.R_MAPPO(a, pol)

    pol, tr = trainer()
    set_vn(tr, vn0)
    tr.ppo_update(s1)
    set_vn(tr, vn0)
    out = np.array(tr.ppo_update(s2), dtype=np.float64)
    grad = pol.flat_grad.clone()
    pol_f, tr_f = trainer()
    set_vn(tr_f, vn0)
    out_f = np.array(tr_f.ppo_update(s2), dtype=np.float64)
    assert torch.equal(pol.flat_params, pol_f.flat_params)                     # zero learning rates: same weights
    names = ("value_loss", "critic_grad_norm", "policy_loss", "dist_entropy", "actor_grad_norm", "ratio")
    print("\nafter the larger shape / fresh: " + ", ".join(f"{n} {x:.9g} / {y:.9g}" for n, x, y in zip(names, out, out_f)))
    diff = (grad - pol_f.flat_grad).abs().max().item() / pol_f.flat_grad.abs().max().item()
    print(f"flat_grad max|diff| / max|fresh| = {diff:.3e}")
    assert np.array_equal(out, out_f), dict(zip(names, zip(out, out_f)))
    assert torch.equal(grad, pol_f.flat_grad), f"flat_grad differs by {diff:.3e} of its maximum"
