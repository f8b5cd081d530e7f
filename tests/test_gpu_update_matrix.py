"""Every fused PPO update path against a float64 reference.

mappo_actor_update / mappo_critic_update (launch_update<HEAD> in mlp.hip) and mappo_actor_critic_update choose among four
kernel families, each instantiated over the activation, layer_N and (network, input width):

    upd16   one wave per 16-sample tile (mlp_upd16.h)          in_dim <= 64, layer_N <= 1, actor out_dim <= 16, LDS layout fits
    upd16x  the same from z1 on, layer 1 in mlp_wide16.h      65..512 inputs, layer_N <= 1, actor out_dim <= 16
    upd2    pair kernel (mlp_upd2.h)                           in_dim <= 64 otherwise
    wide    K-chunked wide kernel (mlp_update_kernel, mlp_upd.h)  65..512 inputs otherwise

and the dual launch takes upd16d (both networks upd16) or upd2d (the pair kernel for both).  MATRIX is a covering design of
those instances with every loss flag set and feature normalisation off on every family; test_matrix_covers_every_instance
checks that on the CPU through a Python mirror of the dispatch.  Each case runs the fused single-network launches, the dual
launch (in_dim <= 64) and the unfused sequence (mlp_forward -> ppo_loss_fwd_bwd -> mlp_backward) and compares all three with
float64 autograd through the oracle networks and the oracle's loss expressions (O.ppo_losses_ref).  Cases marked `nan` fill
the slabs and loss partials with NaN and check the write contract of each entry point.

test_ppo_update_flag_sweep runs R_MAPPO.ppo_update, fused and unfused, on the H = 64 fixture cases with each flag flipped,
against O.ppo_update_ref in float64."""
import copy

import numpy as np
import pytest
import torch

from conftest import golden, sub
from oracle import mappo_oracle as O
from test_gpu_e2e import M, make_args, set_vn, TUPLE   # noqa: F401  (M: the trainer-level fixture)
from test_gpu_kernels import close, close_rel_max, dev, _flat_from_module, _randomize, _relu_margin, _loss_margin

# ---- Python mirror of the dispatch (mappo_amd/csrc/mlp.hip, mlp_upd16.h) -------------------------------------------
HID, NUM_CU, UPD16_WAVES, TS = 64, 256, 8, 32
UPD16_LDS_MAX = 160 * 1024 - 256                                     # UPD16_LDS_MAX


def l16_total(LN, HEAD, WIDE):
    """L16<LN, HEAD, WIDE>::TOTAL (mlp_upd16.h), floats."""
    CP, NBK = (16, 4) if WIDE else (8, 2)
    XST = 16 * NBK + 4
    W2 = HID * 4 * CP
    WH = W2 + (2 * HID * HID if LN > 0 else 0)
    B1 = WH + (16 * 80 if HEAD == 1 else HID)
    TILES = B1 + 2 * HID + 16 + 6 * HID                         # B2, BH | FN_W | FN_B, G1, T1, G2, T2
    wave_stride = 16 * XST + (16 * 68 if LN > 0 else 0) + 16 * 68 + (16 * 20 if HEAD == 1 else 0)
    DMAX = 64 if WIDE else 32
    PMAX = 2 * DMAX + HID * DMAX + 3 * HID + (HID * HID + 3 * HID if LN > 0 else 0) + (16 * HID + 16 if HEAD == 1 else HID + 1)
    cap = (160 * 1024 - 256) // 4
    epi4, epi8 = 1024 + UPD16_WAVES * 4 * 256 + PMAX, 1024 + UPD16_WAVES * 8 * 256 + PMAX
    ta0 = max(UPD16_WAVES * wave_stride, epi4)
    ta = epi8 if ta0 < epi8 and TILES + epi8 <= cap and 2 * (TILES + ta0) > cap else ta0
    return TILES + ta


def upd16_eligible(D, out, LN, actor):
    """upd16_eligible (with upd16_lds_floats)."""
    return (D <= 64 and LN <= 1 and (out <= 16 if actor else out == 1)
            and 4 * l16_total(LN, 1 if actor else 2, D > 32) <= UPD16_LDS_MAX)


def upd16x_eligible(D, out, LN, actor):
    """upd16x_eligible."""
    return 64 < D <= 512 and LN <= 1 and (out <= 16 if actor else out == 1)


def single_family(D, out, LN, actor):
    """launch_update<1 | 2>."""
    if upd16_eligible(D, out, LN, actor):
        return "upd16"
    if upd16x_eligible(D, out, LN, actor):
        return "upd16x"
    return "upd2" if D <= 64 else "wide"


def dual_family(D, S, A, LN):
    """mappo_actor_critic_update (both in_dim <= 64)."""
    return "upd16d" if upd16_eligible(D, A, LN, True) and upd16_eligible(S, 1, LN, False) else "upd2d"


def upd16_tile_cost(D, out, LN, actor):
    """upd16_tile_cost."""
    c = 4 * ((D + 3) // 4) + 16 * (4 if D > 32 else 2) + 40 + (3 * 64 if LN > 0 else 0)
    return c + (32 + 4 * ((out + 3) // 4) if actor else 0)


def upd16_split(D, S, A, LN, B):
    """upd16_split: workgroups (nA, nC) of the dual 16-sample-tile launch."""
    want = ((B + 15) // 16 + UPD16_WAVES - 1) // UPD16_WAVES
    ca, cc = upd16_tile_cost(D, A, LN, True), upd16_tile_cost(S, 1, LN, False)
    a = min(max(NUM_CU * ca // (ca + cc), 64), NUM_CU - 64)
    return min(want, a), min(want, NUM_CU - a)


def dual_slabs(D, S, A, LN, B):
    """mappo_dual_update_slabs."""
    if dual_family(D, S, A, LN) == "upd16d":
        return max(upd16_split(D, S, A, LN, B))
    return min((B + TS - 1) // TS, NUM_CU // 2)


# ---- the matrix ------------------------------------------------------------------------------------------------------
FLAGS = {"default": {}, "huber_off": dict(use_huber_loss=False), "vclip_off": dict(use_clipped_value_loss=False),
         "pmask_off": dict(use_policy_active_masks=False), "vmask_off": dict(use_value_active_masks=False),
         "vn_off": dict(use_valuenorm=False),
         "hyper": dict(clip_param=0.05, entropy_coef=0.1, value_loss_coef=0.5, huber_delta=1.0)}

# actor in_dim D, critic in_dim S, actions A, layer_N, ReLU, feature norm, B, gathered rows, flag set, NaN-filled slabs
MATRIX = [
    # upd16: narrow / 33..64 bodies, out_dim <= 8 and 9..16, both activations and layer_N
    (20, 44, 5, 1, True, True, 1500, True, "default", True),
    (40, 12, 12, 0, False, False, 2100, False, "huber_off", False),
    (9, 64, 16, 1, False, True, 3001, True, "vclip_off", False),
    (30, 7, 3, 0, True, True, 999, True, "pmask_off", False),
    (50, 33, 8, 0, True, False, 1234, False, "vmask_off", False),
    (25, 40, 10, 1, True, True, 2500, True, "vn_off", False),
    (14, 50, 2, 1, False, True, 640, True, "hyper", False),
    (61, 3, 16, 0, False, True, 777, True, "default", False),
    # upd16 dual launch with unequal shares: nA < nC (the bench networks) and nA > nC
    (18, 54, 5, 1, True, True, 16500, True, "default", True),
    (60, 5, 16, 0, False, True, 12000, True, "pmask_off", True),
    # pair kernel: an actor with 33..64 inputs and layer_N = 1 (its upd16 layout needs 171 072 B of LDS), out_dim > 16, layer_N = 2
    (36, 54, 5, 1, True, True, 777, True, "default", True),
    (44, 16, 9, 1, False, False, 900, True, "vmask_off", False),
    (33, 20, 32, 2, False, True, 2000, True, "default", True),
    (12, 60, 17, 2, True, False, 1111, False, "huber_off", False),
    (24, 64, 20, 0, False, True, 1600, True, "vclip_off", False),
    (48, 30, 18, 1, True, True, 3333, True, "pmask_off", False),
    (64, 10, 25, 2, True, True, 2222, False, "vn_off", False),
    (8, 41, 24, 1, False, True, 1500, True, "hyper", False),
    (52, 22, 19, 0, True, True, 1000, True, "hyper", False),
    (5, 9, 17, 2, False, True, 333, True, "vn_off", False),
    # upd16x: 65..512 inputs, layer_N <= 1
    (130, 70, 5, 1, True, True, 2000, True, "default", True),
    (200, 300, 16, 0, False, False, 1500, False, "huber_off", False),
    (77, 129, 9, 1, False, True, 2600, True, "vclip_off", False),
    (100, 90, 3, 0, True, True, 1800, True, "pmask_off", False),
    (512, 66, 12, 1, True, True, 1000, False, "vmask_off", False),
    (96, 256, 4, 0, True, True, 700, True, "vn_off", False),
    (300, 80, 8, 1, False, True, 1200, True, "hyper", False),
    (140, 260, 5, 1, True, True, 40000, True, "default", False),          # steady state: > 2 048 tiles of 16
    # K-chunked wide kernel: layer_N = 2 or actor out_dim > 16
    (130, 100, 18, 2, True, True, 1500, True, "default", True),
    (70, 200, 20, 0, False, False, 1300, False, "huber_off", False),
    (90, 66, 32, 1, True, True, 2000, True, "vclip_off", False),
    (256, 90, 17, 2, False, True, 900, True, "pmask_off", False),
    (66, 140, 24, 2, True, False, 1100, False, "vmask_off", False),
    (180, 75, 19, 0, True, True, 1000, True, "vn_off", False),
    (400, 300, 21, 2, False, True, 800, True, "hyper", False),
    (120, 80, 30, 1, False, True, 1300, True, "pmask_off", False),
    (200, 130, 18, 2, True, True, 36000, True, "default", False),         # steady state
]


def _case_instances(c):
    """{(family, layer_N, relu)} a MATRIX case launches, with its feature-norm and flag settings."""
    D, S, A, LN, relu, fn, B, _, flags, _ = c
    fams = {single_family(D, A, LN, True), single_family(S, 1, LN, False)}
    if D <= 64 and S <= 64:
        fams.add(dual_family(D, S, A, LN))
    return {(f, LN, relu) for f in fams}


def test_matrix_covers_every_instance():
    """The covering design reaches every (family, layer_N, activation) instance that HEAD 1 / 2 can reach, both body widths
    of the 16-sample-tile and pair kernels on each network, the three actor head sizes, both split directions of the upd16
    dual launch, feature normalisation off and every flag set on every family."""
    reach = set()
    for D in range(1, 513):
        for out, actor in [(o, True) for o in (2, 8, 9, 16, 17, 32)] + [(1, False)]:
            for LN in (0, 1, 2):
                for relu in (False, True):
                    reach.add((single_family(D, out, LN, actor), LN, relu))
                    if D <= 64 and actor:
                        reach.add((dual_family(D, 54, out, LN), LN, relu))
                        reach.add((dual_family(D, 18, out, LN), LN, relu))
    got = set().union(*(_case_instances(c) for c in MATRIX))
    assert got == reach, reach - got
    # the layout that does not fit is no longer eligible, the bench shape still is (18-wide actor, 54-wide critic, layer_N 1)
    assert 4 * l16_total(1, 1, True) == 171072 > UPD16_LDS_MAX and not upd16_eligible(36, 5, 1, True)
    assert dual_family(18, 54, 5, 1) == "upd16d" and single_family(54, 1, 1, False) == "upd16"
    fam_flags, fam_nofn, bodies, heads, splits = {}, set(), set(), set(), set()
    for c in MATRIX:
        D, S, A, LN, relu, fn, B, _, flags, _ = c
        for f, _, _ in _case_instances(c):
            fam_flags.setdefault(f, set()).add(flags)
            if not fn:
                fam_nofn.add(f)
        for d, out, actor in ((D, A, True), (S, 1, False)):
            f = single_family(d, out, LN, actor)
            if f in ("upd16", "upd2"):
                bodies.add((f, actor, d > 32))
        if single_family(D, A, LN, True) == "upd16":
            heads.add("<=8" if A <= 8 else "9..16")
        elif single_family(D, A, LN, True) in ("upd2", "wide"):
            heads.add(">16" if A > 16 else "pair<=16")
        if c[-1] and D <= 64 and S <= 64 and dual_family(D, S, A, LN) == "upd16d":
            nA, nC = upd16_split(D, S, A, LN, B)
            splits.add((nA > nC) - (nA < nC))
    families = {"upd16", "upd16x", "upd2", "wide", "upd16d", "upd2d"}
    assert set(fam_flags) == families
    for f in families:
        assert fam_flags[f] == set(FLAGS), (f, set(FLAGS) - fam_flags[f])
    assert fam_nofn == families
    assert bodies == {(f, actor, w) for f in ("upd16", "upd2") for actor in (True, False) for w in (False, True)}, bodies
    assert {"<=8", "9..16", ">16", "pair<=16"} <= heads
    assert {-1, 1} <= splits                                      # NaN-filled slabs with nA < nC and nA > nC
    assert {single_family(d, o, c[3], o > 1) for c in MATRIX if c[-1] for d, o in ((c[0], c[2]), (c[1], 1))} >= {"upd16x", "wide"}
    assert any(B > 2048 * 16 and single_family(D, A, LN, True) == "upd16x" for D, S, A, LN, _, _, B, *_ in MATRIX)
    assert any(B > 2048 * 16 and single_family(S, 1, LN, False) == "wide" for D, S, A, LN, _, _, B, *_ in MATRIX)


@pytest.fixture(scope="module")
def ops(gpu_device):
    from mappo_amd import ops as _ops
    return _ops


def _safe_inputs(a, actor, critic, rng, n_rows, D, S, A, relu, flags):
    """Loss inputs whose every row is at least 1e-4 away from the non-smooth points of the ReLU trunks and of the losses
    (_relu_margin / _loss_margin): all implementations then differentiate the same function.  Unsafe rows are redrawn, not
    deactivated: with the active masks off an inactive row still counts."""
    f = np.float32
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
    vn = O.ValueNormRef()
    vn.update(ret[:50].reshape(-1, 1))
    for _ in range(20):
        with torch.no_grad():
            v_now = critic(torch.from_numpy(sobs), None, None)[0].numpy().reshape(-1)
        v_old = (v_now + noise).astype(f)
        m = _loss_margin(a, actor, critic, obs, sobs, actions, avail, active, old_logp, v_old, ret, vn)
        if relu:
            m = np.minimum(m, np.minimum(_relu_margin(actor, torch.from_numpy(obs)), _relu_margin(critic, torch.from_numpy(sobs))))
        bad = np.flatnonzero(m < 1e-4)
        if bad.size == 0:
            return obs, sobs, avail, actions, old_logp, adv, active, ret, v_old
        assert bad.size < 0.1 * n_rows
        obs[bad] = rng.standard_normal((bad.size, D))
        sobs[bad] = rng.standard_normal((bad.size, S))
        old_logp[bad] = -np.abs(rng.standard_normal(bad.size)) * 0.3 - np.log(A)
        noise[bad] = rng.standard_normal(bad.size) * 0.25
    raise AssertionError("could not draw inputs away from the kinks")


def _reference(a, actor, critic, rows, obs, sobs, avail, actions, old_logp, adv, active, v_old, ret, vn):
    """float64 autograd through deep copies of the oracle networks: (value_loss, policy_loss, entropy, ratio mean) and the
    gradient of every parameter of each network."""
    ad, cd = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    t = lambda x: torch.from_numpy(x[rows]).double()
    act = t(active).view(-1, 1)
    lp, ent, _ = ad.evaluate_actions(t(obs), None, t(actions).view(-1, 1), None, None if avail is None else t(avail), act)
    vals = cd(t(sobs), None, None)[0]
    ret_t = t(ret).view(-1, 1)
    tgt = vn.normalize(ret_t.float()).double() if a.use_valuenorm else ret_t
    pl, vl, imp = O.ppo_losses_ref(a, lp, ent, vals, t(old_logp).view(-1, 1), t(adv).view(-1, 1), act, t(v_old).view(-1, 1), tgt)
    (pl - a.entropy_coef * ent).backward()
    (vl * a.value_loss_coef).backward()
    stats = [vl.item(), pl.item(), ent.item(), imp.mean().item()]
    ga = {k: p.grad.numpy() for k, p in ad.named_parameters() if p.grad is not None}
    gc = {k: p.grad.numpy() for k, p in cd.named_parameters() if p.grad is not None}
    return stats, ga, gc, (tgt - vals).detach().numpy()


def _check_grads(gflat, la, lc, col_c, ga, gc, what):
    for key, off, shape in la:
        close_rel_max(gflat[off: off + int(np.prod(shape))].reshape(shape), ga[key], 1e-4, f"{what}: actor {key}")
    for key, off, shape in lc:
        close_rel_max(gflat[col_c + off: col_c + off + int(np.prod(shape))].reshape(shape), gc[key], 1e-4, f"{what}: critic {key}")


def _check_written(s, rows_written, ranges, what):
    """Slab rows [0, rows_written) are finite in every column range the launch owns; every other entry is still NaN."""
    owned = np.zeros(s.shape, dtype=bool)
    for c0, n in ranges:
        owned[:rows_written, c0:c0 + n] = True
    assert np.isfinite(s[owned]).all(), f"{what}: a promised slab entry was not written"
    assert np.isnan(s[~owned]).all(), f"{what}: wrote outside its rows / columns"


def _check_partials(p, rows_written, what):
    p = p.view(-1, 4).cpu().numpy()
    assert np.isfinite(p[:rows_written]).all(), f"{what}: a promised loss-partial row was not written"
    assert np.isnan(p[rows_written:]).all(), f"{what}: wrote loss partials beyond its rows"


@pytest.mark.gpu
@pytest.mark.parametrize("D,S,A,LN,relu,fn,B,with_rows,flags,nan", MATRIX)
def test_update_matrix_vs_float64_autograd(ops, D, S, A, LN, relu, fn, B, with_rows, flags, nan):
    torch.manual_seed(B + D + S)
    rng = np.random.default_rng(B * 7 + A)
    a = O.default_args(use_ReLU=relu, layer_N=LN, use_feature_normalization=fn, **FLAGS[flags])
    actor, critic = O.ActorRef(a, D, A), O.CriticRef(a, S)
    _randomize(actor, D + 3); _randomize(critic, S + 4)
    da, dc = ops.net_desc(D, A, LN, relu, fn), ops.net_desc(S, 1, LN, relu, fn)
    pa, la, Pa = _flat_from_module(ops, actor, da, "act.action_out.linear")
    pc, lc, Pc = _flat_from_module(ops, critic, dc, "v_out")
    n_rows = B + 64 if with_rows else B
    rows = rng.permutation(n_rows)[:B].astype(np.int32) if with_rows else np.arange(B, dtype=np.int32)
    obs, sobs, avail, actions, old_logp, adv, active, ret, v_old = _safe_inputs(a, actor, critic, rng, n_rows, D, S, A, relu, flags)
    vn = O.ValueNormRef(); vn.update(ret[:50].reshape(-1, 1)); vn.update(ret[rows].reshape(-1, 1))
    ref_stats, ga, gc, err = _reference(a, actor, critic, rows.astype(np.int64), obs, sobs, avail, actions, old_logp, adv, active,
                                        v_old, ret, vn)
    if flags == "hyper":
        assert (np.abs(err) > a.huber_delta).any() and (np.abs(err) <= a.huber_delta).any()    # both Huber branches
    d_rows = dev(rows, torch.int32) if with_rows else None
    g = dict(obs=dev(obs), sobs=dev(sobs), avail=dev(avail), actions=dev(actions), old=dev(old_logp), adv=dev(adv),
             active=dev(active), ret=dev(ret), vold=dev(v_old), vn=dev(vn.state()) if a.use_valuenorm else None)
    mom = torch.zeros(4, dtype=torch.float64, device="cuda")
    ops.minibatch_moments(g["ret"], g["active"], d_rows, B, mom)
    cfg = ops.ppo_cfg(a)
    ns = ops.mlp_backward_slabs(B)
    col_c = ((Pa + 255) // 256) * 256
    P = col_c + ((Pc + 255) // 256) * 256 + 256                 # a spare 256 columns after the critic's range: must stay untouched
    nanf = float("nan")

    def partials(fill):
        return torch.full((ops.update_partials("cuda").numel(),), fill, dtype=torch.float64, device="cuda")

    # (1) fused single-network launches
    def single(fill):
        slabs = torch.full((ns + 3, P), fill, device="cuda")
        for d, c0, Pn in ((D, 0, Pa), (S, col_c, Pc)):
            if d > 64:
                slabs[:ns, c0:c0 + Pn] = 0.0     # wide inputs: the caller zeroes its column range (mappo_wide_l1_backward writes fewer rows)
        part_a, part_c = partials(fill), partials(fill)
        ops.actor_update(pa, da, g["obs"], d_rows, B, g["avail"], g["actions"], g["old"], g["adv"], g["active"], mom, cfg, slabs, P, 0, part_a)
        ops.critic_update(pc, dc, g["sobs"], d_rows, B, g["vold"], g["ret"], g["active"], g["vn"], mom, cfg, slabs, P, col_c, part_c)
        stats = torch.zeros(6, dtype=torch.float64, device="cuda")
        ops.update_stats(part_a, ns, part_c, ns, mom, cfg, stats)
        grad = torch.zeros(P, device="cuda")
        ops.slab_reduce(slabs, ns, P, P, grad)
        return slabs, part_a, part_c, stats.cpu().numpy(), grad.cpu().numpy()

    _, _, _, stats_f, grad_f = single(0.0)
    close(stats_f[:4], ref_stats, 1e-5, 1e-7, "fused stats vs float64 autograd")
    _check_grads(grad_f, la, lc, col_c, ga, gc, "fused")
    if nan:
        slabs, part_a, part_c, stats_n, grad_n = single(nanf)
        _check_written(slabs.cpu().numpy(), ns, [(0, Pa), (col_c, Pc)], "single launches")
        _check_partials(part_a, ns, "actor_update"); _check_partials(part_c, ns, "critic_update")
        close(stats_n, stats_f, 0, 0, "stats: NaN-filled vs zero-filled buffers")
        for c0, Pn in ((0, Pa), (col_c, Pc)):
            close_rel_max(grad_n[c0:c0 + Pn], grad_f[c0:c0 + Pn], 1e-6, "grad: NaN-filled vs zero-filled slabs")

    # (2) both networks in one launch
    if D <= 64 and S <= 64:
        nd = ops.dual_update_slabs(da, dc, B)
        assert nd == dual_slabs(D, S, A, LN, B)                   # the Python mirror of the dispatch agrees with the library

        def dual(fill):
            slabs = torch.full((nd + 3, P), fill, device="cuda")
            pda, pdc = partials(fill), partials(fill)
            ops.actor_critic_update(pa, da, g["obs"], pc, dc, g["sobs"], d_rows, B, g["avail"], g["actions"], g["old"], g["adv"],
                                    g["active"], g["vold"], g["ret"], g["vn"], mom, cfg, slabs, P, 0, col_c, pda, pdc)
            stats = torch.zeros(6, dtype=torch.float64, device="cuda")
            ops.update_stats(pda, nd, pdc, nd, mom, cfg, stats)
            grad = torch.zeros(P, device="cuda")
            ops.slab_reduce(slabs, nd, P, P, grad)
            return slabs, pda, pdc, stats.cpu().numpy(), grad.cpu().numpy()

        _, _, _, stats_d, grad_d = dual(0.0)
        close(stats_d, stats_f, 1e-6, 1e-9, "stats dual vs separate launches")
        close_rel_max(grad_d, grad_f, 2e-6, "grad dual vs separate launches")
        close(stats_d[:4], ref_stats, 1e-5, 1e-7, "dual stats vs float64 autograd")
        _check_grads(grad_d, la, lc, col_c, ga, gc, "dual")
        if nan:
            slabs, pda, pdc, stats_n, grad_n = dual(nanf)
            _check_written(slabs.cpu().numpy(), nd, [(0, Pa), (col_c, Pc)], "dual launch")
            _check_partials(pda, nd, "dual launch, actor"); _check_partials(pdc, nd, "dual launch, critic")
            close(stats_n, stats_d, 0, 0, "dual stats: NaN-filled vs zero-filled buffers")
            for c0, Pn in ((0, Pa), (col_c, Pc)):
                close_rel_max(grad_n[c0:c0 + Pn], grad_d[c0:c0 + Pn], 1e-6, "dual grad: NaN-filled vs zero-filled slabs")

    # (3) unfused: forward, standalone loss, backward
    logits, values = torch.zeros(B, A, device="cuda"), torch.zeros(B, device="cuda")
    ops.mlp_forward(pa, da, g["obs"], d_rows, B, logits)
    ops.mlp_forward(pc, dc, g["sobs"], d_rows, B, values)
    dl, dv = torch.zeros(B, A, device="cuda"), torch.zeros(B, device="cuda")
    stats_u = torch.zeros(6, dtype=torch.float64, device="cuda")
    ops.ppo_loss_fwd_bwd(logits, values, d_rows, g["avail"], g["actions"], g["old"], g["adv"], g["active"], g["vold"], g["ret"],
                         g["vn"], mom, dl, dv, stats_u, cfg)
    slabs_u = torch.zeros(ns, P, device="cuda")
    ops.mlp_backward(pa, da, g["obs"], d_rows, B, dl, slabs_u, P, 0)
    ops.mlp_backward(pc, dc, g["sobs"], d_rows, B, dv.view(B, 1), slabs_u, P, col_c)
    grad_u = torch.zeros(P, device="cuda")
    ops.slab_reduce(slabs_u, ns, P, P, grad_u)
    stats_u = stats_u.cpu().numpy()
    assert np.array_equal(stats_f[4:], stats_u[4:])
    close(stats_u[:4], ref_stats, 1e-5, 1e-7, "unfused stats vs float64 autograd")
    _check_grads(grad_u.cpu().numpy(), la, lc, col_c, ga, gc, "unfused")


# ---- trainer level: R_MAPPO.ppo_update with every flag flipped ---------------------------------------------------------
SWEEP = dict(FLAGS, clip_norm=dict(max_grad_norm=0.05), no_clip=dict(use_max_grad_norm=False), critic_only={}, two_steps={})


def _policy_pair(M, a, oa, D, S, A, state=None, seed=0):
    """A trainer policy and a float64 oracle policy with the same weights (`state`: fixture prefix, else random)."""
    pol = M.R_MAPPOPolicy(a, [D], [S], M.Discrete(A))
    opol = O.PolicyRef(oa, D, S, A)
    if state is None:
        _randomize(opol.actor, seed); _randomize(opol.critic, seed + 1)
    else:
        g, prefix = state
        opol.actor.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sub(g, f"{prefix}/actor0").items()})
        opol.critic.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sub(g, f"{prefix}/critic0").items()})
    pol.actor.load_state_dict(opol.actor.state_dict())
    pol.critic.load_state_dict(opol.critic.state_dict())
    opol.actor.double(); opol.critic.double()                    # in place: the Adam optimizers keep their parameters
    return pol, opol


def _compare_update(M, a, oa, pol, opol, sample, vn0, steps, update_actor, rec, what, policy_stats=True):
    tr = M.R_MAPPO(a, pol)
    ovn = None
    if a.use_valuenorm:
        set_vn(tr, vn0)
        ovn = O.ValueNormRef(); ovn.load_state(vn0)
    stat_tol, grad_tol, p_atol = (2e-5, 2e-4, 4e-6) if rec else (2e-6, 1e-4, 3e-6)
    for rep in range(steps):
        out = tr.ppo_update(sample, update_actor)
        vl, cn, pl, ent, an, imp = O.ppo_update_ref(oa, opol, ovn, sample, update_actor, dtype=torch.float64)
        ref = [vl, cn, pl, ent, an, float(imp.mean())]
        keep = [0, 1, 2, 3, 4, 5] if policy_stats else [0, 1, 4]
        close(np.array(out, dtype=np.float64)[keep], np.array(ref)[keep], stat_tol, 1e-8, f"{what} step {rep}: stats")
        for seg, net, onet, norm in ((0, pol.actor, opol.actor, an), (1, pol.critic, opol.critic, cn)):
            lo = pol.seg_bounds[seg]
            # flat_grad is the gradient before clipping; the oracle's .grad after clip_grad_norm_
            coef = min(1.0, oa.max_grad_norm / (norm + 1e-6)) if oa.use_max_grad_norm else 1.0
            og = dict(onet.named_parameters())
            for key, off, shape in net.layout:
                n = int(np.prod(shape))
                got = pol.flat_grad[lo + off: lo + off + n].view(shape)
                if og[key].grad is None:
                    assert seg == 0 and not update_actor and not got.abs().max().item(), f"{what}: actor gradient without update_actor"
                    continue
                close_rel_max(got, og[key].grad.numpy() / coef, grad_tol, f"{what} step {rep}: grad {key}")
            osd = onet.state_dict()
            for k, v in net.state_dict().items():
                close(v, osd[k].numpy(), 1e-5, p_atol, f"{what} step {rep}: {k}")
            opt = opol.actor_optimizer if seg == 0 else opol.critic_optimizer
            for key, off, shape in net.layout:
                st = opt.state.get(og[key])
                if not st:
                    continue
                n = int(np.prod(shape))
                # the fixture tests' absolute floors (1e-8, 1e-12) hold for its gradient scale; without ValueNorm the raw returns
                # make the critic's gradients larger, so the floors scale with the tensor (a 96-term fp32 sum rounds at ~1e-7 of it)
                m1, m2 = st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
                close(pol.exp_avg[lo + off: lo + off + n].view(shape), m1, 1e-4, max(1e-8, 1e-6 * np.abs(m1).max()), f"{what}: {key} exp_avg")
                close(pol.exp_avg_sq[lo + off: lo + off + n].view(shape), m2, 2e-4, max(1e-12, 1e-6 * np.abs(m2).max()), f"{what}: {key} exp_avg_sq")
        if a.use_valuenorm:
            close(tr.value_normalizer.state, ovn.state(), 2e-6, 1e-9, f"{what}: ValueNorm state")


@pytest.mark.gpu
@pytest.mark.parametrize("unfused", [False, True])
@pytest.mark.parametrize("case", [0, 7, 9])
@pytest.mark.parametrize("flip", list(SWEEP))
def test_ppo_update_flag_sweep(M, case, flip, unfused):
    """R_MAPPO.ppo_update on the fixture's H = 64 cases (weights and sample; c9 is the recurrent one, the GRU kernels' only
    fused-loss coverage) with one flag set flipped, against O.ppo_update_ref in float64 on the same inputs: the six
    statistics, the raw gradient, the post-step parameters, the Adam moments and the ValueNorm state."""
    g = golden("ppo_update")
    d = sub(g, f"c{case}")
    T, N, Ma, D, S, A, H = [int(x) for x in d["dims"]]
    fl = dict(zip([str(x) for x in d["flag_names"]], [bool(x) for x in d["flags"]]))
    rec = fl["use_recurrent_policy"]
    hy = d["hyper"]
    kw = dict(episode_length=T, n_rollout_threads=N, hidden_size=H, clip_param=float(hy[0]), entropy_coef=float(hy[1]),
              value_loss_coef=float(hy[2]), huber_delta=float(hy[3]), max_grad_norm=float(hy[4]), lr=float(hy[5]),
              critic_lr=float(hy[6]), opti_eps=float(hy[7]), weight_decay=float(hy[8]), data_chunk_length=int(hy[9]),
              **{k: v for k, v in fl.items() if k not in ("update_actor", "two_steps")})
    kw.update(SWEEP[flip])
    a = make_args(M, unfused_update=unfused, **kw)
    oa = O.default_args(**kw)
    pol, opol = _policy_pair(M, a, oa, D, S, A, state=(g, f"c{case}"))
    sample = [d[f"sample/{nm}"] for nm in TUPLE]
    if flip == "hyper":
        sample[6] = sample[6] * 4.0                                # returns: some normalised targets beyond huber_delta = 1
    # update_actor=False: the fused paths (update kernels, GRU training kernels) do not run the actor at all and report policy
    # loss, entropy and ratio as 0, where the reference still evaluates them (r_mappo.py:109-123); only the unfused MLP path does
    policy_stats = flip != "critic_only" or (unfused and not rec)
    _compare_update(M, a, oa, pol, opol, tuple(sample), d["vn0"], 2 if flip == "two_steps" else 1, flip != "critic_only", rec,
                    f"c{case} {flip}", policy_stats)


@pytest.mark.gpu
@pytest.mark.parametrize("unfused", [False, True])
def test_ppo_update_36_wide_actor(M, unfused):
    """MPE simple_spread with 6 agents: 36-wide observations, 5 actions, layer_N = 1 — an actor whose 16-sample-tile layout
    does not fit the LDS.  R_MAPPO.ppo_update (dual launch by default) against the float64 oracle, two steps."""
    D, S, A, B = 36, 216, 5, 600
    kw = dict(hidden_size=64, lr=7e-4, critic_lr=7e-4)
    a = make_args(M, unfused_update=unfused, **kw)
    oa = O.default_args(**kw)
    pol, opol = _policy_pair(M, a, oa, D, S, A, seed=36)
    rng = np.random.default_rng(36)
    f = np.float32
    avail = (rng.random((B, A)) > 0.3).astype(f)
    actions = rng.integers(0, A, (B, 1)).astype(f)
    avail[np.arange(B), actions[:, 0].astype(int)] = 1.0
    obs, sobs = rng.standard_normal((B, D)).astype(f), rng.standard_normal((B, S)).astype(f)
    with torch.no_grad():
        v_now = opol.critic(torch.from_numpy(sobs).double(), None, None)[0].numpy().astype(f)
    sample = (sobs, obs, np.zeros((B, 1, 64), f), np.zeros((B, 1, 64), f), actions,
              (v_now + rng.standard_normal((B, 1)) * 0.25).astype(f), (rng.standard_normal((B, 1)) * 3).astype(f),
              np.ones((B, 1), f), (rng.random((B, 1)) > 0.2).astype(f), (-np.abs(rng.standard_normal((B, 1))) - 1.0).astype(f),
              rng.standard_normal((B, 1)).astype(f), avail)
    _compare_update(M, a, oa, pol, opol, sample, np.array([0.1, 2.0, 0.5], f), 2, True, False, "36-wide actor")

