"""MultiDiscrete action spaces on the GPU: the mappo_*_md entry points against a float64 restatement of the reference's semantics
(tests/md_ref.py) and a host Philox (tests/rollout_ref.py), and the policy / trainer / runner on top of them.

  1. one head reduces to Discrete, bit for bit (sampling) and within the update bounds (loss);
  2. per-head sampling: head j of row i draws Philox index (j << 32) | i;
  3. the update launches (single and dual) against float64 autograd: every parameter gradient within 1e-4 of its tensor's
     largest entry, statistics within 2e-6 relative, the slab / partial write contract, bit-identical repeats;
  4. MPERunner on SyntheticMPEEnv(action_dims=(5, 10)).
Shapes: B = 53 (a ragged 16-row tile after three full ones; 32-row tiles: one full + ragged), 203 / 643 (several tiles per
wave of a workgroup) and 87."""
import copy

import numpy as np
import pytest
import torch

import md_ref
import rollout_ref as RR
from oracle import mappo_oracle as O
from test_gpu_kernels import close_rel_max, dev, _flat_from_module, _randomize, _relu_margin, _loss_margin

SEED, CTR = 0x1234567887654321, 77


@pytest.fixture(scope="module")
def ops(gpu_device):
    from mappo_amd import ops as _ops
    return _ops


def _nets(ops, D, S, A, LN, relu, fn, seed=3, **flags):
    torch.manual_seed(seed)
    a = O.default_args(use_ReLU=relu, layer_N=LN, use_feature_normalization=fn, **flags)
    actor, critic = O.ActorRef(a, D, A), O.CriticRef(a, S)
    _randomize(actor, D + 3); _randomize(critic, S + 4)
    da, dc = ops.net_desc(D, A, LN, relu, fn), ops.net_desc(S, 1, LN, relu, fn)
    pa, la, Pa = _flat_from_module(ops, actor, da, "act.action_out.linear")
    pc, lc, Pc = _flat_from_module(ops, critic, dc, "v_out")
    return a, actor, critic, da, dc, (pa, la, Pa), (pc, lc, Pc)


def _step(ops, md, pa, da, pc, dc, obs, sobs, heads, det, M=0, insert=None):
    B = obs.shape[0]
    K = len(heads)
    act = torch.full((B, K) if md else (B,), -7.0, device="cuda")
    lp = torch.full_like(act, -7.0)
    val = torch.empty(B, device="cuda")
    if md:
        ops.rollout_step_md(pa, da, pc, dc, (obs, 0, 0), (sobs, 0, 0), M, B, heads, det, SEED, CTR, None, act, lp, val, insert)
    else:
        ops.rollout_step(pa, da, pc, dc, (obs, 0, 0), (sobs, 0, 0), M, B, None, det, SEED, CTR, None, act, lp, val, insert)
    return act, lp, val


# ---- 1. a single head is the Discrete policy, bit for bit ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("det", [False, True])
def test_single_head_equals_discrete(ops, det):
    B, D, S, A = 53, 21, 42, 5
    _, _, _, da, dc, (pa, _, _), (pc, _, _) = _nets(ops, D, S, A, 1, True, True)
    rng = np.random.default_rng(1)
    obs, sobs = dev(rng.standard_normal((B, D))), dev(rng.standard_normal((B, S)))
    a0, l0 = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    a1, l1 = torch.empty(B, 1, device="cuda"), torch.empty(B, 1, device="cuda")
    ops.actor_act(pa, da, obs, None, B, det, SEED, CTR, a0, l0)
    ops.actor_act_md(pa, da, obs, (A,), B, det, SEED, CTR, a1, l1)
    assert torch.equal(a0, a1.view(B)) and torch.equal(l0, l1.view(B))
    s0 = _step(ops, False, pa, da, pc, dc, obs, sobs, (A,), det)
    s1 = _step(ops, True, pa, da, pc, dc, obs, sobs, (A,), det)
    assert torch.equal(s0[0], s1[0].view(B)) and torch.equal(s0[1], s1[1].view(B)) and torch.equal(s0[2], s1[2])
    if not det:
        assert len(set(a0.cpu().numpy().tolist())) > 1


# ---- 2. sampling per head ---------------------------------------------------------------------------------------------------
HEADS = [(5, 10), (3, 3, 3, 3), (2, 14), (16,)]


def _check_heads(z64, z32, heads, actions, logp, det, what):
    """Every head against the host Philox on its float64 logit slice; returns (near pairs, pairs, draws [B, K])."""
    B = z64.shape[0]
    _, tol = RR.err_and_tol(z64, z32)
    near = 0
    us = []
    for j, (lo, hi) in enumerate(md_ref.head_slices(heads)):
        u = RR.uniform24(SEED, CTR, (np.uint64(j) << np.uint64(32)) | np.arange(B, dtype=np.uint64))
        us.append(u)
        exp = RR.expected_argmax(z64[:, lo:hi], None, tol) if det else RR.expected_sample(z64[:, lo:hi], None, u, tol)
        fails = RR.check_actions(exp, None, actions[:, j], logp[:, j], tol, f"{what} head {j}")
        assert not fails, fails
        near += int(exp.near.sum())
    return near, B * len(heads), np.stack(us, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: "x".join(map(str, h)))
@pytest.mark.parametrize("D", [21, 64])
@pytest.mark.parametrize("LN", [0, 1])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "tanh"])
def test_sampling_per_head(ops, heads, D, LN, relu):
    A, S, K = sum(heads), 42, len(heads)
    _, actor, critic, da, dc, (pa, _, _), (pc, _, _) = _nets(ops, D, S, A, LN, relu, True, seed=D + LN)
    rng = np.random.default_rng(D * 7 + A)
    for B, M in ((53, 0), (203, 7)):
        obs = rng.standard_normal((B, D)).astype(np.float32)
        sobs = rng.standard_normal((B, S)).astype(np.float32)
        z64, _ = RR.actor_eval(actor, obs)
        z32, _ = RR.actor_eval(actor, obs, dtype=torch.float32)
        for det in (False, True):
            act = torch.empty(B, K, device="cuda"); lp = torch.empty(B, K, device="cuda")
            ops.actor_act_md(pa, da, dev(obs), heads, B, det, SEED, CTR, act, lp)
            n1, tot, us = _check_heads(z64, z32, heads, act.cpu().numpy(), lp.cpu().numpy(), det, f"act_md B={B} det={det}")
            a2, l2, _ = _step(ops, True, pa, da, pc, dc, dev(obs), dev(sobs), heads, det)
            n2, _, _ = _check_heads(z64, z32, heads, a2.cpu().numpy(), l2.cpu().numpy(), det, f"rollout_step_md B={B} det={det}")
            assert max(n1, n2) <= 0.02 * tot, f"{max(n1, n2)} of {tot} (row, head) pairs near a boundary"
    if M:
        # fused insert: rows read from the env output in place (N threads x M agents), buffer slots equal a separate insert
        N = B // M
        env_obs = dev(rng.standard_normal((N, M, D)))
        rew = dev(rng.standard_normal((N, M)))
        dones = torch.as_tensor(rng.random((N, M)) > 0.5).cuda()
        share = dev(rng.standard_normal((B, S)))
        Sd = M * D

        def slots():
            return (torch.full((B, D), -3.0, device="cuda"), torch.full((B, Sd), -3.0, device="cuda"), torch.full((B,), -3.0, device="cuda"),
                    torch.full((B,), -3.0, device="cuda"))
        o1, s1, r1, m1 = slots()
        ins = dict(obs_dst=o1, share_dst=s1, rewards=(rew, M, 1), dones=(dones, M, 1), rew_dst=r1, mask_dst=m1, centralized=True)
        act = torch.empty(B, K, device="cuda"); lp = torch.empty(B, K, device="cuda"); val = torch.empty(B, device="cuda")
        ops.rollout_step_md(pa, da, pc, dc, (env_obs, M * D, D), (share, M * S, S), M, B, heads, False, SEED, CTR, None, act, lp, val, ins)
        o2, s2, r2, m2 = slots()
        ops.insert_mpe(env_obs, rew, dones, o2, s2, r2, m2, True)
        for x, y in ((o1, o2), (s1, s2), (r1, r2), (m1, m2)):
            assert torch.equal(x, y)
        a3 = torch.empty(B, K, device="cuda"); l3 = torch.empty(B, K, device="cuda")
        ops.actor_act_md(pa, da, env_obs.view(B, D), heads, B, False, SEED, CTR, a3, l3)
        assert (act == a3).float().mean() > 0.98                 # same rows, same draws (two kernel families: boundaries may differ)


@pytest.mark.gpu
def test_heads_draw_different_numbers(ops):
    """Two heads with IDENTICAL logits (head 1's weight rows and biases copied from head 0): a kernel that reused head 0's Philox
    index for head 1 would return the same action for both in every row; with separate draws they differ in most rows."""
    B, D, S, heads = 203, 21, 42, (8, 8)
    _, actor, critic, da, dc, (pa, la, _), (pc, _, _) = _nets(ops, D, S, 16, 1, True, True, seed=4)
    off = {k: o for k, o, _ in la}
    w, b = off["act.action_out.linear.weight"], off["act.action_out.linear.bias"]
    pa[w + 8 * 64: w + 16 * 64] = pa[w: w + 8 * 64]
    pa[b + 8: b + 16] = pa[b: b + 8]
    rng = np.random.default_rng(2)
    obs, sobs = dev(rng.standard_normal((B, D))), dev(rng.standard_normal((B, S)))
    act = torch.empty(B, 2, device="cuda"); lp = torch.empty(B, 2, device="cuda")
    ops.actor_act_md(pa, da, obs, heads, B, False, SEED, CTR, act, lp)
    a2, l2, _ = _step(ops, True, pa, da, pc, dc, obs, sobs, heads, False)
    for a_, l_, what in ((act, lp, "actor_act_md"), (a2, l2, "rollout_step_md")):
        assert len(torch.unique(a_[:, 0])) > 2, what                               # the heads are not degenerate
        assert (a_[:, 0] != a_[:, 1]).any(), f"{what}: both heads returned the same action in all {B} rows"
        same = a_[:, 0] == a_[:, 1]
        assert torch.equal(l_[same, 0], l_[same, 1]), what                          # identical logits: equal actions, equal log-probs
    act_d = torch.empty(B, 2, device="cuda"); lp_d = torch.empty(B, 2, device="cuda")
    ops.actor_act_md(pa, da, obs, heads, B, True, SEED, CTR, act_d, lp_d)
    assert torch.equal(act_d[:, 0], act_d[:, 1])                                    # the argmax needs no draw


# ---- 3. the update launches against float64 autograd --------------------------------------------------------------------------
def _md_inputs(a, actor, critic, rng, n_rows, D, S, heads, relu):
    """Loss inputs at least 1e-4 away from the ReLU / clip / min kinks (the scheme of test_gpu_update_matrix._safe_inputs)."""
    f = np.float32
    K, A = len(heads), sum(heads)
    obs = rng.standard_normal((n_rows, D)).astype(f)
    sobs = rng.standard_normal((n_rows, S)).astype(f)
    actions = np.stack([rng.integers(0, d, n_rows) for d in heads], 1).astype(f)
    old_logp = (-np.abs(rng.standard_normal((n_rows, K))) * 0.3 - np.log(np.asarray(heads, f))).astype(f)
    adv = rng.standard_normal(n_rows).astype(f)
    active = (rng.random(n_rows) > 0.25).astype(f)
    ret = (rng.standard_normal(n_rows) * 3).astype(f)
    noise = (rng.standard_normal(n_rows) * 0.25).astype(f)
    vn = O.ValueNormRef()
    vn.update(ret[:50].reshape(-1, 1))
    ad = copy.deepcopy(actor).double()
    c = a.clip_param
    ones = np.ones((n_rows, A), f)
    for _ in range(20):
        with torch.no_grad():
            v_now = critic(torch.from_numpy(sobs), None, None)[0].numpy().reshape(-1)
            z = ad.act.logits(ad.features(torch.from_numpy(obs).double(), None, None)[0], None)
            lp, _ = md_ref.evaluate_heads(z, heads, torch.from_numpy(actions).double())
        v_old = (v_now + noise).astype(f)
        r = torch.exp(lp - torch.from_numpy(old_logp).double())
        m = torch.minimum((r - (1 - c)).abs(), (r - (1 + c)).abs()).min(1).values.numpy()
        # the critic's kinks: _loss_margin with a ratio of exactly 1 on its (single-head) actor side
        with torch.no_grad():
            lp0 = ad.evaluate_actions(torch.from_numpy(obs).double(), None, torch.zeros(n_rows, 1).double(), None,
                                      torch.from_numpy(ones).double(), torch.from_numpy(active).double().view(-1, 1))[0].numpy().reshape(-1)
        m = np.minimum(m, _loss_margin(a, actor, critic, obs, sobs, np.zeros(n_rows, f), ones, active, lp0.astype(np.float64), v_old, ret, vn))
        if relu:
            m = np.minimum(m, np.minimum(_relu_margin(actor, torch.from_numpy(obs)), _relu_margin(critic, torch.from_numpy(sobs))))
        bad = np.flatnonzero(m < 1e-4)
        if bad.size == 0:
            return obs, sobs, actions, old_logp, adv, active, ret, v_old
        assert bad.size < 0.1 * n_rows
        obs[bad] = rng.standard_normal((bad.size, D))
        sobs[bad] = rng.standard_normal((bad.size, S))
        old_logp[bad] = -np.abs(rng.standard_normal((bad.size, K))) * 0.3 - np.log(np.asarray(heads, f))
        noise[bad] = rng.standard_normal(bad.size) * 0.25
    raise AssertionError("could not draw inputs away from the kinks")


def _md_reference(a, actor, critic, heads, rows, obs, sobs, actions, old_logp, adv, active, v_old, ret, vn):
    ad, cd = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    t = lambda x: torch.from_numpy(x[rows]).double()
    act = t(active).view(-1, 1)
    z = ad.act.logits(ad.features(t(obs), None, None)[0], None)
    pl, ent, ratio, _ = md_ref.policy_terms(z, heads, t(actions), t(old_logp), t(adv).view(-1, 1), act, a.clip_param,
                                            a.use_policy_active_masks)
    vals = cd(t(sobs), None, None)[0]
    ret_t = t(ret).view(-1, 1)
    tgt = vn.normalize(ret_t.float()).double() if a.use_valuenorm else ret_t
    dummy = torch.zeros_like(ret_t)
    _, vl, _ = O.ppo_losses_ref(a, dummy, dummy.sum(), vals, dummy, t(adv).view(-1, 1), act, t(v_old).view(-1, 1), tgt)
    (pl - a.entropy_coef * ent).backward()
    (vl * a.value_loss_coef).backward()
    ga = {k: p.grad.numpy() for k, p in ad.named_parameters() if p.grad is not None}
    gc = {k: p.grad.numpy() for k, p in cd.named_parameters() if p.grad is not None}
    return [vl.item(), pl.item(), ent.item(), ratio.item()], ga, gc


def _check_layout(g, layout, col0, ref, what):
    for key, off, shape in layout:
        n = int(np.prod(shape))
        close_rel_max(g[col0 + off: col0 + off + n].reshape(shape), ref[key], 1e-4, f"{what}: {key}")


def _run_updates(ops, a, nets, heads, B, with_rows, rng, relu, nan_check=True, repeats=0):
    _, actor, critic, da, dc, (pa, la, Pa), (pc, lc, Pc) = nets
    D, S = da.in_dim, dc.in_dim
    n_rows = B + 64 if with_rows else B
    rows = rng.permutation(n_rows)[:B].astype(np.int32) if with_rows else np.arange(B, dtype=np.int32)
    obs, sobs, actions, old_logp, adv, active, ret, v_old = _md_inputs(a, actor, critic, rng, n_rows, D, S, heads, relu)
    vn = O.ValueNormRef(); vn.update(ret[:50].reshape(-1, 1)); vn.update(ret[rows].reshape(-1, 1))
    ref_stats, ga, gc = _md_reference(a, actor, critic, heads, rows.astype(np.int64), obs, sobs, actions, old_logp, adv, active, v_old, ret, vn)
    d_rows = dev(rows, torch.int32) if with_rows else None
    g = dict(obs=dev(obs), sobs=dev(sobs), actions=dev(actions), old=dev(old_logp), adv=dev(adv), active=dev(active), ret=dev(ret),
             vold=dev(v_old), vn=dev(vn.state()))
    mom = torch.zeros(4, dtype=torch.float64, device="cuda")
    ops.minibatch_moments(g["ret"], g["active"], d_rows, B, mom)
    cfg = ops.ppo_cfg(a)
    col_c = ((Pa + 255) // 256) * 256
    P = col_c + ((Pc + 255) // 256) * 256 + 256
    nanf = float("nan")
    npart = ops.update_partials("cuda").numel()

    def stats_of(p_a, n_a, p_c, n_c):
        st = torch.zeros(6, dtype=torch.float64, device="cuda")
        ops.update_stats(p_a, n_a, p_c, n_c, mom, cfg, st)
        return st.cpu().numpy()

    def check_stats(st, what):
        for i, name in enumerate(("value_loss", "policy_loss", "dist_entropy", "ratio")):
            print(f"{what}: {name} {st[i]!r} vs {ref_stats[i]!r} (rel {abs(st[i] - ref_stats[i]) / max(abs(ref_stats[i]), 1e-300):.2e})")
            assert abs(st[i] - ref_stats[i]) <= 2e-6 * abs(ref_stats[i]) + 1e-8, f"{what}: {name} {st[i]!r} vs {ref_stats[i]!r}"

    # single launch (actor md + the critic's own launch), NaN-filled: rows / columns outside the promise stay NaN
    ns = ops.mlp_backward_slabs(B)
    slabs = torch.full((ns + 3, P), nanf, device="cuda")
    p_a = torch.full((npart,), nanf, dtype=torch.float64, device="cuda")
    p_c = torch.full((npart,), nanf, dtype=torch.float64, device="cuda")
    ops.actor_update_md(pa, da, g["obs"], d_rows, B, heads, g["actions"], g["old"], g["adv"], g["active"], mom, cfg, slabs, P, 0, p_a)
    ops.critic_update(pc, dc, g["sobs"], d_rows, B, g["vold"], g["ret"], g["active"], g["vn"], mom, cfg, slabs, P, col_c, p_c)
    s = slabs.cpu().numpy()
    owned = np.zeros(s.shape, bool)
    owned[:ns, :Pa] = True; owned[:ns, col_c:col_c + Pc] = True
    assert np.isfinite(s[owned]).all(), "single: a promised slab entry was not written"
    assert np.isnan(s[~owned]).all(), "single: wrote outside its rows / columns"
    pav = p_a.view(-1, 4).cpu().numpy()
    assert np.isfinite(pav[:ns]).all() and np.isnan(pav[ns:]).all(), "single: loss partials are not exactly the promised rows"
    gsum = np.where(owned, s, 0.0).astype(np.float64).sum(0)
    _check_layout(gsum, la, 0, ga, "actor_update_md")
    check_stats(stats_of(p_a, ns, p_c, ns), "actor_update_md")

    # dual launch
    nd = ops.dual_update_slabs(da, dc, B)
    outs = []
    for rep in range(1 + repeats):
        slabs = torch.full((nd + 3, P), nanf, device="cuda")
        p_a = torch.full((npart,), nanf, dtype=torch.float64, device="cuda")
        p_c = torch.full((npart,), nanf, dtype=torch.float64, device="cuda")
        ops.actor_critic_update_md(pa, da, g["obs"], pc, dc, g["sobs"], d_rows, B, heads, g["actions"], g["old"], g["adv"], g["active"],
                                   g["vold"], g["ret"], g["vn"], mom, cfg, slabs, P, 0, col_c, p_a, p_c)
        outs.append((slabs, p_a, p_c))
    slabs, p_a, p_c = outs[0]
    for s2, a2, c2 in outs[1:]:
        assert torch.equal(slabs[:nd].nan_to_num(0.0), s2[:nd].nan_to_num(0.0)) and torch.equal(p_a[:4 * nd], a2[:4 * nd]) and \
            torch.equal(p_c[:4 * nd], c2[:4 * nd]), "the dual launch is not deterministic"
    s = slabs.cpu().numpy()
    owned = np.zeros(s.shape, bool)
    owned[:nd, :Pa] = True; owned[:nd, col_c:col_c + Pc] = True
    assert np.isfinite(s[owned]).all(), "dual: a promised slab entry was not written"
    assert np.isnan(s[~owned]).all(), "dual: wrote outside its rows / columns"
    for p in (p_a, p_c):
        pv = p.view(-1, 4).cpu().numpy()
        assert np.isfinite(pv[:nd]).all() and np.isnan(pv[nd:]).all(), "dual: loss partials are not exactly the promised rows"
    gsum = np.where(owned, s, 0.0).astype(np.float64).sum(0)
    _check_layout(gsum, la, 0, ga, "actor_critic_update_md actor")
    _check_layout(gsum, lc, col_c, gc, "actor_critic_update_md critic")
    check_stats(stats_of(p_a, nd, p_c, nd), "actor_critic_update_md")
    return g, mom, cfg, d_rows, (col_c, P)


UPD_SHAPES = [(21, 42, (5, 10)), (18, 54, (3, 3, 3, 3)), (64, 64, (2, 14)), (21, 42, (16,))]
# (shape, layer_N, B) crossed in full; feature norm, the policy's active masks and the minibatch form alternate so that every
# shape and every layer_N meets both values of each
UPD_CASES = [(i, LN, B, (i + LN + k) % 2 == 0, (i + k) % 2 == 0, (LN + k) % 2 == 0)
             for i in (0, 1, 3) for LN in (0, 1) for k, B in enumerate((87, 16 * 40 + 3))]
# the 64-input actor in full: with layer_N 1 it has a backward-data product of its own (no transposed W2' copy)
UPD_CASES += [(2, LN, B, fn, pm, wr) for LN in (0, 1) for B in (87, 16 * 40 + 3) for fn in (False, True) for pm in (False, True)
              for wr in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,LN,B,fn,pmask,with_rows", UPD_CASES)
def test_update_vs_float64_autograd(ops, shape, LN, B, fn, pmask, with_rows):
    D, S, heads = UPD_SHAPES[shape]
    relu = (shape + LN) % 2 == 0
    nets = _nets(ops, D, S, sum(heads), LN, relu, fn, seed=B + D, use_policy_active_masks=pmask)
    _run_updates(ops, nets[0], nets, heads, B, with_rows, np.random.default_rng(B * 7 + D + LN), relu, repeats=9 if B == 87 else 0)


# ---- 4. one head: the md update agrees with mappo_actor_update -------------------------------------------------------------
@pytest.mark.gpu
def test_single_head_update_matches_discrete(ops):
    D, S, heads, B = 21, 42, (5,), 643
    nets = _nets(ops, D, S, 5, 1, True, True, seed=11)
    a, _, _, da, dc, (pa, la, Pa), _ = nets
    g, mom, cfg, d_rows, (col_c, P) = _run_updates(ops, a, nets, heads, B, True, np.random.default_rng(5), True)
    ns = ops.mlp_backward_slabs(B)
    out = []
    for md in (False, True):
        slabs = torch.zeros(ns, P, device="cuda")
        p_a = torch.zeros(ops.update_partials("cuda").numel(), dtype=torch.float64, device="cuda")
        if md:
            ops.actor_update_md(pa, da, g["obs"], d_rows, B, heads, g["actions"], g["old"], g["adv"], g["active"], mom, cfg, slabs, P, 0, p_a)
        else:
            ops.actor_update(pa, da, g["obs"], d_rows, B, None, g["actions"].view(-1), g["old"].view(-1), g["adv"], g["active"], mom, cfg,
                             slabs, P, 0, p_a)
        out.append((slabs.double().sum(0).cpu().numpy(), p_a.view(-1, 4)[:ns].sum(0).cpu().numpy()))
    for key, off, shape in la:
        n = int(np.prod(shape))
        close_rel_max(out[1][0][off:off + n], out[0][0][off:off + n], 1e-4, f"K = 1 vs Discrete: {key}")
    for k in range(3):
        assert abs(out[1][1][k] - out[0][1][k]) <= 2e-6 * abs(out[0][1][k]) + 1e-8, (k, out[1][1], out[0][1])


# ---- 5. policy, trainer and runner ----------------------------------------------------------------------------------------
def _runner(action_dims, graph, N=8, M=2, D=21, T=5):
    from mappo_amd.config import get_config
    from mappo_amd.envs.synthetic import SyntheticMPEEnv
    from mappo_amd.runner.shared.mpe_runner import MPERunner
    d = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.use_hip_graph, a.ppo_epoch = graph, 2
    torch.manual_seed(1)
    env = SyntheticMPEEnv(N, M, D, episode_length=T, seed=1, device=d, action_dims=action_dims)
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=M, device=d, run_dir=None))
    gen = torch.Generator(device=d).manual_seed(7)
    fp = r.policy.flat_params
    fp.add_(torch.randn(fp.shape, device=d, generator=gen) * 0.1)
    r.warmup()
    return r, env


def _oracle_actor(pol, D, heads):
    """The policy's actor as an oracle ActorRef: the heads' weight rows / biases side by side are ONE linear layer of sum d_j rows."""
    A = sum(heads)
    net = O.ActorRef(O.default_args(), D, A)
    sd = {k: v.detach().cpu() for k, v in pol.actor.state_dict().items()}
    sd["act.action_out.linear.weight"] = torch.cat([sd.pop(f"act.action_outs.{j}.linear.weight") for j in range(len(heads))], 0)
    sd["act.action_out.linear.bias"] = torch.cat([sd.pop(f"act.action_outs.{j}.linear.bias") for j in range(len(heads))], 0)
    net.load_state_dict(sd)
    return net


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_runner_multidiscrete(ops, graph):
    """graph: the third rollout is the REPLAY of the episode captured during the second (collect_step_fused -> rollout_step_md
    under capture, the device counter word bumped per replay): its buffer is checked like the eager one."""
    from mappo_amd.runner.shared.mpe_runner import onehot_actions
    heads = (5, 10)
    r, env = _runner(heads, graph=graph)
    pol, b = r.policy, r.buffer
    assert env.action_space[0].__class__.__name__ == "MultiDiscrete" and pol.actor.head_dims == heads
    keys = list(pol.actor.state_dict().keys())
    assert keys[-4:] == ["act.action_outs.0.linear.weight", "act.action_outs.0.linear.bias", "act.action_outs.1.linear.weight",
                         "act.action_outs.1.linear.bias"]
    assert tuple(pol.actor.state_dict()["act.action_outs.1.linear.weight"].shape) == (10, 64)
    assert not pol.can_fuse_episode() and pol.can_fuse_step()
    assert tuple(b.actions.shape) == (5, 8, 2, 2) and b.available_actions is None
    for it in range(2):
        info, _ = r.run_episode(it, 2)
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in info.values()), info
        if it == 0:
            continue
    # the buffer after the second rollout (train() has moved the parameters since: recompute with a fresh rollout)
    prev_actions, prev_obs = b.actions.clone(), b.obs.clone()
    r.rollout()
    torch.cuda.synchronize()
    if graph:
        assert isinstance(r._rollout_graph, torch.cuda.CUDAGraph)
        assert not torch.equal(b.obs, prev_obs) and not torch.equal(b.actions, prev_actions)      # a fresh episode, fresh draws
    acts = b.actions.cpu().numpy()
    assert (acts == np.round(acts)).all()
    for j, d in enumerate(heads):
        assert acts[..., j].min() >= 0 and acts[..., j].max() < d
    assert len(np.unique(acts[..., 1])) > 3
    T, R = b.episode_length, b.n_rollout_threads * b.num_agents
    h0 = torch.zeros(T * R, 1, 64, device="cuda")
    m1 = torch.ones(T * R, 1, device="cuda")
    vals, lp, ent = pol.evaluate_actions(b.share_obs[:T].reshape(T * R, -1), b.obs[:T].reshape(T * R, -1), h0, h0,
                                         b.actions.reshape(T * R, -1), m1, None, b.active_masks[:T].reshape(T * R, 1))
    # the sampling tolerance (rollout_ref.err_and_tol on this policy's logits): both the buffer's log-probs (rollout kernel) and
    # evaluate_actions' (forward kernel + torch) against the float64 log-probs of the buffer's actions
    net = _oracle_actor(pol, 21, heads)
    obs_np = b.obs[:T].reshape(T * R, -1).cpu().numpy()
    z64, _ = RR.actor_eval(net, obs_np)
    z32, _ = RR.actor_eval(net, obs_np, dtype=torch.float32)
    _, tol = RR.err_and_tol(z64, z32)
    lp64, _ = md_ref.evaluate_heads(torch.from_numpy(z64), heads, b.actions.reshape(T * R, -1).cpu().double())
    e_buf = (b.action_log_probs.view(T * R, -1).cpu().double() - lp64).abs().max().item()
    e_eval = (lp.cpu().double() - lp64).abs().max().item()
    print(f"runner log-probs: buffer off by {e_buf:.2e}, evaluate_actions by {e_eval:.2e}, tol {tol:.2e}")
    assert e_buf <= tol and e_eval <= tol
    assert tuple(lp.shape) == (T * R, 2) and ent.dim() == 0 and torch.isfinite(ent)
    oh = onehot_actions(b.actions[0], env.action_space[0])
    assert tuple(oh.shape) == (8, 2, 15) and (oh.sum(-1) == 2).all()
    a0 = b.actions[0].long()
    assert (oh[..., :5].argmax(-1) == a0[..., 0]).all() and (oh[..., 5:].argmax(-1) == a0[..., 1]).all()
    env.consumes_actions = True
    try:
        assert torch.equal(r._actions_env(b.actions[0]), oh)
    finally:
        del env.consumes_actions
    act, _ = pol.act(b.obs[0].reshape(R, -1), h0[:R], m1[:R], deterministic=True)
    assert tuple(act.shape) == (R, 2) and act.dtype == torch.int64


@pytest.mark.gpu
def test_train_graph_replay_equals_eager(ops):
    """train() on a MultiDiscrete buffer: the hipGraph replay (third call) reproduces the eager pass bit for bit."""
    outs = []
    for graph in (False, True):
        r, _ = _runner((5, 10), graph=graph)
        r._use_graph = False                       # the rollout stays eager on both sides: the same buffers
        for _ in range(3):
            r.rollout()
            r.trainer.train(r.buffer, after_update=True)
        torch.cuda.synchronize()
        if graph:
            assert any(isinstance(g, torch.cuda.CUDAGraph) for g in r.trainer._graphs.values())
        outs.append(r.policy.flat_params.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
def test_discrete_runner_keeps_its_path(ops):
    r, env = _runner(None, graph=False)
    assert env.action_space[0].__class__.__name__ == "Discrete" and r.policy.actor.head_dims is None
    assert r.policy.can_fuse_episode() and r.policy.can_fuse_step()
    info, _ = r.run_episode(0, 1)
    assert tuple(r.buffer.actions.shape) == (5, 8, 2, 1) and all(np.isfinite(v) for v in info.values())


@pytest.mark.gpu
def test_separated_runner_and_data_parallel_refuse_the_space(ops):
    from mappo_amd.config import get_config
    from mappo_amd.envs.synthetic import SyntheticMPEEnv
    from mappo_amd.runner.separated.mpe_runner import MPERunner as SeparatedRunner
    from mappo_amd.algorithms.r_mappo.r_mappo import R_MAPPO
    d = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.env_name, a.share_policy, a.use_hip_graph = 5, 4, "MPE", False, False
    env = SyntheticMPEEnv(4, 2, 21, episode_length=5, seed=1, device=d, action_dims=(5, 10))
    with pytest.raises(NotImplementedError, match="MultiDiscrete.*separated"):
        SeparatedRunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=2, device=d, run_dir=None))
    r, _ = _runner((5, 10), graph=False)
    with pytest.raises(NotImplementedError, match="MultiDiscrete.*data-parallel"):
        R_MAPPO(r.all_args, r.policy, device=d, dist_group=object())
    r.all_args.unfused_update = True
    vn_before = r.trainer.value_normalizer.state.clone()
    with pytest.raises(NotImplementedError, match="unfused_update"):
        R_MAPPO(r.all_args, r.policy, device=d)
    assert torch.equal(r.trainer.value_normalizer.state, vn_before)


# ---- 6. the fixture generated from the reference (tests/golden/generate_golden_multidiscrete.py) ---------------------------
def _golden_setup(case, graph):
    from conftest import golden, sub
    from mappo_amd.config import get_config
    from mappo_amd.utils.shared_buffer import SharedReplayBuffer
    from mappo_amd.utils.util import MultiDiscrete
    from mappo_amd.algorithms.r_mappo.r_mappo import R_MAPPO
    from mappo_amd.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    from test_gpu_e2e import set_vn
    g = golden("multidiscrete")
    d = sub(g, f"c{case}")
    T, N, M, D, S, H, seed = [int(x) for x in d["dims"][:7]]
    heads = tuple(int(x) for x in d["dims"][7:])
    hy = d["hyper"]
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.ppo_epoch, a.num_mini_batch, a.layer_N = T, N, 1, 1, 1
    a.lr, a.critic_lr, a.use_hip_graph, a.perm_device = float(hy[5]), float(hy[6]), graph, "cpu"
    space = MultiDiscrete([[0, h - 1] for h in heads])
    pol = R_MAPPOPolicy(a, [D], [S], space)
    pol.actor.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sub(g, f"c{case}/actor0").items()})
    pol.critic.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sub(g, f"c{case}/critic0").items()})
    tr = R_MAPPO(a, pol)
    set_vn(tr, d["vn0"])
    buf = SharedReplayBuffer(a, M, [D], [S], space)
    assert buf.available_actions is None
    for n in ("share_obs", "obs", "rnn_states", "rnn_states_critic", "value_preds", "returns", "actions", "action_log_probs", "rewards",
              "masks", "bad_masks", "active_masks"):
        getattr(buf, n).copy_(torch.from_numpy(np.ascontiguousarray(d["buf/" + n])))
    return g, d, a, pol, tr, buf, heads


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1])
def test_golden_ppo_update(ops, case):
    """One R_MAPPO.ppo_update on the reference's minibatch: its six return values within 2e-6 relative and the gradient of every
    parameter within 1e-4 of the tensor's largest entry (the fixture's gradient norms are below max_grad_norm: unclipped)."""
    from conftest import sub
    from test_gpu_e2e import TUPLE, close
    g, d, a, pol, tr, buf, heads = _golden_setup(case, False)
    sample = tuple(d.get(f"sample/{nm}") for nm in TUPLE)
    assert sample[-1] is None
    out = tr.ppo_update(sample, True)
    print("ppo_update stats", np.array(out, dtype=np.float64), "reference", d["upd/stats"])
    close(np.array(out, dtype=np.float64), d["upd/stats"], 2e-6, 1e-8, f"case {case} stats")
    for tag, net, seg in (("actor", pol.actor, 0), ("critic", pol.critic, 1)):
        ref = sub(g, f"c{case}/upd/{tag}_grad")
        lo = pol.seg_bounds[seg]
        seen = 0
        for key, off, shape in net.layout:
            sd_key = key
            if key.startswith("act.action_out.linear."):                       # the one head matrix = the heads' rows side by side
                kind = key.rsplit(".", 1)[1]
                want = np.concatenate([ref[f"act.action_outs.{j}.linear.{kind}"] for j in range(len(heads))], 0)
                seen += len(heads)
            else:
                want = ref[sd_key]
                seen += 1
            n = int(np.prod(shape))
            close_rel_max(pol.flat_grad[lo + off: lo + off + n].view(shape), want, 1e-4, f"case {case} {tag} {key}")
        assert seen == len(ref), (seen, sorted(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1])
def test_golden_train_and_graph_replay(ops, case):
    """R_MAPPO.train on the reference's buffer: train_info and the state dicts after it (rtol 1e-5, atol 3e-6); then the captured
    graph: the third train() of a graph trainer (a replay) leaves the parameters of three eager train() calls, bit for bit."""
    from conftest import sub
    from test_gpu_e2e import close
    g, d, a, pol, tr, buf, heads = _golden_setup(case, False)
    torch.manual_seed(3000 + int(d["dims"][6]))
    info = tr.train(buf)
    ref = dict(zip([str(k) for k in d["train/info_keys"]], d["train/info"]))
    print("train info", info, "reference", ref)
    # train_info: 2e-6 relative, plus one float32 ulp at magnitude 1 (2^-23 = 1.2e-7) absolute.  The reference's policy_loss is a
    # float32 mean of signed terms min(r adv, clip(r) adv) of magnitude ~1 that cancel to ~1e-2 (7.7e-3 in case 1): the reference's
    # own rounding of the partial sums is of that absolute size, whatever the size of the result.
    for k, v in info.items():
        close(v, ref[k], 2e-6, 2.0 ** -23, k)
    for tag, net in (("actor", pol.actor), ("critic", pol.critic)):
        ref_sd = sub(g, f"c{case}/train/{tag}")
        assert list(net.state_dict().keys()) == list(ref_sd.keys()) or set(net.state_dict().keys()) == set(ref_sd.keys())
        for k, v in net.state_dict().items():
            close(v, ref_sd[k], 1e-5, 3e-6, f"{tag} {k}")
    close(tr.value_normalizer.state, d["train/vn"], 2e-6, 1e-9)
    tr.train(buf); tr.train(buf)
    torch.cuda.synchronize()
    _, _, _, pol_g, tr_g, buf_g, _ = _golden_setup(case, True)
    for _ in range(3):
        tr_g.train(buf_g)
    torch.cuda.synchronize()
    assert any(isinstance(x, torch.cuda.CUDAGraph) for x in tr_g._graphs.values())
    assert torch.equal(pol.flat_params, pol_g.flat_params)
    assert torch.equal(tr.value_normalizer.state, tr_g.value_normalizer.state)
