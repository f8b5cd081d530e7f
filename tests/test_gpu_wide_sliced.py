"""in_dim 513..2048 on the GPU: layer 1 in K slices (mlp_wide_sliced.h) behind mappo_mlp_forward, mappo_actor_act,
mappo_actor_update / mappo_critic_update (+ mappo_wide_l1_backward), mappo_mlp_features and mappo_trunk_backward, against float64
evaluations of the oracle's networks; and the widths up to 512 bit-equal to what the library computed before the limit moved.

Tolerances.  Forward: 4 x (the same module evaluated by torch-CPU in float32 vs float64) + 2e-6 (rollout_ref.err_and_tol), worked
out per case.  Update: the bounds of the D = 512 cases of test_gpu_update_matrix.py (gradients 1e-4 of the largest entry of each
parameter, statistics rtol 1e-5 / atol 1e-7)."""
import copy
import os

import numpy as np
import pytest
import torch

import rollout_ref as RR
from oracle import mappo_oracle as O
from test_gpu_kernels import close, close_rel_max, dev, _flat_from_module, _randomize
from test_wide_sliced import UPDATE_CASES, update_inputs

pytestmark = pytest.mark.gpu

WIDTHS = [513, 576, 1000, 1024, 2048]        # one column past the tuned kernels, one full extra chunk, a ragged last chunk, two slices, the maximum
BATCHES = [1, 16, 17, 48]
A = 5


@pytest.fixture(scope="module")
def ops(gpu_device):
    from mappo_amd import ops as _ops
    return _ops


_nets = {}


def _net(ops, D, relu, LN, fn, actor):
    """(oracle module, descriptor, flat device parameters), built once per shape."""
    key = (D, relu, LN, fn, actor)
    if key not in _nets:
        torch.manual_seed(D * 10 + LN)
        a = O.default_args(use_ReLU=relu, layer_N=LN, use_feature_normalization=fn)
        net = O.ActorRef(a, D, A) if actor else O.CriticRef(a, D)
        _randomize(net, D + (3 if actor else 4))
        desc = ops.net_desc(D, A if actor else 1, LN, relu, fn)
        params, _, _ = _flat_from_module(ops, net, desc, "act.action_out.linear" if actor else "v_out")
        _nets[key] = (net, desc, params)
    return _nets[key]


@pytest.mark.parametrize("fn", [True, False], ids=["fn", "nofn"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "tanh"])
@pytest.mark.parametrize("LN", [0, 1])
@pytest.mark.parametrize("D", WIDTHS)
def test_forward_vs_float64(ops, D, LN, relu, fn):
    """Actor logits and critic values of mappo_mlp_forward at every batch size, with and without a row gather."""
    actor, da, pa = _net(ops, D, relu, LN, fn, True)
    critic, dc, pc = _net(ops, D, relu, LN, fn, False)
    rng = np.random.default_rng(D + LN)
    n_rows = max(BATCHES) + 9
    x = (rng.standard_normal((n_rows, D)) * 1.5 + 0.25).astype(np.float32)
    xd = dev(x)
    z64, _ = RR.actor_eval(actor, x)
    z32, _ = RR.actor_eval(actor, x, dtype=torch.float32)
    v64, _ = RR.critic_eval(critic, x)
    v32, _ = RR.critic_eval(critic, x, dtype=torch.float32)
    (ez, tz), (ev, tv) = RR.err_and_tol(z64, z32), RR.err_and_tol(v64, v32)
    for B in BATCHES:
        for with_rows in (False, True):
            rows = rng.permutation(n_rows)[:B].astype(np.int32) if with_rows else np.arange(B, dtype=np.int32)
            dr = dev(rows, torch.int32) if with_rows else None
            logits = torch.full((B + 1, A), float("nan"), device="cuda")
            values = torch.full((B + 1,), float("nan"), device="cuda")
            ops.mlp_forward(pa, da, xd, dr, B, logits)
            ops.mlp_forward(pc, dc, xd, dr, B, values)
            lg, vl = logits.cpu().numpy().astype(np.float64), values.cpu().numpy().astype(np.float64)
            assert np.isnan(lg[B]).all() and np.isnan(vl[B]), "wrote beyond the batch"
            errz, errv = np.abs(lg[:B] - z64[rows]).max(), np.abs(vl[:B] - v64[rows]).max()
            print(f"D={D} LN={LN} relu={relu} fn={fn} B={B} rows={with_rows}: logits err {errz:.2e} (fp32 CPU {ez:.2e}), values err {errv:.2e} (fp32 CPU {ev:.2e})")
            assert errz <= tz, f"logits B={B} rows={with_rows}: {errz:.3e} > {tz:.3e}"
            assert errv <= tv, f"values B={B} rows={with_rows}: {errv:.3e} > {tv:.3e}"


@pytest.mark.parametrize("D", WIDTHS)
def test_actor_act_argmax_and_philox_sampling(ops, D):
    """mappo_actor_act: deterministic = argmax of the float64 logits wherever the top-two gap exceeds 1e-4; sampled actions follow
    the Philox contract (row i draws uniform24(seed, counter, i), inverse CDF over the available actions)."""
    actor, da, pa = _net(ops, D, True, 1, True, True)
    rng = np.random.default_rng(D + 77)
    seed, counter = 0x1234ABCD5678, 41
    for B in BATCHES:
        x = (rng.standard_normal((B, D)) * 1.5).astype(np.float32)
        avail = (rng.random((B, A)) > 0.3).astype(np.float32)
        avail[np.arange(B), rng.integers(0, A, B)] = 1.0
        z64, _ = RR.actor_eval(actor, x, avail)
        z32, _ = RR.actor_eval(actor, x, avail, dtype=torch.float32)
        _, tol = RR.err_and_tol(np.where(avail > 0, z64, 0.0), np.where(avail > 0, z32, 0.0))
        for det in (True, False):
            actions = torch.full((B,), float("nan"), device="cuda")
            logp = torch.full((B,), float("nan"), device="cuda")
            ops.actor_act(pa, da, dev(x), dev(avail), B, det, seed, counter, actions, logp)
            if det:
                exp = RR.expected_argmax(z64, avail, 5e-5)                    # near a boundary: top-two gap < 1e-4
            else:
                exp = RR.expected_sample(z64, avail, RR.uniform24(seed, counter, np.arange(B)), tol)
            fails = RR.check_actions(exp, avail, actions.cpu().numpy(), logp.cpu().numpy(), max(tol, 1e-5), f"D={D} B={B} det={det}")
            assert not fails, fails


def _reference(c):
    """float64 autograd: (value_loss, policy_loss, entropy, ratio mean) and every parameter's gradient of both networks."""
    a = c["a"]
    ad, cd = copy.deepcopy(c["actor"]).double(), copy.deepcopy(c["critic"]).double()
    rows = c["rows"].astype(np.int64)
    t = lambda x: torch.from_numpy(x[rows]).double()
    act = t(c["active"]).view(-1, 1)
    lp, ent, _ = ad.evaluate_actions(t(c["obs"]), None, t(c["actions"]).view(-1, 1), None, t(c["avail"]), act)
    vals = cd(t(c["sobs"]), None, None)[0]
    ret_t = t(c["ret"]).view(-1, 1)
    tgt = c["vn"].normalize(ret_t.float()).double()
    pl, vl, imp = O.ppo_losses_ref(a, lp, ent, vals, t(c["old_logp"]).view(-1, 1), t(c["adv"]).view(-1, 1), act, t(c["v_old"]).view(-1, 1), tgt)
    (pl - a.entropy_coef * ent).backward()
    (vl * a.value_loss_coef).backward()
    ga = {k: p.grad.numpy() for k, p in ad.named_parameters() if p.grad is not None}
    gc = {k: p.grad.numpy() for k, p in cd.named_parameters() if p.grad is not None}
    return [vl.item(), pl.item(), ent.item(), imp.mean().item()], ga, gc


@pytest.mark.parametrize("with_rows", [False, True], ids=["ungathered", "gathered"])
@pytest.mark.parametrize("D,B,LN", UPDATE_CASES)
def test_update_vs_float64_autograd(ops, D, B, LN, with_rows):
    """mappo_actor_update / mappo_critic_update (+ mappo_wide_l1_backward) with NaN-filled slabs and loss partials: every
    parameter's gradient, the loss partials, and the write contract (nothing outside the network's columns or beyond the announced
    rows)."""
    c = update_inputs(D, B, with_rows, LN=LN)
    a = c["a"]
    assert c["near"].sum() <= 0.1 * B
    da, dc = ops.net_desc(D, c["A"], LN, True, True), ops.net_desc(D, 1, LN, True, True)
    pa, la, Pa = _flat_from_module(ops, c["actor"], da, "act.action_out.linear")
    pc, lc, Pc = _flat_from_module(ops, c["critic"], dc, "v_out")
    ref_stats, ga, gc = _reference(c)
    d_rows = dev(c["rows"], torch.int32) if with_rows else None
    g = {k: dev(c[k]) for k in ("obs", "sobs", "avail", "actions", "old_logp", "adv", "active", "ret", "v_old")}
    vn = dev(c["vn"].state())
    mom = torch.zeros(4, dtype=torch.float64, device="cuda")
    ops.minibatch_moments(g["ret"], g["active"], d_rows, B, mom)
    cfg = ops.ppo_cfg(a)
    ns = ops.mlp_backward_slabs(B)
    assert ops.wide_l1_slabs(B) == ns
    col_c = ((Pa + 255) // 256) * 256
    P = col_c + ((Pc + 255) // 256) * 256 + 256                 # a spare 256 columns after the critic's range: must stay untouched
    nanf = float("nan")
    slabs = torch.full((ns + 2, P), nanf, device="cuda")
    n_part = ops.update_partials("cuda").numel()
    part_a = torch.full((n_part,), nanf, dtype=torch.float64, device="cuda")
    part_c = torch.full((n_part,), nanf, dtype=torch.float64, device="cuda")
    ops.actor_update(pa, da, g["obs"], d_rows, B, g["avail"], g["actions"], g["old_logp"], g["adv"], g["active"], mom, cfg, slabs, P, 0, part_a)
    ops.critic_update(pc, dc, g["sobs"], d_rows, B, g["v_old"], g["ret"], g["active"], vn, mom, cfg, slabs, P, col_c, part_c)
    torch.cuda.synchronize()
    s = slabs.cpu().numpy()
    owned = np.zeros(s.shape, dtype=bool)
    owned[:ns, 0:Pa] = True
    owned[:ns, col_c:col_c + Pc] = True
    assert np.isfinite(s[owned]).all(), "a promised slab entry was not written"
    assert np.isnan(s[~owned]).all(), "wrote outside its rows / columns"
    for p in (part_a, part_c):
        pn = p.view(-1, 4).cpu().numpy()
        assert np.isfinite(pn[:ns]).all() and np.isnan(pn[ns:]).all(), "loss partial rows"
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    ops.update_stats(part_a, ns, part_c, ns, mom, cfg, stats)
    grad = torch.zeros(P, device="cuda")
    ops.slab_reduce(slabs[:ns].contiguous(), ns, P, P, grad)
    gf = grad.cpu().numpy()
    print(f"D={D} B={B} rows={with_rows}: stats {stats.cpu().numpy()[:4]} vs {ref_stats}")
    close(stats.cpu().numpy()[:4], ref_stats, 1e-5, 1e-7, "stats vs float64 autograd")
    worst = 0.0
    for lay, col0, gr, who in ((la, 0, ga, "actor"), (lc, col_c, gc, "critic")):
        for key, off, shape in lay:
            got = gf[col0 + off: col0 + off + int(np.prod(shape))].reshape(shape).astype(np.float64)
            err = np.abs(got - gr[key]).max() / max(np.abs(gr[key]).max(), 1e-12)
            worst = max(worst, err)
            print(f"  {who} {key}: max err / max|ref| = {err:.2e}")
    print(f"  worst {worst:.2e}")
    for lay, col0, gr, who in ((la, 0, ga, "actor"), (lc, col_c, gc, "critic")):
        for key, off, shape in lay:
            close_rel_max(gf[col0 + off: col0 + off + int(np.prod(shape))].reshape(shape), gr[key], 1e-4, f"{who} {key}")


def test_recurrent_features_and_trunk_backward(ops):
    """A recurrent critic's trunk at D = 600 through the feature-major forms (L = 3 steps of Nc = 17 sequences, gathered rows):
    mappo_mlp_features against the float64 trunk, mappo_trunk_backward (+ mappo_wide_l1_backward) against float64 autograd."""
    D, L, Nc = 600, 3, 17
    B = L * Nc
    torch.manual_seed(D)
    a = O.default_args(use_recurrent_policy=True, use_ReLU=True, layer_N=1)
    net = O.CriticRef(a, D)
    _randomize(net, D + 3)
    desc = ops.net_desc(D, 1, 1, True, True, recurrent=True)
    params, layout, Pn = _flat_from_module(ops, net, desc, "v_out")
    rng = np.random.default_rng(D)
    n_rows = B + 13
    x = (rng.standard_normal((n_rows, D)) * 1.5 + 0.25).astype(np.float32)
    rows = rng.permutation(n_rows)[:B].astype(np.int32)
    dHT = rng.standard_normal((64, B)).astype(np.float32)
    n64, n32 = copy.deepcopy(net).double(), net
    xt = torch.from_numpy(x[rows])
    f64 = n64.base(xt.double())
    with torch.no_grad():
        f32 = n32.base(xt).numpy()
    err32, tol = RR.err_and_tol(f64.detach().numpy(), f32)
    featT = torch.full((64, B), float("nan"), device="cuda")
    ops.mlp_features(params, desc, dev(x), dev(rows, torch.int32), B, featT)
    err = np.abs(featT.cpu().numpy().T.astype(np.float64) - f64.detach().numpy()).max()
    print(f"features err {err:.2e} (fp32 CPU {err32:.2e})")
    assert err <= tol
    (f64 * torch.from_numpy(dHT.T.copy()).double()).sum().backward()
    ns = ops.mlp_backward_slabs(B)
    P = ((Pn + 255) // 256) * 256
    slabs = torch.zeros(ns, P, device="cuda")
    ops.trunk_backward(params, desc, dev(x), dev(rows, torch.int32), B, dev(dHT), slabs, P, 0)
    grad = torch.zeros(P, device="cuda")
    ops.slab_reduce(slabs, ns, P, P, grad)
    gf = grad.cpu().numpy()
    gr = {k: p.grad.numpy() for k, p in n64.named_parameters() if p.grad is not None}
    seen = 0
    for key, off, shape in layout:
        if key in gr:
            seen += 1
            close_rel_max(gf[off: off + int(np.prod(shape))].reshape(shape), gr[key], 1e-4, f"trunk {key}")
    assert seen >= 6                                                 # feature norm, fc1 (+ LayerNorm), fc2 (+ LayerNorm)


def test_rollout_step_and_features_dual_beyond_512(ops):
    """Both networks beyond 512 columns: mappo_rollout_step (strided (thread, agent) rows read in place, centralized share rows)
    and mappo_mlp_features_dual run one sliced launch per network — bit-equal to the single-network entry points on the same rows."""
    N, M, D = 9, 2, 600
    S, B = M * D, N * M
    actor, da, pa = _net(ops, D, True, 1, True, True)
    critic, dc, pc = _net(ops, S, True, 1, True, False)
    g = torch.Generator(device="cuda").manual_seed(5)
    obs = torch.randn(N, M, D, device="cuda", generator=g) * 1.5
    seed = 0xABCDEF
    actions, logp, values = (torch.full((B,), float("nan"), device="cuda") for _ in range(3))
    ops.rollout_step(pa, da, pc, dc, (obs, M * D, D), (obs, M * D, 0), M, B, None, False, seed, 3, None, actions, logp, values)
    a2, l2 = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    ops.actor_act(pa, da, obs.view(B, D), None, B, False, seed, 3, a2, l2)
    share = obs.view(N, 1, S).expand(N, M, S).reshape(B, S).contiguous()
    v2 = torch.zeros(B, device="cuda")
    ops.mlp_forward(pc, dc, share, None, B, v2)
    for got, want, what in ((actions, a2, "actions"), (logp, l2, "log-probs"), (values, v2, "values")):
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=what)
    fa, fc, fa2, fc2 = (torch.full((64, B), float("nan"), device="cuda") for _ in range(4))
    ops.mlp_features_dual(pa, da, obs.view(B, D), fa, pc, dc, share, fc, B)
    ops.mlp_features(pa, da, obs.view(B, D), None, B, fa2)
    ops.mlp_features(pc, dc, share, None, B, fc2)
    np.testing.assert_array_equal(fa.cpu().numpy(), fa2.cpu().numpy())
    np.testing.assert_array_equal(fc.cpu().numpy(), fc2.cpu().numpy())
    assert np.isfinite(fa.cpu().numpy()).all() and np.isfinite(fc.cpu().numpy()).all()


def test_unchanged_below_limit(ops):
    """in_dim 65 and 512: mappo_mlp_forward and mappo_actor_update (+ mappo_wide_l1_backward) bit-equal to the arrays the same calls
    produced before in_dim 513..2048 was admitted (tests/golden/generate_wide_sliced_golden.py)."""
    import importlib.util
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("generate_wide_sliced_golden", os.path.join(here, "generate_wide_sliced_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = np.load(os.path.join(here, "wide_sliced_parent.npz"))
    got = gen.run(ops, torch, O.default_args())
    assert str(want["meta/commit"]).startswith("732b3d4")            # the parent of the change that admitted 513..2048
    keys = [k for k in want.files if not k.startswith("meta/")]
    assert set(got) == set(keys)
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
