"""mappo_actor_critic_update_group / mappo_reduce_clip_adam_group against the single calls, bit for bit.

The grouped launch runs every job's workgroups through the body the single dual launch runs, with the job-local block index and
count, so a job's slab rows [0, mappo_dual_update_slabs), its zero-filled rows and its loss partials must EQUAL what
mappo_actor_critic_update writes on the same inputs — torch.equal on the whole arrays (NaN-prefilled: compared as bit patterns, so
"wrote nothing else" is part of the equality).  The premise — two single calls on the same inputs are themselves bit-equal — is
asserted first.  Three jobs shaped like simple_adversary (obs 8 / 10 / 10, share 28, 5 actions) with 40, 17 and 64 rows (a ragged
last tile; barely more than one tile; whole tiles), one with a row index, one with masked actions; layer_N 0 / 1 x ReLU / Tanh.  A
two-job case with 16 500 rows reaches unequal workgroup shares (nA < nC: the critic's workgroups zero-fill the actor's rows).
Inputs are drawn as tests/test_gpu_update_matrix.py draws them."""
import numpy as np
import pytest
import torch

from oracle import mappo_oracle as O
from test_gpu_kernels import dev, _flat_from_module, _randomize
from test_gpu_update_matrix import _safe_inputs, upd16_split

pytestmark = pytest.mark.gpu

# (actor in_dim, critic in_dim, actions, rows B, gathered rows, avail)
ADVERSARY = [(8, 28, 5, 40, False, False), (10, 28, 5, 17, True, False), (10, 28, 5, 64, False, True)]
COMBOS = [(0, True), (0, False), (1, True), (1, False)]           # layer_N, ReLU


@pytest.fixture(scope="module")
def ops(gpu_device):
    from mappo_amd import ops as _ops
    return _ops


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(x, y, what):
    assert x.shape == y.shape and torch.equal(_bits(x), _bits(y)), \
        f"{what}: {int((_bits(x) != _bits(y)).sum())} of {x.numel()} elements differ"


class Job:
    """One (actor, critic) pair with its loss inputs on the device."""

    def __init__(self, ops, idx, D, S, A, B, with_rows, with_avail, LN, relu, accumulate):
        torch.manual_seed(100 * idx + B + D)
        rng = np.random.default_rng(1000 * idx + 7 * B + A + 2 * LN + relu)
        a = O.default_args(use_ReLU=relu, layer_N=LN)
        actor, critic = O.ActorRef(a, D, A), O.CriticRef(a, S)
        _randomize(actor, D + 3 + idx); _randomize(critic, S + 4 + idx)
        self.da, self.dc = ops.net_desc(D, A, LN, relu, True), ops.net_desc(S, 1, LN, relu, True)
        self.pa, _, self.Pa = _flat_from_module(ops, actor, self.da, "act.action_out.linear")
        self.pc, _, self.Pc = _flat_from_module(ops, critic, self.dc, "v_out")
        n_rows = B + 64
        obs, sobs, avail, actions, old_logp, adv, active, ret, v_old = _safe_inputs(a, actor, critic, rng, n_rows, D, S, A, relu, "default")
        rows = rng.permutation(n_rows)[:B].astype(np.int32) if with_rows else None
        vn = O.ValueNormRef(); vn.update(ret[:50].reshape(-1, 1)); vn.update(ret[:B].reshape(-1, 1))
        self.B, self.rows = B, dev(rows, torch.int32) if with_rows else None
        self.g = dict(obs=dev(obs), sobs=dev(sobs), avail=dev(avail) if with_avail else None, actions=dev(actions), old=dev(old_logp),
                      adv=dev(adv), active=dev(active), ret=dev(ret), vold=dev(v_old), vn=dev(vn.state()))
        if with_avail:
            assert float(self.g["avail"][:B].min()) == 0.0                   # masked actions inside the batch
        self.mom = torch.zeros(4, dtype=torch.float64, device="cuda")
        ops.minibatch_moments(self.g["ret"], self.g["active"], self.rows, B, self.mom)
        self.cfg = ops.ppo_cfg(a, accumulate_partials=accumulate)
        self.accumulate = accumulate
        self.col_c = ((self.Pa + 255) // 256) * 256
        self.P = self.col_c + ((self.Pc + 255) // 256) * 256
        self.nd = ops.dual_update_slabs(self.da, self.dc, B)
        self.split = upd16_split(D, S, A, LN, B)

    def outputs(self, ops):
        """Fresh NaN-filled slabs (two spare rows) and loss partials (accumulating launches: a finite fill they add to)."""
        slabs = torch.full((self.nd + 2, self.P), float("nan"), device="cuda")
        fill = 1.5 if self.accumulate else float("nan")
        n = ops.update_partials("cuda").numel()
        return slabs, torch.full((n,), fill, dtype=torch.float64, device="cuda"), torch.full((n,), fill, dtype=torch.float64, device="cuda")

    def args(self, out):
        g = self.g
        slabs, part_a, part_c = out
        return (self.pa, self.da, g["obs"], self.pc, self.dc, g["sobs"], self.rows, self.B, g["avail"], g["actions"], g["old"], g["adv"],
                g["active"], g["vold"], g["ret"], g["vn"], self.mom, self.cfg, slabs, self.P, 0, self.col_c, part_a, part_c)

    def single(self, ops):
        out = self.outputs(ops)
        ops.actor_critic_update(*self.args(out))
        return out


def _group(ops, jobs):
    outs = [j.outputs(ops) for j in jobs]
    ops.actor_critic_update_group([ops.update_job(*j.args(o)) for j, o in zip(jobs, outs)])
    return outs


def _check_contract(j, out):
    """Rows [0, nd) of both column ranges finite (written or zero-filled), every other slab entry still NaN."""
    s = out[0]
    assert bool(torch.isfinite(s[:j.nd, :j.Pa]).all()) and bool(torch.isfinite(s[:j.nd, j.col_c:j.col_c + j.Pc]).all())
    assert bool(torch.isnan(s[j.nd:]).all()) and bool(torch.isnan(s[:, j.Pa:j.col_c]).all()) and bool(torch.isnan(s[:, j.col_c + j.Pc:]).all())


_CACHE = {}


def _adversary_jobs(ops, LN, relu):
    key = (LN, relu)
    if key not in _CACHE:
        jobs = [Job(ops, i, *c, LN, relu, accumulate=(LN == 1 and relu)) for i, c in enumerate(ADVERSARY)]
        _CACHE[key] = (jobs, [j.single(ops) for j in jobs])            # the reference: computed once, never written again
    return _CACHE[key]


@pytest.mark.parametrize("LN,relu", COMBOS, ids=[f"L{l}-{'relu' if r else 'tanh'}" for l, r in COMBOS])
def test_group_equals_single_calls(ops, LN, relu):
    jobs, ref = _adversary_jobs(ops, LN, relu)
    for j, r in zip(jobs, ref):                                          # the premise: the single call repeats itself bit for bit
        again = j.single(ops)
        for x, y, n in zip(again, r, ("slabs", "actor partials", "critic partials")):
            _same(x, y, f"single call twice, B={j.B}: {n}")
        _check_contract(j, r)
    # all three in one launch, in two orders; each alone (n_jobs = 1)
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        outs = _group(ops, [jobs[i] for i in order])
        for i, out in zip(order, outs):
            for x, y, n in zip(out, ref[i], ("slabs", "actor partials", "critic partials")):
                _same(x, y, f"order {order}, job of B={jobs[i].B}: {n}")
    for j, r in zip(jobs, ref):
        (out,) = _group(ops, [j])
        for x, y, n in zip(out, r, ("slabs", "actor partials", "critic partials")):
            _same(x, y, f"n_jobs = 1, B={j.B}: {n}")
    torch.cuda.synchronize()


def test_group_with_unequal_shares_and_eight_jobs(ops):
    """16 500 rows with an 18-wide actor and a 54-wide critic: nA < nC, the critic's last workgroups zero-fill the actor's slab and
    partial rows — inside a group of 8 (the limit), between small jobs, and with a 40-wide actor without a hidden layer beside
    narrow ones (both body widths in one launch)."""
    big = Job(ops, 7, 18, 54, 5, 16500, True, True, 0, True, False)
    assert big.split[0] < big.split[1] == big.nd and big.nd > 64
    wide = Job(ops, 8, 40, 28, 12, 50, False, True, 0, True, False)
    small, _ = _adversary_jobs(ops, 0, True)
    jobs = [small[0], big, small[1], wide, small[2], small[0], wide, small[1]]
    ref = [j.single(ops) for j in jobs]
    _check_contract(big, ref[1])
    assert float(ref[1][0][big.split[0]:big.nd, :big.Pa].abs().max()) == 0.0        # the zero-filled actor rows
    outs = _group(ops, jobs)
    for k, (j, out, r) in enumerate(zip(jobs, outs, ref)):
        for x, y, n in zip(out, r, ("slabs", "actor partials", "critic partials")):
            _same(x, y, f"job {k} (B={j.B}): {n}")


def _optim_state(j, slabs, seed):
    g = torch.Generator().manual_seed(seed)
    P = j.P
    params = torch.zeros(P)
    params[:j.Pa] = j.pa.cpu(); params[j.col_c:j.col_c + j.Pc] = j.pc.cpu()
    m = 0.01 * torch.randn(P, generator=g)
    v = 1e-4 * torch.rand(P, generator=g)
    # per segment {lr, beta1, beta2, eps, weight_decay, max_grad_norm, use_clip, enabled}
    hyper = torch.tensor([[5e-4, 0.9, 0.999, 1e-5, 0.0, 0.5 if seed % 2 else 10.0, 1.0, 1.0],
                          [7e-4, 0.9, 0.999, 1e-5, 1e-3 if seed % 2 else 0.0, 10.0, 1.0, 1.0]])
    return dict(slabs=slabs, params=params.cuda(), grad=torch.full((P,), float("nan"), device="cuda"), m=m.cuda(), v=v.cuda(),
                hyper=hyper.cuda(), step=torch.tensor([3, 5 + seed], dtype=torch.int32, device="cuda"),
                norms=torch.zeros(2, device="cuda"), acc=torch.full((2,), 0.25, dtype=torch.float64, device="cuda"))


def _clone(st):
    return {k: v.clone() for k, v in st.items()}


def test_optim_group_equals_single_calls(ops):
    """Parameters, gradient, Adam moments, steps, norms and the norm accumulator after two successive optimiser calls per job:
    grouped (three jobs, two orders, and alone) against mappo_reduce_clip_adam, on the slabs of the update test."""
    jobs, ref = _adversary_jobs(ops, 1, False)
    big = Job(ops, 7, 18, 54, 5, 16500, True, True, 1, False, False)       # 129 slab rows: the 16-row batches of the reduction
    jobs = jobs + [big]
    # (the padding columns between the networks' ranges are the caller's: zero, as in the trainer's slab array)
    slabs = [torch.nan_to_num(s, nan=0.0) for s in [r[0] for r in ref] + [big.single(ops)[0]]]
    states = [_optim_state(j, s, k) for k, (j, s) in enumerate(zip(jobs, slabs))]
    seg = lambda j: [0, j.col_c, j.P]
    ws = [ops.optim_workspace(j.P, "cuda") for j in jobs]

    def single(k):
        st, j = _clone(states[k]), jobs[k]
        for _ in range(2):
            ops.reduce_clip_adam(st["slabs"], j.nd, j.P, st["params"], st["grad"], st["m"], st["v"], seg(j), st["hyper"], st["step"],
                                 st["norms"], ws[k], norm_acc=st["acc"])
        return st

    def grouped(order):
        sts = [_clone(states[k]) for k in order]
        for _ in range(2):
            ops.reduce_clip_adam_group([ops.optim_job(st["slabs"], jobs[k].nd, jobs[k].P, st["params"], st["grad"], st["m"], st["v"], seg(jobs[k]),
                                                      st["hyper"], st["step"], st["norms"], ws[k], norm_acc=st["acc"])
                                        for k, st in zip(order, sts)])
        return sts

    want = [single(k) for k in range(len(jobs))]
    again = single(3)
    for name in ("params", "grad", "m", "v", "step", "norms", "acc"):
        assert torch.equal(again[name], want[3][name]), f"single call twice: {name}"          # the premise
    for k, w in enumerate(want):
        assert bool(torch.isfinite(w["params"]).all()) and not torch.equal(w["params"], states[k]["params"])
        assert w["step"].tolist() == [5, 7 + k] and float(w["norms"].min()) > 0.0
    for order in ([0, 1, 2, 3], [3, 1, 0, 2], [2], [3]):
        for k, got in zip(order, grouped(order)):
            for name in ("params", "grad", "m", "v", "step", "norms", "acc"):
                assert torch.equal(got[name], want[k][name]), f"order {order}, job {k}: {name}"
