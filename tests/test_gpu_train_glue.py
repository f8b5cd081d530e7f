"""The fused once-per-train() launches (csrc/train_glue.hip) against the separate launches they replace, bit for bit:
mappo_train_prologue == adv_moments + minibatch_moments + valuenorm_update_n + a fill (adv_normalize follows on both sides),
mappo_train_epilogue == update_stats + copy_batch, and a trainer with fuse_train_glue on == the same trainer with it off.
Both forms run the same device functions (csrc/stats_core.h, insert_core.h) over the same partition, so `torch.equal` is the
bound everywhere."""
import numpy as np
import pytest
import torch

from mappo_amd import ops

BETA = 0.99999
N_ZERO, PAD = 2056, 5           # the trainer's fill range, and guard doubles on either side of it


def _inputs(n, seed, active="ones", dev="cuda:0"):
    g = torch.Generator(device=dev).manual_seed(seed)
    ret = torch.randn(n, device=dev, generator=g) * 3.0 + 1.5
    vp = torch.randn(n, device=dev, generator=g)
    if active == "ones":
        act = torch.ones(n, device=dev)
    elif active == "zeros":
        act = torch.zeros(n, device=dev)
    else:                                                     # ~30 % zeros
        act = (torch.rand(n, device=dev, generator=g) >= 0.3).float()
    vn = torch.tensor([0.37, 2.9, 0.81], device=dev) + torch.rand(3, device=dev, generator=g) * 0.1
    return ret, vp, act, vn


def _separate(ret, vp, act, vn, n_epochs):
    """The launches the prologue replaces (+ the normalisation), on copies of the state they update."""
    dev, n = ret.device, ret.numel()
    adv = torch.empty(n, device=dev)
    am = torch.zeros(3, dtype=torch.float64, device=dev)
    mm = torch.zeros(4, dtype=torch.float64, device=dev)
    vn = vn.clone() if vn is not None else None
    states = torch.full((n_epochs, 3), float("nan"), device=dev)
    ops.adv_moments(ret, vp, act, vn, adv, am)
    ops.adv_normalize(adv, am)
    ops.minibatch_moments(ret, act, None, n, mm)
    if vn is not None:
        ops.valuenorm_update_n(vn, mm, BETA, n_epochs, states)
    return dict(adv=adv, adv_moments=am, mb_moments=mm, states=states, vn=vn)


class _Fused:
    """One workspace, one ticket word, one set of output arrays: reused by every call, as the trainer does."""

    def __init__(self, n, n_epochs, dev="cuda:0"):
        self.ws, self.ticket = ops.train_prologue_workspace(n, dev)
        self.adv = torch.empty(n, device=dev)
        self.am = torch.zeros(3, dtype=torch.float64, device=dev)
        self.mm = torch.zeros(4, dtype=torch.float64, device=dev)
        self.states = torch.full((n_epochs, 3), float("nan"), device=dev)
        self.zbuf = torch.empty(PAD + N_ZERO + PAD, dtype=torch.float64, device=dev)
        self.n_epochs = n_epochs

    def poison(self):
        self.zbuf.fill_(float("nan"))
        self.zbuf[:PAD] = 7.0
        self.zbuf[-PAD:] = -7.0

    def launch(self, ret, vp, act, vn):
        ops.train_prologue(ret, vp, act, vn, self.adv, self.am, self.mm, BETA, self.n_epochs, self.states if vn is not None else None,
                           self.zbuf[PAD:PAD + N_ZERO], self.ws, self.ticket)
        ops.adv_normalize(self.adv, self.am)

    def check(self, want, vn, what=""):
        got = dict(adv=self.adv, adv_moments=self.am, mb_moments=self.mm, states=self.states, vn=vn)
        for k, w in want.items():
            if w is None:
                assert got[k] is None
                continue
            if k == "states" and vn is None:
                continue
            assert torch.equal(got[k], w), f"{what}{k}: max |diff| {(got[k].double() - w.double()).abs().max().item()}"
        z = self.zbuf
        assert torch.equal(z[PAD:PAD + N_ZERO], torch.zeros(N_ZERO, dtype=torch.float64, device=z.device)), f"{what}fill range"
        assert bool((z[:PAD] == 7.0).all()) and bool((z[-PAD:] == -7.0).all()), f"{what}doubles next to the fill range"
        assert int(self.ticket.item()) == 0, f"{what}ticket word"


# 1: the only workgroup is its own last one; 1023..1025: one -> two workgroups; 257*1024+3: more than 256 workgroups, the final
# reduction strides a second time; 1024*1024+5: the grid is capped at 1024 workgroups and every thread takes a second trip
SIZES = [1, 1023, 1024, 1025, 257 * 1024 + 3, 1024 * 1024 + 5]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_prologue_matches_separate_launches(gpu_device, n):
    ret, vp, act, vn = _inputs(n, seed=n % 1000)
    want = _separate(ret, vp, act, vn, 10)
    f = _Fused(n, 10)
    f.poison()
    vn_f = vn.clone()
    f.launch(ret, vp, act, vn_f)
    torch.cuda.synchronize()
    f.check(want, vn_f)
    assert float(f.mm[3].item()) == float(n)


@pytest.mark.gpu
@pytest.mark.parametrize("active,use_vn,n_epochs", [("some", True, 10), ("zeros", True, 10), ("ones", False, 10), ("some", True, 1),
                                                     ("zeros", False, 1)])
def test_prologue_flag_variants(gpu_device, active, use_vn, n_epochs):
    n = 3 * 1024 + 17
    ret, vp, act, vn = _inputs(n, seed=11, active=active)
    if not use_vn:
        vn = None
    want = _separate(ret, vp, act, vn, n_epochs)
    f = _Fused(n, n_epochs)
    f.poison()
    vn_f = vn.clone() if vn is not None else None
    f.launch(ret, vp, act, vn_f)
    torch.cuda.synchronize()
    f.check(want, vn_f)
    if active == "zeros":
        assert float(f.am[2].item()) == 0.0 and bool(torch.isfinite(f.adv).all())       # the count guard of adv_normalize


@pytest.mark.gpu
def test_prologue_ticket_reuse_and_graph_replay(gpu_device):
    """Three eager calls, then one captured call replayed twice on changed inputs: one workspace, one ticket word."""
    n = 40 * 1024 + 9
    f = _Fused(n, 10)
    for k in range(3):
        ret, vp, act, vn = _inputs(n, seed=100 + k, active="some")
        want = _separate(ret, vp, act, vn, 10)
        f.poison()
        vn_f = vn.clone()
        f.launch(ret, vp, act, vn_f)
        torch.cuda.synchronize()
        f.check(want, vn_f, what=f"eager call {k}: ")
    # static inputs of the graph
    ret, vp, act, vn_f = (t.clone() for t in _inputs(n, seed=200, active="some"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f.launch(ret, vp, act, vn_f)
    for k in range(2):
        r2, v2, a2, vn2 = _inputs(n, seed=300 + k, active="some")
        ret.copy_(r2), vp.copy_(v2), act.copy_(a2), vn_f.copy_(vn2)
        want = _separate(ret, vp, act, vn_f, 10)
        f.poison()
        g.replay()
        torch.cuda.synchronize()
        f.check(want, vn_f, what=f"replay {k}: ")


def _cfg(policy_active=True, value_active=True):
    from mappo_amd.config import get_config
    a = get_config().parse_known_args([])[0]
    a.use_policy_active_masks, a.use_value_active_masks = policy_active, value_active
    return ops.ppo_cfg(a)


@pytest.mark.gpu
@pytest.mark.parametrize("with_acc", [True, False])
@pytest.mark.parametrize("n_critic", [1, 300])
@pytest.mark.parametrize("n_actor", [0, 1, 256])
def test_epilogue_matches_update_stats_and_copy_batch(gpu_device, n_actor, n_critic, with_acc):
    dev = gpu_device
    g = torch.Generator(device=dev).manual_seed(1000 * n_actor + 10 * n_critic + with_acc)
    f64 = dict(dtype=torch.float64, device=dev)
    pa = torch.randn(max(n_actor, 1), 4, generator=g, **f64) if n_actor else None
    pc = torch.randn(n_critic, 4, generator=g, **f64)
    mm = torch.tensor([12.5, 99.0, 61000.0, 76800.0], **f64)
    cfg = _cfg(policy_active=bool(n_actor % 2), value_active=bool(n_critic % 2))
    acc0 = torch.randn(6, generator=g, **f64)
    for numels in ([1], [7], [4096 + 3], [1, 7, 4096 + 3] * 5 + [64]):          # 1 pair (three sizes) and 16 pairs
        srcs = [torch.randn(m, device=dev, generator=g) for m in numels]
        # odd sizes leave the next array of a packed allocation off 16-byte alignment: both copy paths run
        pool = torch.randn(sum(numels) + 4 * len(numels), device=dev, generator=g)
        outs = []
        for fused in (False, True):
            dst_pool, off, dsts = pool.clone(), 0, []
            for m in numels:
                dsts.append(dst_pool[off:off + m])
                off += m + (m % 3)
            stats = torch.full((6,), float("nan"), **f64)
            acc = acc0.clone() if with_acc else None
            pairs = list(zip(dsts, srcs))
            if fused:
                ops.train_epilogue(pa, n_actor, pc, n_critic, mm, cfg, stats, acc, pairs)
            else:
                ops.update_stats(pa, n_actor, pc, n_critic, mm, cfg, stats, acc)
                ops.copy_batch(pairs)
            torch.cuda.synchronize()
            outs.append((stats, acc, dst_pool, dsts))
        (s0, a0, p0, d0), (s1, a1, p1, d1) = outs
        assert torch.equal(s0, s1) and bool(torch.isfinite(s1).all()), f"stats ({len(numels)} pairs)"
        if with_acc:
            assert torch.equal(a0, a1) and not torch.equal(a1, acc0)
        for j, (x, y) in enumerate(zip(d0, d1)):
            assert torch.equal(x, y) and torch.equal(y, srcs[j]), f"destination {j} of {len(numels)}"
        assert torch.equal(p0, p1)                                                  # nothing outside the destinations moved


def _runner(fuse, use_valuenorm=True, N=8, T=5):
    from mappo_amd.config import get_config
    from mappo_amd.envs.synthetic import SyntheticMPEEnv
    from mappo_amd.runner.shared.mpe_runner import MPERunner
    dev = torch.device("cuda:0")
    M, D, A = 3, 18, 5
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.ppo_epoch, a.use_valuenorm, a.fuse_train_glue = 3, use_valuenorm, fuse
    torch.manual_seed(1)
    env = SyntheticMPEEnv(N, M, D, A, T, seed=1, device=dev)
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=M, device=dev, run_dir=None))
    r.warmup()
    return r


def _trainer_state(r):
    p = r.policy
    out = dict(params=p.flat_params, exp_avg=p.exp_avg, exp_avg_sq=p.exp_avg_sq, returns=r.buffer.returns,
               obs0=r.buffer.obs[0], masks0=r.buffer.masks[0])
    if r.trainer.value_normalizer is not None:
        out["vn_state"] = r.trainer.value_normalizer.state
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("use_valuenorm,update_actor", [(True, True), (False, True), (True, False)])
def test_trainer_with_fused_glue_is_bit_identical(gpu_device, use_valuenorm, update_actor):
    """Four iterations (eager pass, capture + replay, two replays) of two runners that differ in fuse_train_glue only."""
    runs = []
    for fuse in (False, True):
        r = _runner(fuse, use_valuenorm)
        assert r.trainer._fuse_glue == fuse
        steps = []
        for _ in range(4):
            if update_actor:
                info, _ = r.run_episode()
            else:
                r.rollout()
                r.trainer.prep_training()
                info = r.trainer.train(r.buffer, update_actor=False, after_update=True)
            torch.cuda.synchronize()
            steps.append((info, _trainer_state(r)))
        assert (r.trainer._glue_ws is not None) == fuse                            # the path under test was (not) taken
        runs.append(steps)
    for it, ((i0, s0), (i1, s1)) in enumerate(zip(*runs)):
        assert set(i0) == set(i1)
        for k in i0:
            assert np.float64(i0[k]).tobytes() == np.float64(i1[k]).tobytes(), f"iteration {it}: train_info[{k}] {i0[k]!r} != {i1[k]!r}"
        for k in s0:
            assert torch.equal(s0[k], s1[k]), f"iteration {it}: {k}"
    assert not torch.equal(runs[1][0][1]["params"], runs[1][3][1]["params"])          # training moved the parameters
