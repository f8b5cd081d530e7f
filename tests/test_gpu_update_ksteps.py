"""The 16-sample-tile update kernels (mlp_upd16.h) run exactly C = ceil(in_dim / 4) layer-1 k-steps: the last group of four
takes C % 4 of them.  Input widths that cover every residue of C % 4, for the narrow (in_dim <= 32) and the wide (33..64)
body and on both networks of the dual launch, with ragged last tiles: fused single-network launches, the dual launch, the
unfused kernels and autograd through the oracle networks agree (tolerances of test_gpu_kernels.py), and repeated dual
launches are bit-identical."""
import numpy as np
import pytest
import torch

from oracle import mappo_oracle as O
from test_gpu_kernels import test_fused_update_kernels_vs_unfused_and_autograd as _fused_vs_unfused_and_autograd


def _c_mod4(d):
    return ((d + 3) // 4) % 4


# (actor in_dim, critic in_dim): actor narrow C % 4 = 0, 1, 2, 3 | critic wide C % 4 = 3, 2, 0, 1 (an actor wider than 32
# inputs with layer_N = 1 does not fit the 16-sample-tile kernel's LDS and takes the pair kernel: test_gpu_update_matrix.py)
KSTEP_CASES = [(13, 44, 5, True, 333, True), (17, 54, 5, True, 1001, False), (22, 61, 9, False, 517, True),
               (26, 33, 3, True, 250, False), (18, 64, 5, True, 3072, True), (30, 54, 16, False, 129, False),
               (25, 21, 7, True, 495, False), (10, 14, 2, False, 17, True)]


def test_cases_cover_every_residue():
    narrow = {_c_mod4(d) for c in KSTEP_CASES for d in c[:2] if d <= 32}
    wide = {_c_mod4(d) for c in KSTEP_CASES for d in c[:2] if 32 < d <= 64}
    assert narrow == {0, 1, 2, 3} and wide == {0, 1, 2, 3}


@pytest.fixture(scope="module")
def ops(gpu_device):
    from mappo_amd import ops as _ops
    return _ops


@pytest.mark.gpu
@pytest.mark.parametrize("D,S,A,relu,B,with_rows", KSTEP_CASES)
def test_update_ksteps_vs_unfused_and_autograd(ops, D, S, A, relu, B, with_rows):
    _fused_vs_unfused_and_autograd(ops, D, S, A, relu, B, with_rows)


@pytest.mark.gpu
@pytest.mark.parametrize("D,S,B", [(26, 44, 5003), (17, 61, 76800 - 9)])
def test_dual_update_ksteps_deterministic(ops, D, S, B):
    """Repeated dual launches (row gather, ragged last tile) give bit-identical gradients and loss statistics."""
    cfg = ops.ppo_cfg(O.default_args())
    NR = B + 100
    g = torch.Generator(device="cuda").manual_seed(D * S)
    da, dc = ops.net_desc(D, 5), ops.net_desc(S, 1)
    Pa, Pc = ops.net_param_count(da), ops.net_param_count(dc)
    col_c = ((Pa + 255) // 256) * 256
    P = col_c + ((Pc + 255) // 256) * 256
    pa = torch.randn(Pa, device="cuda", generator=g) * 0.1
    pc = torch.randn(Pc, device="cuda", generator=g) * 0.1
    obs, sobs = torch.randn(NR, D, device="cuda", generator=g), torch.randn(NR, S, device="cuda", generator=g)
    ret = torch.randn(NR, device="cuda", generator=g)
    active = (torch.rand(NR, device="cuda", generator=g) > 0.1).float()
    rows = torch.randperm(NR, device="cuda", generator=g)[:B].to(torch.int32).contiguous()
    mom = torch.zeros(4, dtype=torch.float64, device="cuda")
    ops.minibatch_moments(ret, active, rows, B, mom)
    av = (torch.rand(NR, 5, device="cuda", generator=g) > 0.2).float()
    av[:, 0] = 1
    act = torch.randint(0, 5, (NR,), device="cuda", generator=g).float()
    av[torch.arange(NR, device="cuda"), act.long()] = 1
    olp = -torch.rand(NR, device="cuda", generator=g) - 1
    adv, vold = torch.randn(NR, device="cuda", generator=g), torch.randn(NR, device="cuda", generator=g)
    vn = torch.tensor([0., 1., 1.], device="cuda")
    nd = ops.dual_update_slabs(da, dc, B)

    def run():
        slabs = torch.full((nd, P), float("nan"), device="cuda")
        pda, pdc = ops.update_partials("cuda"), ops.update_partials("cuda")
        ops.actor_critic_update(pa, da, obs, pc, dc, sobs, rows, B, av, act, olp, adv, active, vold, ret, vn, mom, cfg, slabs, P, 0, col_c, pda, pdc)
        stats = torch.zeros(6, dtype=torch.float64, device="cuda")
        ops.update_stats(pda, nd, pdc, nd, mom, cfg, stats)
        # every slab row the launch owns is written in full (its own network's columns, or zeros for the other network)
        s = slabs.cpu().numpy()
        assert np.isfinite(s[:, :Pa]).all() and np.isfinite(s[:, col_c:col_c + Pc]).all()
        return s, stats.cpu().numpy()

    s0, t0 = run()
    for _ in range(10):
        s, t = run()
        assert np.array_equal(s[:, :Pa], s0[:, :Pa]) and np.array_equal(s[:, col_c:col_c + Pc], s0[:, col_c:col_c + Pc])
        assert np.array_equal(t, t0)
