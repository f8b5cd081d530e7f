"""The synthetic SMAC env kernels (csrc/synth_env.hip: mappo_synth_smac_step, mappo_synth_smac_pool) against the host Philox mirror
(tests/synth_ref.py), value by value, at the grids where the launch's own counter advance (a two-level ticket scheme over
min(grid, 32) groups) changes shape: 1, 31, 32, 33 and 65 workgroups, and over the grid caps (4096 / 8192), where the grid-stride
loop takes a second trip.  avail, dones, dead and the counter are equal to the mirror, the tickets are zero after every launch; the
normals are held to the neighbouring draw (see test_step_normals...); the dead / terminated state machine, graph replays and the
Python wrapper follow the same stream.  Every output sits in front of a guard region.

Normals, as measured on the MI355X (the worst |kernel - float64| / bound over every case below, the bound being the largest change of
the float64 normal when one of its two uniforms moves one step of the 24-bit grid):
  the kernel (Box-Muller in float64 on the device, rounded to float32 once)       0.624  (at over_cap_p3; 0.60 .. 0.62 at the 31 .. 65
                                                                                         workgroup shapes; the float32 cast of the mirror gives
                                                                                         the same figures: it is a correctly rounded float32,
                                                                                         for which first-order calculus gives at most 2 / e = 0.74)
  the float32 formula sqrtf(-2 logf(u1)) cosf(6.2831853f u2) evaluated in NumPy   2.556  (the product 6.2831853f * u2 alone rounds by up to
                                                                                         2.4e-7 where a grid step of u2 turns the angle by 3.7e-7)
  the kernel as it was before these tests, that formula on __logf / __cosf        3.211  (it missed the bound at every shape but `minimal`:
                                                                                         1.2 .. 3.2; this is why the kernel changed)
"""
import functools

import numpy as np
import pytest
import torch

import synth_ref as SR

pytestmark = pytest.mark.gpu

G = 64                 # guard entries behind every array
SENT = 9               # guard / not-yet-written value of the uint8 arrays
P_DEATH, P_TERM = 0.05, 0.1


def _seed(name):
    return SR.SEEDS[name.split("_p")[0]]


def _guarded(shape, dtype=torch.float32):
    """(the whole buffer, the owned view of `shape`): float arrays hold NaN everywhere, bool arrays (uint8 storage) SENT."""
    n = int(np.prod(shape))
    if dtype == torch.bool:
        full = torch.full((n + G,), SENT, dtype=torch.uint8, device="cuda")
        return full, full[:n].view(torch.bool).view(*shape)
    full = torch.full((n + G,), float("nan"), dtype=torch.float32, device="cuda")
    return full, full[:n].view(*shape)


class Bufs:
    """The outputs of one launch ([P] leading for a pool), each in front of its guard."""

    def __init__(self, N, M, D, S, A, P=None):
        lead = () if P is None else (P,)
        self.full, self.view = {}, {}
        for k, shape, dt in (("obs", (N, M, D), torch.float32), ("share", (N, M, S), torch.float32), ("avail", (N, M, A), torch.float32),
                             ("rewards", (N,), torch.float32), ("dones", (N, M), torch.bool)):
            self.full[k], self.view[k] = _guarded(lead + shape, dt)

    def host(self):
        """Host copies of the owned parts (uint8 for dones, so that an unwritten SENT shows); asserts the guards."""
        out = {}
        for k, full in self.full.items():
            n = self.view[k].numel()
            if full.dtype == torch.uint8:
                assert bool((full[n:] == SENT).all()), f"{k}: guard touched"
            else:
                assert bool(torch.isnan(full[n:]).all()), f"{k}: guard touched"
            out[k] = full[:n].view(*self.view[k].shape).cpu().numpy()
        return out


def _state(N, M, dead0):
    """(dead buffer, dead view [N, M] bool, counter buffer, counter view [34])."""
    dfull, dead = _guarded((N, M), torch.bool)
    dfull[:N * M] = torch.from_numpy(np.asarray(dead0, dtype=np.uint8).reshape(-1)).cuda()
    cfull = torch.full((34 + G,), -77, dtype=torch.int64, device="cuda")
    cfull[:34] = 0
    cfull[0] = 1
    return dfull, dead, cfull, cfull[:34]


def _dead0(N, M):
    return np.arange(N * M).reshape(N, M) % 3 == 1


def _launch(bufs, dead, ctr, seed, p_death=P_DEATH, p_term=P_TERM, pooled=False):
    from mappo_amd import ops
    v = bufs.view
    (ops.synth_smac_pool if pooled else ops.synth_smac_step)(v["obs"], v["share"], v["avail"], v["rewards"], dead, v["dones"], p_death, p_term,
                                                              seed, ctr)


def _finish(dfull, cfull, N, M):
    """Host copies of dead [N, M] uint8 and the counter words [34], their guards asserted."""
    assert bool((dfull[N * M:] == SENT).all()), "dead: guard touched"
    assert bool((cfull[34:] == -77).all()), "counter: guard touched"
    return dfull[:N * M].view(N, M).cpu().numpy(), cfull[:34].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _three_launches(name, pooled):
    """Three launches back to back, no host synchronisation between them, each into buffers of its own; the results on the host,
    computed once per case and shared read-only by the tests on exact outputs and on normals.  The tickets are read after the third
    launch only; every launch needs them zero to advance, so the counter after three launches holds the first two to it as well."""
    shape, P = SR.POOL_SHAPES[name] if pooled else (SR.STEP_SHAPES[name], None)
    N, M, D, S, A = shape
    dfull, dead, cfull, ctr = _state(N, M, _dead0(N, M))
    bufs = [Bufs(N, M, D, S, A, P) for _ in range(3)]
    for b in bufs:
        _launch(b, dead, ctr, _seed(name), pooled=pooled)
    torch.cuda.synchronize()
    dead_h, ctr_h = _finish(dfull, cfull, N, M)
    return [b.host() for b in bufs], dead_h, ctr_h


@functools.lru_cache(maxsize=None)
def _mirror(name, pooled):
    """The mirror of _three_launches: a list of three step() / pool() results, computed once per case and left unchanged."""
    shape, P = SR.POOL_SHAPES[name] if pooled else (SR.STEP_SHAPES[name], None)
    N, M = shape[:2]
    dead, c, out = _dead0(N, M), 1, []
    for _ in range(3):
        o = SR.pool(_seed(name), c, *shape, P_DEATH, P_TERM, dead, P) if pooled else SR.step(_seed(name), c, *shape, P_DEATH, P_TERM, dead)
        dead, c = o["dead_out"], o["counter"]
        out.append(o)
    return out


def _assert_exact(got, want, what):
    """avail, dones of one launch against the mirror's; every owned entry written."""
    assert got["dones"].max() <= 1, f"{what}: a dones entry was not written"
    np.testing.assert_array_equal(got["dones"], want["dones"].astype(np.uint8), err_msg=f"{what}: dones")
    assert not np.isnan(got["avail"]).any(), f"{what}: an avail entry was not written"
    np.testing.assert_array_equal(got["avail"], want["avail"], err_msg=f"{what}: avail")


def _normal_ratio(got, want, what):
    """The worst |kernel - float64| / bound over obs, share and rewards of one launch; every entry finite (and so written)."""
    worst = 0.0
    for k in ("obs", "share", "rewards"):
        assert np.isfinite(got[k]).all(), f"{what}: {k} has a non-finite (or unwritten) entry"
        worst = max(worst, float((np.abs(got[k].astype(np.float64) - want[k]) / want[k + "_bound"]).max()))
    return worst


def _check_exact(name, pooled):
    got, dead_h, ctr_h = _three_launches(name, pooled)
    want = _mirror(name, pooled)
    for i in range(3):
        _assert_exact(got[i], want[i], f"launch {i}")
    assert dead_h.max() <= 1
    np.testing.assert_array_equal(dead_h, want[2]["dead_out"].astype(np.uint8), err_msg="dead after the third launch")
    steps = 3 * (SR.POOL_SHAPES[name][1] if pooled else 1)
    assert int(ctr_h[0]) == want[2]["counter"] == 1 + steps, "the counter after three launches"
    assert not ctr_h[1:].any(), f"tickets left non-zero: {ctr_h[1:].tolist()}"


def _check_normals(name, pooled):
    got, _, _ = _three_launches(name, pooled)
    want = _mirror(name, pooled)
    ratios = [_normal_ratio(got[i], want[i], f"launch {i}") for i in range(3)]
    f32 = max(w["f32_ratio"] for w in want)
    print(f"{name}: worst |kernel - float64| / bound {max(ratios):.3f}; the float32 formula in NumPy {f32:.3f}")
    if name.startswith("over_cap"):
        # the two ends of u1 over the whole stream of this case: the largest normal's radius and the one closest to zero
        for u, i, k, j in SR.extreme_u1(want):
            g, w, b = float(got[i][k].reshape(-1)[j]), float(want[i][k].reshape(-1)[j]), float(want[i][k + "_bound"].reshape(-1)[j])
            print(f"  u1 = {u:.9g}: kernel {g:.9g}, float64 {w:.9g}, bound {b:.3g}, ratio {abs(g - w) / b:.3f}")
            assert abs(g - w) <= b, (u, g, w, b)
    assert max(ratios) <= 1.0, ratios


# ---- exact outputs and the counter, per grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SR.STEP_SHAPES))
def test_step_exact_outputs_and_counter(gpu_device, name):
    """avail, dones, dead and the counter equal the mirror over three unsynchronised launches; the 33 tickets are zero again."""
    _check_exact(name, False)


@pytest.mark.parametrize("name", list(SR.POOL_SHAPES))
def test_pool_exact_outputs_and_counter(gpu_device, name):
    _check_exact(name, True)


# ---- normals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SR.STEP_SHAPES))
def test_step_normals_within_the_neighbouring_draw(gpu_device, name):
    """obs, share_obs and rewards against the float64 Box-Muller of the same uniforms: every value finite and no further from it than
    the float64 value moves when one of the two uniforms moves one step of its grid (a bound from the mirror alone).  Figures: the
    module's docstring."""
    _check_normals(name, False)


@pytest.mark.parametrize("name", list(SR.POOL_SHAPES))
def test_pool_normals_within_the_neighbouring_draw(gpu_device, name):
    _check_normals(name, True)


# ---- the dead / terminated state machine -----------------------------------------------------------------------------------------------------
def _state_mirror(p_death, p_term, dead0, steps):
    c = SR.STATE_CASE
    return SR.run(c["seed"], 1, c["N"], c["M"], c["D"], c["S"], c["A"], p_death, p_term, dead0, steps)[0]


def _run_stepwise(p_death, p_term, dead0, steps):
    """-> (dones per step, dead after each step, counter words)."""
    c = SR.STATE_CASE
    N, M = c["N"], c["M"]
    dfull, dead, cfull, ctr = _state(N, M, dead0)
    b = Bufs(N, M, c["D"], c["S"], c["A"])
    dones, deads = [], []
    for _ in range(steps):
        _launch(b, dead, ctr, c["seed"], p_death, p_term)
        dones.append(b.host()["dones"])
        deads.append(_finish(dfull, cfull, N, M)[0])
    return dones, deads, _finish(dfull, cfull, N, M)[1]


def _run_pooled(p_death, p_term, dead0, steps, P):
    """-> (dones per step, dead after each pool, counter words)."""
    c = SR.STATE_CASE
    N, M = c["N"], c["M"]
    dfull, dead, cfull, ctr = _state(N, M, dead0)
    b = Bufs(N, M, c["D"], c["S"], c["A"], P)
    dones, deads = [], []
    for _ in range(-(-steps // P)):
        _launch(b, dead, ctr, c["seed"], p_death, p_term, pooled=True)
        dones.extend(b.host()["dones"])
        deads.append(_finish(dfull, cfull, N, M)[0])
    return dones[:steps], deads, _finish(dfull, cfull, N, M)[1]


def test_state_machine_stepwise(gpu_device):
    """12 steps at p_death 0.3, p_term 0.2 from a state with dead agents (every transition occurs: tests/test_synth_ref.py): dones and
    dead equal the mirror at every step."""
    c = SR.STATE_CASE
    want = _state_mirror(c["p_death"], c["p_term"], SR.state_case_dead0(), c["steps"])
    dones, deads, ctr = _run_stepwise(c["p_death"], c["p_term"], SR.state_case_dead0(), c["steps"])
    for t in range(c["steps"]):
        np.testing.assert_array_equal(dones[t], want[t]["dones"].astype(np.uint8), err_msg=f"dones, step {t}")
        np.testing.assert_array_equal(deads[t], want[t]["dead_out"].astype(np.uint8), err_msg=f"dead, step {t}")
    assert ctr.tolist() == [1 + c["steps"]] + [0] * 33


def test_state_machine_pooled(gpu_device):
    """The same 12 steps through pools of 5 (a pool boundary inside the run; the third pool draws steps 10..14): dones at every step,
    dead — which a pool launch carries to the pool's end — after steps 5, 10 and 15."""
    c, P = SR.STATE_CASE, 5
    want = _state_mirror(c["p_death"], c["p_term"], SR.state_case_dead0(), 15)
    dones, deads, ctr = _run_pooled(c["p_death"], c["p_term"], SR.state_case_dead0(), c["steps"], P)
    assert len(dones) == c["steps"] and len(deads) == 3
    for t in range(c["steps"]):
        np.testing.assert_array_equal(dones[t], want[t]["dones"].astype(np.uint8), err_msg=f"dones, step {t}")
    for j in range(3):
        np.testing.assert_array_equal(deads[j], want[P * (j + 1) - 1]["dead_out"].astype(np.uint8), err_msg=f"dead after pool {j}")
    assert ctr.tolist() == [1 + 3 * P] + [0] * 33


@pytest.mark.parametrize("pooled", [False, True], ids=["step", "pool"])
def test_state_machine_degenerate_probabilities(gpu_device, pooled):
    """The uniforms lie in (0, 1]: `<= 1` always fires, `<= 0` never.  p_term = 1: every env ends every step, everybody reports done
    and dead is zero after it, whatever it held.  p_death = 1, p_term = 0: everybody is dead and done from the first step on."""
    run = (lambda *a: _run_pooled(*a, 5)) if pooled else _run_stepwise
    c = SR.STATE_CASE
    for p_death, p_term, dead0, dead_after in ((c["p_death"], 1.0, SR.state_case_dead0(), 0), (1.0, 0.0, np.zeros((c["N"], c["M"]), bool), 1)):
        want = _state_mirror(p_death, p_term, dead0, 5)
        dones, deads, _ = run(p_death, p_term, dead0, 5)
        for t in range(5):
            assert (dones[t] == 1).all() and want[t]["dones"].all(), (p_death, p_term, t)
        for d in deads:
            assert (d == dead_after).all(), (p_death, p_term)
        assert (want[-1]["dead_out"] == bool(dead_after)).all()


# ---- graph replay --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pooled", [("wg33", False), ("wg33_p7", True)])
def test_graph_replays_advance_the_stream(gpu_device, name, pooled):
    """One launch on 33 workgroups (unequal groups) captured into a graph and replayed three times: after an eager launch (step 1 of
    the stream) each replay produces the next launch of the mirror's stream, the counter advances by 1 (step) or P (pool) per replay
    and the tickets are zero after each."""
    shape, P = SR.POOL_SHAPES[name] if pooled else (SR.STEP_SHAPES[name], None)
    N, M, D, S, A = shape
    inc = P or 1
    dfull, dead, cfull, ctr = _state(N, M, _dead0(N, M))
    b = Bufs(N, M, D, S, A, P)
    _launch(b, dead, ctr, _seed(name), pooled=pooled)                   # eager: loads the code object outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _launch(b, dead, ctr, _seed(name), pooled=pooled)
    torch.cuda.synchronize()
    dead_h, ctr_h = _finish(dfull, cfull, N, M)
    assert ctr_h.tolist() == [1 + inc] + [0] * 33                       # the capture itself ran nothing
    mdead, c = _dead0(N, M), 1
    for i in range(4):
        want = SR.pool(_seed(name), c, *shape, P_DEATH, P_TERM, mdead, P) if pooled else SR.step(_seed(name), c, *shape, P_DEATH, P_TERM, mdead)
        mdead, c = want["dead_out"], want["counter"]
        if i > 0:
            g.replay()
            torch.cuda.synchronize()
        got = b.host()
        dead_h, ctr_h = _finish(dfull, cfull, N, M)
        _assert_exact(got, want, f"launch {i}")
        assert _normal_ratio(got, want, f"launch {i}") <= 1.0
        np.testing.assert_array_equal(dead_h, mdead.astype(np.uint8), err_msg=f"dead, launch {i}")
        assert ctr_h.tolist() == [1 + inc * (i + 1)] + [0] * 33, (i, ctr_h.tolist())


# ---- the Python wrapper ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool_steps", [0, 7])
def test_wrapper_hands_out_the_mirrors_stream(gpu_device, pool_steps):
    """SyntheticSMACEnv over 9 steps, one launch per step and in pools of 7: obs, share_obs, the rewards expanded to [N, M, 1], boolean
    dones, the all-false bad flags, avail and env.dead (which the pooled env holds at the end of the current pool) against the mirror."""
    from mappo_amd.envs.synthetic import SyntheticSMACEnv
    N, M, D, S, A, seed, p_death, p_term = 37, 4, 30, 48, 9, 5, 0.05, 0.1
    env = SyntheticSMACEnv(N, num_agents=M, obs_dim=D, share_dim=S, n_actions=A, p_death=p_death, p_term=p_term, seed=seed, pool_steps=pool_steps)
    env.reset()
    want = SR.run(seed, 1, N, M, D, S, A, p_death, p_term, np.zeros((N, M), bool), 14)[0]
    worst = 0.0
    for t in range(9):
        obs, share, rew, dones, bad, avail = env.step(None)
        assert obs.shape == (N, M, D) and share.shape == (N, M, S) and avail.shape == (N, M, A) and rew.shape == (N, M, 1)
        assert dones.shape == (N, M) and dones.dtype == torch.bool and bad.shape == (N, M) and bad.dtype == torch.bool and not bool(bad.any())
        w = want[t]
        got = dict(obs=obs.cpu().numpy(), share=share.cpu().numpy(), rewards=rew[:, 0, 0].cpu().numpy())
        assert bool((rew == rew[:, :1]).all())
        worst = max(worst, _normal_ratio(got, w, f"step {t}"))
        np.testing.assert_array_equal(avail.cpu().numpy(), w["avail"], err_msg=f"avail, step {t}")
        np.testing.assert_array_equal(dones.cpu().numpy(), w["dones"], err_msg=f"dones, step {t}")
        at = t if not pool_steps else (t // pool_steps + 1) * pool_steps - 1
        assert env.dead.dtype == torch.bool
        np.testing.assert_array_equal(env.dead.cpu().numpy(), want[at]["dead_out"], err_msg=f"env.dead, step {t}")
    print(f"pool_steps {pool_steps}: worst |kernel - float64| / bound {worst:.3f}")
    assert worst <= 1.0
