"""simple_spread beyond 3 agents and 3 landmarks on the GPU: mappo_mpe_spread_reset / mappo_mpe_spread_step (csrc/mpe_env.hip,
csrc/mpe_core.h) take M and L at run time, and everything here is held against something that shares no code with them — the
fixture stepped by the reference's own environment at seven shapes (tests/golden/mpe_spread_shapes.npz), the NumPy oracle that
tests/test_mpe_spread_shapes.py pins to it, and the host Philox (tests/mpe_spread_np.py).  Every case is a handful of environments
for six steps."""
import numpy as np
import pytest
import torch

import mpe_spread_np as MS
from conftest import golden, sub
from oracle import mpe_oracle as R

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-6, atol=1e-6)               # the fp32 cast of the outputs: the tolerance of every env test here
SHAPES = [(1, 1), (1, 3), (2, 5), (4, 3), (5, 2), (7, 1), (8, 8)]
SOFT = 3
# The float64 state after every step of the fixture's episodes against the oracle (only exp / log1p differ between the two sides):
# the largest |difference| measured on the MI355X per shape (printed by test_step_follows_the_reference, recorded in DESIGN.md).
# The bound is 100 times the measured figure, the margin of test_gpu_mpe_tag.py, but never below 1e-12 (the precision at which the
# oracle itself is pinned to the reference) and never above 1e-9.  The measured figures are an ulp or a few of coordinates of order
# 1 to 10, so the lower limit decides everywhere: 1e-12.  The fp32 outputs differed from the fp32 cast of the reference's by 0.
STATE_MEASURED = {(1, 1): 0.0, (1, 3): 0.0, (2, 5): 0.0, (4, 3): 1.2e-16, (5, 2): 1.2e-16, (7, 1): 1.8e-15, (8, 8): 8.9e-16}


def state_bound(shape=None):
    measured = max(STATE_MEASURED.values()) if shape is None else STATE_MEASURED[shape]
    return min(max(100.0 * measured, 1e-12), 1e-9)


@pytest.fixture(scope="module")
def fx():
    g = golden("mpe_spread_shapes")
    assert MS.shapes(g) == SHAPES
    return {s: sub(g, "%dx%d" % s) for s in SHAPES}


def _env(N, M, L, T, seed=11):
    from mappo_amd.envs.mpe_spread import SimpleSpreadVecEnv
    return SimpleSpreadVecEnv(N, M, L, T, seed=seed)


def _np(t):
    return t.detach().cpu().numpy()


def _oracle_obs(pos, vel, lpos):
    return np.stack([R.observation(pos[n], vel[n], lpos[n]) for n in range(pos.shape[0])])


# ---- the step kernel against the reference's own episodes -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["onehot", "index"])
@pytest.mark.parametrize("M,L", SHAPES)
def test_step_follows_the_reference(gpu_device, fx, M, L, mode):
    """onehot: every episode in action mode 0 on the rows that were fed to the reference (the probability rows of the soft episode
    included); index: the one-hot episodes in mode 1 on [N, M, 1] indices.  One env with the fixture's episode length (dones and the
    reset at the last step), one that does not end (the observation of the last stepped state, the float64 state at every step)."""
    f = fx[(M, L)]
    rows = np.arange(len(f["kind"])) if mode == "onehot" else np.flatnonzero(f["kind"] != SOFT)
    E, T, D = len(rows), f["obs"].shape[1], 4 + 2 * L + 4 * (M - 1)
    ending, lasting = _env(E, M, L, T), _env(E, M, L, T + 1)
    for env in (ending, lasting):
        env.set_state(f["pos0"][rows], f["vel0"][rows], f["lpos"][rows])
    ref = R.SimpleSpreadRef(f["pos0"][rows], f["vel0"][rows], f["lpos"][rows], T + 1)
    out_worst = state_worst = 0.0
    for t in range(T):
        if mode == "onehot":
            a = torch.from_numpy(f["actions_env"][rows, t].astype(np.float32)).cuda()
            assert tuple(a.shape) == (E, M, 5)
        else:
            a = torch.from_numpy(f["actions"][rows, t].astype(np.float32)).cuda().view(E, M, 1)
        want_obs, want_rew = f["obs"][rows, t].astype(np.float32), f["rewards"][rows, t].astype(np.float32)
        for env in (ending, lasting):
            obs, rew, dones, _ = env.step(a)
            assert tuple(obs.shape) == (E, M, D) and tuple(rew.shape) == (E, M, 1) and dones.dtype == torch.bool
            out_worst = max(out_worst, float(np.abs(_np(rew)[..., 0] - want_rew).max()))
            np.testing.assert_allclose(_np(rew)[..., 0], want_rew, err_msg=f"rewards, step {t}", **TOL)
            if env is ending:
                end_obs = obs
                np.testing.assert_array_equal(_np(dones), f["dones"][rows, t], err_msg=f"dones, step {t}")
            else:
                assert not bool(dones.any())
            if env is lasting or t < T - 1:    # the step that ends the episode returns the observation of the env's own reset state
                out_worst = max(out_worst, float(np.abs(_np(obs) - want_obs).max()))
                np.testing.assert_allclose(_np(obs), want_obs, err_msg=f"obs, step {t}", **TOL)
        ref.step(f["actions_env"][rows, t])
        state_worst = max(state_worst, float(np.abs(_np(lasting.agent_pos) - ref.pos).max()), float(np.abs(_np(lasting.agent_vel) - ref.vel).max()))
        np.testing.assert_array_equal(_np(lasting.landmark_pos), f["lpos"][rows])
    print(f"simple_spread {M} x {L}, {mode}: largest |output - fp32(reference)| {out_worst:.3e}; float64 state against the oracle "
          f"{state_worst:.3e} (bound {state_bound((M, L)):.1e})")
    assert state_worst <= state_bound((M, L))
    # the ended episodes were reset: the env's own draws, at rest, step 0, and the observation returned is that state's
    pos, lpos = MS.reset_draws(11, 1, E, M, L)
    np.testing.assert_array_equal(_np(ending.agent_pos), pos)
    np.testing.assert_array_equal(_np(ending.landmark_pos), lpos)
    assert float(ending.agent_vel.abs().max()) == 0.0 and int(ending.tstep.abs().max()) == 0 and _np(ending.episode).tolist() == [1] * E
    np.testing.assert_array_equal(_np(end_obs), _oracle_obs(pos, np.zeros_like(pos), lpos).astype(np.float32))


# ---- reset against the host Philox ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("M,L", [(1, 1), (3, 3), (5, 2), (8, 8)])
def test_reset_draws_equal_the_host_philox(gpu_device, M, L, N):
    seed, D = 11, 4 + 2 * L + 4 * (M - 1)

    def check(env, seed, episode, obs=None):
        pos, lpos = MS.reset_draws(seed, episode, N, M, L)
        np.testing.assert_array_equal(_np(env.agent_pos), pos, err_msg=f"agent_pos, stream ({seed}, {episode})")
        np.testing.assert_array_equal(_np(env.landmark_pos), lpos, err_msg=f"landmark_pos, stream ({seed}, {episode})")
        assert float(env.agent_vel.abs().max()) == 0.0 and int(env.tstep.abs().max()) == 0
        assert _np(env.episode).tolist() == [episode] * N
        if obs is not None:
            assert tuple(obs.shape) == (N, M, D)
            np.testing.assert_array_equal(_np(obs), _oracle_obs(pos, np.zeros_like(pos), lpos).astype(np.float32))
        return pos, lpos

    env = _env(N, M, L, 25, seed)
    obs = env.reset()
    pos, lpos = check(env, seed, 1, obs)
    assert pos.min() >= -1.0 and pos.max() < 1.0 and np.abs(lpos).max() <= 0.8
    check(env, seed, 2, env.reset())                               # the second reset draws stream (seed, 2)
    # reset-on-done inside the step kernel draws the same way, in either action mode
    for a in (torch.zeros(N, M, 1), torch.eye(5)[torch.zeros(N, M, dtype=torch.long)]):
        e1 = _env(N, M, L, 1, seed)
        o, _, dones, _ = e1.step(a.cuda())
        assert bool(dones.all())
        check(e1, seed, 1, o)
    # the episode counter and the seed are 64-bit numbers: neither upper half may be dropped
    states = {}
    for s, ep in ((3, 5), (2 ** 32 + 3, 5), (3, 2 ** 32 + 5)):
        e = _env(N, M, L, 25, s)
        e.episode.fill_(ep)
        states[(s, ep)] = check(e, s, ep + 1, e.reset())
    for other in ((2 ** 32 + 3, 5), (3, 2 ** 32 + 5)):
        assert not np.array_equal(states[(3, 5)][0], states[other][0]) and not np.array_equal(states[(3, 5)][1], states[other][1])
    # ... and not in the step kernel's reset-on-done either
    e = _env(N, M, L, 1, 2 ** 32 + 3)
    e.episode.fill_(2 ** 32 + 5)
    o, _, _, _ = e.step(torch.zeros(N, M, 1).cuda())
    check(e, 2 ** 32 + 3, 2 ** 32 + 6, o)


# ---- nothing is written outside the environments' slices -------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("M,L", [(1, 1), (8, 8), (5, 2)])
def test_partial_block_writes_nothing_beyond_N(gpu_device, M, L, N):
    """Every state and output array sits in front of a NaN (or sentinel) guard region; reset and both step modes, called directly,
    leave it alone, and the rows below N follow the oracle: N next to the edge of the 256-lane block, with values checked."""
    from mappo_amd import ops
    G, D, seed = 64, 4 + 2 * L + 4 * (M - 1), 11
    f64 = lambda *s: torch.full((N + G, *s), float("nan"), dtype=torch.float64, device="cuda")
    f32 = lambda *s: torch.full((N + G, *s), float("nan"), dtype=torch.float32, device="cuda")
    pos, vel, lpos = f64(M, 2), f64(M, 2), f64(L, 2)
    tstep = torch.full((N + G,), -77, dtype=torch.int32, device="cuda")
    ep = torch.full((N + G,), -77, dtype=torch.int64, device="cuda")
    ep[:N] = 0
    obs, rew = f32(M, D), f32(M)
    dones = torch.full((N + G, M), 9, dtype=torch.uint8, device="cuda")

    def guards(when):
        for name, t in (("pos", pos), ("vel", vel), ("lpos", lpos), ("obs", obs), ("rew", rew)):
            assert bool(torch.isnan(t[N:]).all()), (when, name)
        for name, t in (("tstep", tstep), ("episode", ep)):
            assert bool((t[N:] == -77).all()), (when, name)
        assert bool((dones[N:] == 9).all()), when

    ops.mpe_spread_reset(pos, vel, lpos, tstep, ep, obs, N, M, L, seed)
    guards("reset")
    p0, l0 = MS.reset_draws(seed, 1, N, M, L)
    np.testing.assert_array_equal(_np(pos[:N]), p0)
    np.testing.assert_array_equal(_np(lpos[:N]), l0)
    np.testing.assert_array_equal(_np(obs[:N]), _oracle_obs(p0, np.zeros_like(p0), l0).astype(np.float32))
    assert bool(torch.isnan(rew).all()) and bool((dones == 9).all())                  # the reset has no such outputs
    ref = R.SimpleSpreadRef(p0, np.zeros_like(p0), l0, 2)
    idx = ((torch.arange(N)[:, None] + torch.arange(M)[None, :]) % 5).float().cuda().contiguous()
    # first step: index actions; episode length 2, so nothing ends
    ops.mpe_spread_step(pos, vel, lpos, tstep, ep, idx, 1, obs, rew, dones, N, M, L, 2, seed)
    guards("index step")
    o_ref, r_ref, d_ref = ref.step(np.eye(5)[_np(idx).astype(np.int64)])
    np.testing.assert_allclose(_np(obs[:N]), o_ref, **TOL)
    np.testing.assert_allclose(_np(rew[:N]), r_ref[..., 0], **TOL)
    assert not d_ref.any() and bool((dones[:N] == 0).all()) and _np(tstep[:N]).tolist() == [1] * N
    np.testing.assert_allclose(_np(pos[:N]), ref.pos, rtol=0, atol=state_bound())
    np.testing.assert_allclose(_np(vel[:N]), ref.vel, rtol=0, atol=state_bound())
    # second step: one-hot actions; every episode ends and is reset inside the launch
    onehot = torch.eye(5, device="cuda")[idx.long()].contiguous()
    ops.mpe_spread_step(pos, vel, lpos, tstep, ep, onehot, 0, obs, rew, dones, N, M, L, 2, seed)
    guards("one-hot step")
    p1, l1 = MS.reset_draws(seed, 2, N, M, L)
    _, r_ref, d_ref = ref.step(_np(onehot).astype(np.float64), lambda n: (p1[n], np.zeros_like(p1[n]), l1[n]))
    np.testing.assert_allclose(_np(rew[:N]), r_ref[..., 0], **TOL)
    assert d_ref.all() and bool((dones[:N] == 1).all())
    assert _np(ep[:N]).tolist() == [2] * N and _np(tstep[:N]).tolist() == [0] * N
    np.testing.assert_array_equal(_np(pos[:N]), p1)
    np.testing.assert_array_equal(_np(lpos[:N]), l1)
    assert float(vel[:N].abs().max()) == 0.0
    np.testing.assert_array_equal(_np(obs[:N]), _oracle_obs(p1, np.zeros_like(p1), l1).astype(np.float32))
    for name, t in (("pos", pos), ("vel", vel), ("lpos", lpos), ("obs", obs), ("rew", rew)):
        assert bool(torch.isfinite(t[:N]).all()), name


# ---- index actions outside 0 .. 4 -----------------------------------------------------------------------------------------------------------
def test_index_actions_outside_the_moves_apply_no_force(gpu_device, fx):
    """The rule stated in include/mappo_hip.h: the fp32 index is truncated towards zero to an int, and only 1 .. 4 move the agent.
    -3, 9 and 0 are the same action (no clamp to the nearest move, unlike simple_tag), 2.7 is 2, 4.9 is 4, -0.9 is 0."""
    M, L = 5, 2
    f = fx[(M, L)]
    E = len(f["kind"])

    def run(row):
        env = _env(E, M, L, 25)
        env.set_state(f["pos0"], f["vel0"], f["lpos"])
        obs, rew, dones, _ = env.step(torch.tensor([row] * E, dtype=torch.float32).cuda().view(E, M, 1))
        return obs.clone(), rew.clone(), dones.clone(), env.agent_pos.clone(), env.agent_vel.clone()

    def same(x, y):
        return all(torch.equal(a, b) for a, b in zip(x, y))

    still = run([0.0, 0.0, 0.0, 0.0, 0.0])
    assert same(run([-3.0, 9.0, 0.0, 5.0, -1.0]), still)
    assert same(run([-0.9, 0.9, -3.5, 1e9, -1e9]), still)
    moves = run([2.0, 2.0, 4.0, 1.0, 3.0])
    assert same(run([2.7, 2.0, 4.9, 1.5, 3.999]), moves)
    assert not torch.equal(moves[4], still[4])                                        # the moves do act
    # and 2 is what the one-hot of 2 does
    env = _env(E, M, L, 25)
    env.set_state(f["pos0"], f["vel0"], f["lpos"])
    onehot = torch.eye(5)[torch.tensor([[2, 2, 4, 1, 3]] * E)].cuda()
    obs, rew, dones, _ = env.step(onehot)
    assert same((obs, rew, dones, env.agent_pos, env.agent_vel), moves)
