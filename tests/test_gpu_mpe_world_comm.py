"""GPU-vectorised MPE simple_world_comm: the env kernel (csrc/mpe_world_comm_env.hip) against the fixture stepped by the reference's
own environment (tests/golden/mpe_world_comm.npz) — float outputs within 1e-6 of the fp32 cast, the in_forest flags, the zeros of
hidden agents, the leader's word and the dones EQUAL —, in both action modes, across reset-on-done, at the block edges N = 1 / 255 /
256 / 257, and the entry points' refusals on live device memory."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
import mpe_world_comm_np as MW

pytestmark = pytest.mark.gpu

OBS = MW.OBS
TOL = dict(rtol=1e-6, atol=1e-6)      # tests/test_gpu_mpe_tag.py's: the same softplus term and bound() through the device's exp / log1p
MODES = ["onehot_list", "index_list", "index_tensor"]


def _fx(tag):
    g = golden("mpe_world_comm")
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}


def _env(N, T=10, seed=3):
    from mappo_amd.envs import SimpleWorldCommVecEnv
    return SimpleWorldCommVecEnv(N, episode_length=T, seed=seed)


def _np(t):
    return t.detach().cpu().numpy()


def _act(a, mode):
    """Recorded indices [N, 7] (leader move, leader word, agents 1..5) in one of the forms step() takes."""
    if mode == "onehot_list":
        return [torch.from_numpy(x.astype(np.float32)).cuda() for x in MW.onehots(a)]
    if mode == "index_list":
        return [torch.from_numpy(a[:, :2].astype(np.float32)).cuda()] + [torch.from_numpy(a[:, 2 + m].astype(np.float32)).cuda() for m in range(5)]
    return torch.from_numpy(a.astype(np.float32)).cuda()


def _check_obs(got, want64, m, what):
    """One agent's observation [N, D] against the reference's float64: the floats within TOL of the fp32 cast; the in_forest flags,
    the hidden agents' zeros (exactly where the reference has them, nowhere else) and the leader's word equal."""
    want = want64.astype(np.float32)
    np.testing.assert_allclose(got, want, err_msg=what, **TOL)
    adv = m < MW.ADV
    np.testing.assert_array_equal(got[:, MW.IN_FOREST[adv]], want[:, MW.IN_FOREST[adv]], err_msg=what + ": in_forest")
    assert set(np.unique(got[:, MW.IN_FOREST[adv]])) <= {-1.0, 1.0}
    for sl in (MW.OTHER_POS, MW.OTHER_VEL[adv]):
        # (the fp32 cast: a visible agent's velocity of 1e-169 is a zero in fp32 on both sides)
        np.testing.assert_array_equal(got[:, sl] == 0, want[:, sl] == 0, err_msg=what + ": zeros of hidden entries")
    if adv:
        np.testing.assert_array_equal(got[:, MW.COMM], want[:, MW.COMM], err_msg=what + ": the leader's word")
    return float(np.abs(got - want).max())


# ---- the env kernel against the fixture -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_runs(gpu_device):
    """The fixture's 8 episodes x 10 steps in every action form: per mode, per step (obs, rewards, dones) and the state after it."""
    g = _fx("long")
    E, T = g["actions"].shape[:2]
    out = {}
    for mode in MODES:
        env = _env(E, T=T)
        env.set_state(g["pos0"], g["vel0"], g["lpos"])
        steps = []
        for t in range(T):
            obs, rew, dones, _ = env.step(_act(g["actions"][:, t], mode))
            assert dones.dtype == torch.bool and tuple(rew.shape) == (E, 6, 1)
            steps.append(([o.clone() for o in obs], rew.clone(), dones.clone(), {k: v.clone() for k, v in env.state_tensors().items()}))
        out[mode] = steps
    return g, out


@pytest.mark.parametrize("mode", MODES)
def test_fixture_parity_long_episodes(long_runs, mode):
    g, runs = long_runs
    E, T = g["actions"].shape[:2]
    worst = 0.0
    for t, (obs, rew, dones, state) in enumerate(runs[mode]):
        np.testing.assert_array_equal(_np(dones), g["dones"][:, t], err_msg=f"dones, step {t}")
        # the last step ends the episode: its rewards are the ended step's, its observations the env's own reset state's (checked in
        # test_fixture_parity_across_reset_on_done); the stepped float64 state is held against the mirror in the test below
        for m in range(6 if t < T - 1 else 0):
            worst = max(worst, _check_obs(_np(obs[m]), g["obs_" + OBS[m]][:, t], m, f"obs of agent {m}, step {t}"))
        want = g["rewards"][:, t].astype(np.float32)
        worst = max(worst, float(np.abs(_np(rew)[..., 0] - want).max()))
        np.testing.assert_allclose(_np(rew)[..., 0], want, err_msg=f"rewards, step {t}", **TOL)
        if t < T - 1:
            np.testing.assert_array_equal(_np(state["landmark_pos"]), g["lpos"])
    print(f"{mode}: largest |output - fp32(reference)| over the {T} steps: {worst:.3e}")
    last = runs[mode][-1][3]
    assert int(last["tstep"].abs().max()) == 0 and _np(last["episode"]).tolist() == [1] * E      # every episode ended and was reset


def test_both_action_modes_give_identical_outputs_and_states(long_runs):
    _, runs = long_runs
    ref = runs["onehot_list"]
    for mode in ("index_list", "index_tensor"):
        for t, (a, b) in enumerate(zip(ref, runs[mode])):
            for m in range(6):
                assert torch.equal(a[0][m], b[0][m]), (mode, t, m)
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (mode, t)
            for k in a[3]:
                assert torch.equal(a[3][k], b[3][k]), (mode, t, k)


def test_float64_state_follows_the_mirror(gpu_device):
    """The float64 state along the fixture's episodes — contacts, clamps and the arena's edge included — against the NumPy mirror
    (which equals the reference).  Only exp and log1p differ between the two; a contact force is 1e2 x a softplus term of order 1e-3
    times dt 0.1 twice, so an ulp or two of a double there moves a coordinate by far less than 1e-12."""
    g = _fx("long")
    E, T = g["actions"].shape[:2]
    env = _env(E, T=T + 1)
    env.set_state(g["pos0"], g["vel0"], g["lpos"])
    mirror = MW.SimpleWorldCommNp(g["pos0"], g["vel0"], g["lpos"], episode_length=T + 1)
    worst = 0.0
    for t in range(T):
        env.step(_act(g["actions"][:, t], "index_tensor"))
        mirror.step(g["actions"][:, t])
        worst = max(worst, float(np.abs(_np(env.agent_pos) - mirror.pos).max()), float(np.abs(_np(env.agent_vel) - mirror.vel).max()))
    np.testing.assert_array_equal(mirror.pos, g["pos1"])
    print(f"float64 state against the mirror: largest difference at any step {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("mode", ["onehot_list", "index_tensor"])
def test_fixture_parity_across_reset_on_done(gpu_device, mode):
    """episode_length 5, 10 steps.  Rewards and dones follow the fixture's at every step, the ending ones included; a step that ends
    an episode returns the observation of the env's OWN reset state (its Philox draws, not NumPy's): agents in [-1, 1]^2, landmarks
    in [-0.8, 0.8]^2, at rest, nothing said, step 0; the fixture's reset state is then loaded and the second episode must follow the
    fixture again."""
    g = _fx("short")
    E = 2
    env = _env(E, T=5, seed=5)
    env.set_state(g["pos0"], g["vel0"], g["lpos"])
    resets = 0
    for t in range(10):
        obs, rew, dones, _ = env.step(_act(g["actions"][:, t], mode))
        np.testing.assert_array_equal(_np(dones), g["dones"][:, t])
        np.testing.assert_allclose(_np(rew)[..., 0], g["rewards"][:, t].astype(np.float32), err_msg=f"rewards, step {t}", **TOL)
        if g["dones"][:, t].all():
            resets += 1
            assert int(env.tstep.abs().max()) == 0 and _np(env.episode).tolist() == [resets] * E and float(env.agent_vel.abs().max()) == 0.0
            assert float(env.agent_pos.abs().max()) <= 1.0 and float(env.landmark_pos.abs().max()) <= 0.8
            pos, lpos = MW.reset_draws(5, resets, E)
            np.testing.assert_array_equal(_np(env.agent_pos), pos)
            np.testing.assert_array_equal(_np(env.landmark_pos), lpos)
            want = MW.observation(pos, np.zeros_like(pos), lpos, np.zeros((E, 4)))
            for m in range(6):
                np.testing.assert_array_equal(_np(obs[m]), want[m].astype(np.float32), err_msg=f"reset obs of agent {m}")
                assert float(obs[m][:, 0:2].abs().max()) == 0.0
                if m < MW.ADV:
                    assert float(obs[m][:, MW.COMM].abs().max()) == 0.0
            k = resets - 1
            env.set_state(g["reset_pos"][:, k], np.zeros((E, 6, 2)), g["reset_lpos"][:, k])
        else:
            for m in range(6):
                _check_obs(_np(obs[m]), g["obs_" + OBS[m]][:, t], m, f"obs of agent {m}, step {t}")
    assert resets == 2


def test_index_actions_are_clamped(gpu_device):
    a, b = _env(4), _env(4)
    a.reset(); b.reset()
    oa, ra, _, _ = a.step(torch.tensor([[-3.0, 9.0, 9.0, 4.0, 5.0, -1.0, 2.0]] * 4).cuda())
    ob, rb, _, _ = b.step(torch.tensor([[0.0, 3.0, 4.0, 4.0, 4.0, 0.0, 2.0]] * 4).cuda())
    assert all(torch.equal(x, y) for x, y in zip(oa, ob)) and torch.equal(ra, rb)
    assert torch.equal(a.agent_pos, b.agent_pos) and torch.equal(a.agent_vel, b.agent_vel)
    assert _np(oa[1][:, MW.COMM]).tolist() == [[0.0, 0.0, 0.0, 1.0]] * 4


# ---- reset ----------------------------------------------------------------------------------------------------------------------------------
def test_reset_draws_equal_the_host_philox(gpu_device):
    N, seed = 37, 11
    env = _env(N, seed=seed)
    obs = env.reset()
    pos, lpos = MW.reset_draws(seed, 1, N)
    np.testing.assert_array_equal(_np(env.agent_pos), pos)
    np.testing.assert_array_equal(_np(env.landmark_pos), lpos)
    assert float(env.agent_pos.min()) >= -1.0 and float(env.agent_pos.max()) < 1.0 and float(env.landmark_pos.abs().max()) <= 0.8
    assert float(env.agent_vel.abs().max()) == 0.0 and _np(env.episode).tolist() == [1] * N and int(env.tstep.abs().max()) == 0
    want = MW.observation(pos, np.zeros_like(pos), lpos, np.zeros((N, 4)))
    for m in range(6):
        assert tuple(obs[m].shape) == (N, MW.OBS_DIMS[m])
        np.testing.assert_array_equal(_np(obs[m]), want[m].astype(np.float32))
    env.reset()                                                    # the second reset draws stream (seed, 2)
    np.testing.assert_array_equal(_np(env.agent_pos), MW.reset_draws(seed, 2, N)[0])
    # reset-on-done inside step() draws the same way
    e2 = _env(N, T=1, seed=seed)
    e2.step(torch.zeros(N, 7).cuda())
    np.testing.assert_array_equal(_np(e2.agent_pos), pos)
    np.testing.assert_array_equal(_np(e2.landmark_pos), lpos)


# ---- block edges ---------------------------------------------------------------------------------------------------------------------------
def _tiled(g, N):
    rows = np.arange(N) % g["pos0"].shape[0]
    return rows, g["pos0"][rows], g["vel0"][rows], g["lpos"][rows]


@pytest.fixture(scope="module")
def single_lanes(gpu_device):
    """Each of the fixture's 8 start states stepped alone (N = 1) through its first 4 recorded actions: {row: [per step (obs, rew,
    dones, state)]}."""
    g = _fx("long")
    out = {}
    for e in range(g["pos0"].shape[0]):
        env = _env(1, T=50)
        env.set_state(g["pos0"][e:e + 1], g["vel0"][e:e + 1], g["lpos"][e:e + 1])
        steps = []
        for t in range(4):
            obs, rew, dones, _ = env.step(_act(g["actions"][e:e + 1, t], "index_tensor"))
            steps.append(([o.clone() for o in obs], rew.clone(), dones.clone(), env.agent_pos.clone(), env.agent_vel.clone()))
        out[e] = steps
    return g, out


@pytest.mark.parametrize("N", [255, 256, 257])
def test_block_edges_match_the_same_states_at_N_1(single_lanes, N):
    """One lane per env in 256-lane blocks: the last lanes of the first block and the first lanes of the second compute what the same
    state computes alone at N = 1, bit for bit (no episode ends here, so no draw depends on the lane)."""
    g, single = single_lanes
    rows, pos, vel, lpos = _tiled(g, N)
    env = _env(N, T=50)
    env.set_state(pos, vel, lpos)
    lanes = sorted({0, 1, 253, 254, N - 1} | ({255} if N > 255 else set()) | ({256} if N > 256 else set()))
    for t in range(4):
        obs, rew, dones, _ = env.step(_act(g["actions"][rows, t], "index_tensor"))
        assert not bool(dones.any())
        for n in lanes:
            so, sr, sd, sp, sv = single[int(rows[n])][t]
            for m in range(6):
                assert torch.equal(obs[m][n], so[m][0]), (N, t, n, m)
            assert torch.equal(rew[n], sr[0]) and torch.equal(env.agent_pos[n], sp[0]) and torch.equal(env.agent_vel[n], sv[0]), (N, t, n)


@pytest.mark.parametrize("N", [1, 255, 257])
def test_partial_block_writes_nothing_beyond_N(gpu_device, N):
    """Every output and state array sits in front of a NaN (or sentinel) guard region; reset and both step modes leave it alone."""
    from mappo_amd import ops
    G = 64
    f64 = lambda *s: torch.full((N + G, *s), float("nan"), dtype=torch.float64, device="cuda")
    f32 = lambda *s: torch.full((N + G, *s), float("nan"), dtype=torch.float32, device="cuda")
    pos, vel, lpos = f64(6, 2), f64(6, 2), f64(5, 2)
    tstep = torch.full((N + G,), -77, dtype=torch.int32, device="cuda")
    ep = torch.full((N + G,), -77, dtype=torch.int64, device="cuda")
    ep[:N] = 0
    obs, rew = [f32(d) for d in MW.OBS_DIMS], f32(6)
    dones = torch.full((N + G, 6), 9, dtype=torch.uint8, device="cuda")
    ops.mpe_world_comm_reset(pos, vel, lpos, tstep, ep, obs, N, 11)
    idx = torch.stack([(torch.arange(N) + m) % (4 if m == 1 else 5) for m in range(7)], dim=1).float().cuda().contiguous()
    ops.mpe_world_comm_step(pos, vel, lpos, tstep, ep, idx, 1, obs, rew, dones, N, 2, 11)
    hot = [x.cuda().contiguous() for x in (torch.from_numpy(h.astype(np.float32)) for h in MW.onehots(_np(idx)))]
    ops.mpe_world_comm_step(pos, vel, lpos, tstep, ep, hot, 0, obs, rew, dones, N, 2, 11)
    torch.cuda.synchronize()
    for name, t in [("pos", pos), ("vel", vel), ("lpos", lpos), ("rew", rew)] + [(f"obs{m}", o) for m, o in enumerate(obs)]:
        assert bool(torch.isnan(t[N:]).all()), name
        assert bool(torch.isfinite(t[:N]).all()), name
    for name, t in (("tstep", tstep), ("episode", ep)):
        assert bool((t[N:] == -77).all()), name
    assert bool((dones[N:] == 9).all()) and bool((dones[:N] == 1).all())                            # episode length 2: done at the second step
    assert _np(ep[:N]).tolist() == [2] * N and _np(tstep[:N]).tolist() == [0] * N


# ---- the entry points refuse before they launch ---------------------------------------------------------------------------------------------
def test_bad_arguments_return_einval_and_launch_nothing(gpu_device):
    """Null pointers, N = 0, a bad mode and a wrong num_agents on LIVE device memory: MAPPO_EINVAL with a message, and every state
    and output tensor keeps its sentinel."""
    from mappo_amd import _lib
    lib = _lib.load()
    N = 8
    pos, vel, lpos = (torch.full((N, k, 2), 7.0, dtype=torch.float64, device="cuda") for k in (6, 6, 5))
    tstep = torch.full((N,), 3, dtype=torch.int32, device="cuda")
    ep = torch.full((N,), 5, dtype=torch.int64, device="cuda")
    obs = [torch.full((N, d), 7.0, device="cuda") for d in MW.OBS_DIMS]
    rew, dones = torch.full((N, 6), 7.0, device="cuda"), torch.full((N, 6), 7, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(N, 7, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    arr = lambda ts: (C.c_void_p * 6)(*[None if t is None else t.data_ptr() for t in ts])
    state = [p(pos), p(vel), p(lpos), p(tstep), p(ep)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def step(state=state, act=arr([idx] + [None] * 5), mode=1, o=arr(obs), r=p(rew), d=p(dones), n=N, M=6, L=1, T=25):
        return lib.mappo_mpe_world_comm_step(*state, act, mode, o, r, d, n, M, L, T, 1, stream), lib.mappo_last_error().decode()

    def reset(state=state, o=arr(obs), n=N, M=6, L=1):
        return lib.mappo_mpe_world_comm_reset(*state, o, n, M, L, 1, stream), lib.mappo_last_error().decode()

    bad = [(step, dict(n=0), "N=0"), (step, dict(mode=2), "action_mode 2"), (step, dict(M=4), "num_agents=4"), (step, dict(M=7), "num_agents=7"),
           (step, dict(L=3), "num_landmarks=3"), (step, dict(state=[None] + state[1:]), "null pointer"), (step, dict(act=None), "null pointer"),
           (step, dict(act=arr([None] * 6)), "null pointer"), (step, dict(act=arr([idx] + [None] * 5), mode=0), "null pointer"),
           (step, dict(o=arr(obs[:5] + [None])), "null pointer"), (step, dict(r=None), "null pointer"), (step, dict(d=None), "null pointer"),
           (step, dict(T=0), "episode length 0"),
           (reset, dict(n=0), "N=0"), (reset, dict(M=5), "num_agents=5"), (reset, dict(L=0), "num_landmarks=0"),
           (reset, dict(state=state[:4] + [None]), "null pointer"), (reset, dict(o=None), "null pointer"),
           (reset, dict(o=arr([None] + obs[1:])), "null pointer")]
    for call, kw, word in bad:
        rc, err = call(**kw)
        assert rc == -1 and word in err and "mpe_world_comm_" in err, (kw, rc, err)
    torch.cuda.synchronize()
    for t in [pos, vel, lpos, rew] + obs:
        assert bool((t == 7.0).all())
    assert bool((tstep == 3).all()) and bool((ep == 5).all()) and bool((dones == 7).all())
    rc, err = step()                                               # and the valid call goes through
    assert rc == 0, err
    torch.cuda.synchronize()
    assert bool((tstep == 4).all()) and bool((dones == 0).all())
