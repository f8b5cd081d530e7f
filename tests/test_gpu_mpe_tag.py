"""GPU-vectorised MPE simple_tag: the env kernel (csrc/mpe_ragged_env.hip) against the fixture stepped by the reference's own
environment (tests/golden/mpe_tag.npz) — outputs within 1e-6 of the fp32 cast, the float64 state against the NumPy mirror —, its
reset against the host Philox, and the separated runner's stepwise path on four agents of two observation widths and per-agent
rewards."""
import numpy as np
import pytest
import torch

from conftest import golden
import mpe_tag_np as MT

pytestmark = pytest.mark.gpu

OBS = MT.OBS
TOL = dict(rtol=1e-6, atol=1e-6)      # tests/test_mpe_env.py's, for simple_spread: the same softplus term through the device's exp / log1p
# The float64 state along the fixture's 25-step episodes against the mirror: measured on the MI355X (printed by
# test_float64_state_follows_the_mirror, recorded in DESIGN.md), times 100, the rule the scenario's specification sets.  The measured
# figure is so small — one far-field tail of the softplus, on a force of ~1e-60 — that on coordinates of order 1 the bound MEANS
# EQUALITY to the bit with NumPy's exp / log1p along every trajectory; the factor 100 buys no room for another contact geometry.  If
# this test fails after an update of the device math library by one ulp inside a contact, that is what it has seen: measure again
# and record the new figure, the kernel need not be wrong.
STATE_MEASURED = 1.9e-65          # 0 at the end of every episode; 1.899e-65 at one intermediate step
STATE_BOUND = 100 * STATE_MEASURED
assert STATE_BOUND < 1e-9


def _fx(tag):
    g = golden("mpe_tag")
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}


def _env(N, T=25, seed=3):
    from mappo_amd.envs import SimpleTagVecEnv
    return SimpleTagVecEnv(N, episode_length=T, seed=seed)


def _np(t):
    return t.detach().cpu().numpy()


def _act(a, mode):
    """Recorded indices [N, 4] in one of the forms step() takes."""
    if mode == "onehot":
        return torch.eye(5)[torch.from_numpy(a.astype(np.int64))].cuda()
    if mode == "onehot_list":
        return [torch.eye(5)[torch.from_numpy(a[:, m].astype(np.int64))].cuda() for m in range(4)]
    if mode == "index_list":
        return [torch.from_numpy(a[:, m].astype(np.float32)).cuda() for m in range(4)]
    return torch.from_numpy(a.astype(np.float32)).cuda()


MODES = ["onehot", "onehot_list", "index_list", "index_tensor"]


# ---- the env kernel against the fixture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_fixture_parity_long_episodes(gpu_device, mode):
    g = _fx("long")
    E, T = 12, 25
    env = _env(E, T=T)
    env.set_state(g["pos0"], g["vel0"], g["lpos"])
    worst = 0.0
    for t in range(T):
        obs, rew, dones, _ = env.step(_act(g["actions"][:, t], mode))
        assert dones.dtype == torch.bool
        np.testing.assert_array_equal(_np(dones), g["dones"][:, t], err_msg=f"dones, step {t}")
        # the last step ends the episode: its rewards are the ended step's, its observations the env's own reset state's (checked in
        # test_fixture_parity_across_reset_on_done); the stepped float64 state is held against pos1 / vel1 in the test below
        for m in range(4 if t < T - 1 else 0):
            want = g["obs_" + OBS[m]][:, t].astype(np.float32)
            worst = max(worst, float(np.abs(_np(obs[m]) - want).max()))
            np.testing.assert_allclose(_np(obs[m]), want, err_msg=f"obs of agent {m}, step {t}", **TOL)
        want = g["rewards"][:, t].astype(np.float32)
        worst = max(worst, float(np.abs(_np(rew)[..., 0] - want).max()))
        np.testing.assert_allclose(_np(rew)[..., 0], want, err_msg=f"rewards, step {t}", **TOL)
        assert tuple(rew.shape) == (E, 4, 1)
        if t < T - 1:
            np.testing.assert_array_equal(_np(env.landmark_pos), g["lpos"])
    print(f"{mode}: largest |output - fp32(reference)| over the 25 steps: {worst:.3e}")
    assert int(env.tstep.abs().max()) == 0 and _np(env.episode).tolist() == [1] * E      # every episode ended on step 25 and was reset


def test_float64_state_follows_the_mirror(gpu_device):
    """The state after the fixture's 25 steps — contacts, clamps and the arena's edge included — in float64 against the NumPy mirror
    (which equals the reference).  Only exp and log1p differ between the two."""
    g = _fx("long")
    env = _env(12, T=26)
    env.set_state(g["pos0"], g["vel0"], g["lpos"])
    mirror = MT.SimpleTagNp(g["pos0"], g["vel0"], g["lpos"], episode_length=26)
    worst = 0.0
    for t in range(25):
        env.step(_act(g["actions"][:, t], "index_tensor"))
        mirror.step(g["actions"][:, t])
        worst = max(worst, float(np.abs(_np(env.agent_pos) - mirror.pos).max()), float(np.abs(_np(env.agent_vel) - mirror.vel).max()))
    np.testing.assert_array_equal(mirror.pos, g["pos1"])
    dev = max(float(np.abs(_np(env.agent_pos) - g["pos1"]).max()), float(np.abs(_np(env.agent_vel) - g["vel1"]).max()))
    print(f"float64 state against the mirror: end of episode {dev:.3e}, largest at any step {worst:.3e} (bound {STATE_BOUND:.1e})")
    assert max(dev, worst) <= STATE_BOUND


@pytest.mark.parametrize("mode", ["onehot", "index_tensor"])
def test_fixture_parity_across_reset_on_done(gpu_device, mode):
    """episode_length 7, 14 steps.  Rewards and dones follow the fixture's at every step, the ending ones included; a step that ends
    an episode returns the observation of the env's OWN reset state (its Philox draws, not NumPy's), at rest, step 0; the fixture's
    reset state is then loaded and the second episode must follow the fixture again."""
    g = _fx("short")
    E = 2
    env = _env(E, T=7, seed=5)
    env.set_state(g["pos0"], g["vel0"], g["lpos"])
    resets = 0
    for t in range(14):
        obs, rew, dones, _ = env.step(_act(g["actions"][:, t], mode))
        np.testing.assert_array_equal(_np(dones), g["dones"][:, t])
        np.testing.assert_allclose(_np(rew)[..., 0], g["rewards"][:, t].astype(np.float32), err_msg=f"rewards, step {t}", **TOL)
        if g["dones"][:, t].all():
            resets += 1
            assert int(env.tstep.abs().max()) == 0 and _np(env.episode).tolist() == [resets] * E and float(env.agent_vel.abs().max()) == 0.0
            want = MT.observation(_np(env.agent_pos), _np(env.agent_vel), _np(env.landmark_pos))
            for m in range(4):
                np.testing.assert_array_equal(_np(obs[m]), want[m].astype(np.float32), err_msg=f"reset obs of agent {m}")
            k = resets - 1
            env.set_state(g["reset_pos"][:, k], np.zeros((E, 4, 2)), g["reset_lpos"][:, k])
        else:
            for m in range(4):
                np.testing.assert_allclose(_np(obs[m]), g["obs_" + OBS[m]][:, t].astype(np.float32), err_msg=f"obs of agent {m}, step {t}", **TOL)
    assert resets == 2


def test_index_actions_are_clamped(gpu_device):
    a, b = _env(4), _env(4)
    a.reset(); b.reset()
    oa, ra, _, _ = a.step(torch.tensor([[-3.0, 9.0, 4.0, 5.0]] * 4).cuda())
    ob, rb, _, _ = b.step(torch.tensor([[0.0, 4.0, 4.0, 4.0]] * 4).cuda())
    assert all(torch.equal(x, y) for x, y in zip(oa, ob)) and torch.equal(ra, rb)
    assert torch.equal(a.agent_pos, b.agent_pos) and torch.equal(a.agent_vel, b.agent_vel)


# ---- reset ----------------------------------------------------------------------------------------------------------------------------------
def test_reset_draws_equal_the_host_philox(gpu_device):
    N, seed = 37, 11
    env = _env(N, seed=seed)
    obs = env.reset()
    pos, lpos = MT.reset_draws(seed, 1, N)
    np.testing.assert_array_equal(_np(env.agent_pos), pos)
    np.testing.assert_array_equal(_np(env.landmark_pos), lpos)
    assert float(env.agent_pos.min()) >= -1.0 and float(env.agent_pos.max()) < 1.0 and float(env.landmark_pos.abs().max()) <= 0.8
    assert float(env.agent_vel.abs().max()) == 0.0 and _np(env.episode).tolist() == [1] * N and int(env.tstep.abs().max()) == 0
    want = MT.observation(pos, np.zeros_like(pos), lpos)
    for m in range(4):
        assert tuple(obs[m].shape) == (N, MT.OBS_DIMS[m])
        np.testing.assert_array_equal(_np(obs[m]), want[m].astype(np.float32))
    env.reset()                                                    # the second reset draws stream (seed, 2)
    np.testing.assert_array_equal(_np(env.agent_pos), MT.reset_draws(seed, 2, N)[0])
    # reset-on-done inside step() draws the same way
    e2 = _env(N, T=1, seed=seed)
    e2.step(torch.zeros(N, 4).cuda())
    np.testing.assert_array_equal(_np(e2.agent_pos), pos)
    np.testing.assert_array_equal(_np(e2.landmark_pos), lpos)


@pytest.mark.parametrize("N", [1, 37])
def test_partial_block_writes_nothing_beyond_N(gpu_device, N):
    """Every output and state array sits in front of a NaN (or sentinel) guard region; reset and both step modes leave it alone."""
    from mappo_amd import ops
    G = 64
    f64 = lambda *s: torch.full((N + G, *s), float("nan"), dtype=torch.float64, device="cuda")
    f32 = lambda *s: torch.full((N + G, *s), float("nan"), dtype=torch.float32, device="cuda")
    pos, vel, lpos = f64(4, 2), f64(4, 2), f64(2, 2)
    tstep = torch.full((N + G,), -77, dtype=torch.int32, device="cuda")
    ep = torch.full((N + G,), -77, dtype=torch.int64, device="cuda")
    ep[:N] = 0
    o0, o1, o2, o3, rew = f32(16), f32(16), f32(16), f32(14), f32(4)
    dones = torch.full((N + G, 4), 9, dtype=torch.uint8, device="cuda")
    ops.mpe_tag_reset(pos, vel, lpos, tstep, ep, o0, o1, o2, o3, N, 11)
    idx = torch.stack([(torch.arange(N) + m) % 5 for m in range(4)], dim=1).float().cuda().contiguous()
    ops.mpe_tag_step(pos, vel, lpos, tstep, ep, idx, 1, o0, o1, o2, o3, rew, dones, N, 2, 11)
    ops.mpe_tag_step(pos, vel, lpos, tstep, ep, torch.eye(5, device="cuda")[idx.long()].contiguous(), 0, o0, o1, o2, o3, rew, dones, N, 2, 11)
    torch.cuda.synchronize()
    for name, t in (("pos", pos), ("vel", vel), ("lpos", lpos), ("o0", o0), ("o1", o1), ("o2", o2), ("o3", o3), ("rew", rew)):
        assert bool(torch.isnan(t[N:]).all()), name
        assert bool(torch.isfinite(t[:N]).all()), name
    for name, t in (("tstep", tstep), ("episode", ep)):
        assert bool((t[N:] == -77).all()), name
    assert bool((dones[N:] == 9).all()) and bool((dones[:N] == 1).all())                            # episode length 2: done at the second step
    assert _np(ep[:N]).tolist() == [2] * N and _np(tstep[:N]).tolist() == [0] * N


# ---- the separated runner ---------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    from mappo_amd.config import get_config
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = False
    a.use_naive_recurrent_policy = False
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def test_runner_trains_four_agents_stepwise(gpu_device, monkeypatch):
    """N = 16, T = 5, two iterations on the stepwise path: the four agents are collected through mappo_rollout_step on their own
    widths, the first rollout's stored observations and per-agent rewards follow the mirror stepped on the stored actions, every
    buffer stays finite and each agent's actor and critic change."""
    from mappo_amd.runner.separated.mpe_runner import MPERunner
    monkeypatch.setenv("MAPPO_TAG_EPISODE", "0")
    N, T = 16, 5
    env = _env(N, T)
    a = _args(episode_length=T, n_rollout_threads=N, env_name="MPE", share_policy=False, use_hip_graph=False, seed=1, algorithm_name="mappo",
              ppo_epoch=2, num_mini_batch=1)
    torch.manual_seed(1)
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=4, device=torch.device("cuda"), run_dir=None))
    assert r._ragged and r._fused_ff()
    assert [p.actor.desc.in_dim for p in r.policy] == [16, 16, 16, 14] and [p.critic.desc.in_dim for p in r.policy] == [62] * 4
    r.warmup()
    state0 = {k: _np(v).copy() for k, v in env.state_tensors().items()}
    before = [p.flat_params.clone() for p in r.policy]
    names = ("share_obs", "obs", "value_preds", "returns", "actions", "action_log_probs", "rewards", "masks")
    for it in range(2):
        r.rollout()
        if it == 0:
            first = [{n: getattr(b, n).clone() for n in names} for b in r.buffer]
            end = {k: _np(v).copy() for k, v in env.state_tensors().items()}
        for m, b in enumerate(r.buffer):
            for n in names:
                assert bool(torch.isfinite(getattr(b, n)).all()), (it, m, n)
        infos = r.train()
        assert len(infos) == 4
        for m, info in enumerate(infos):
            for k, v in info.items():
                assert np.isfinite(float(v)), (it, m, k, v)
    for m, p in enumerate(r.policy):
        a0, a1 = before[m][:p.actor.n_params], p.flat_params[:p.actor.n_params]
        lo = p.seg_bounds[1]
        c0, c1 = before[m][lo:lo + p.critic.n_params], p.flat_params[lo:lo + p.critic.n_params]
        assert not torch.equal(a0, a1) and not torch.equal(c0, c1), f"agent {m}: parameters did not change"
        assert bool(torch.isfinite(p.flat_params).all())
    # replay the first rollout's actions through the mirror
    mirror = MT.SimpleTagNp(state0["agent_pos"], state0["agent_vel"], state0["landmark_pos"], episode_length=T)
    o = mirror.obs()
    for m in range(4):
        np.testing.assert_array_equal(_np(first[m]["obs"][0]), o[m].astype(np.float32))
    for t in range(T):
        acts = np.stack([_np(first[m]["actions"][t, :, 0]).astype(np.int64) for m in range(4)], axis=1)
        o, rew, dones = mirror.step(acts)
        assert bool(dones.all()) == (t == T - 1)
        if t == T - 1:                                             # the episode ended: slot T holds the reset state's observations
            o = MT.observation(end["agent_pos"], end["agent_vel"], end["landmark_pos"])
        share = np.concatenate(o, axis=1).astype(np.float32)
        for m in range(4):
            np.testing.assert_allclose(_np(first[m]["obs"][t + 1]), o[m].astype(np.float32), err_msg=f"obs, step {t}, agent {m}", **TOL)
            np.testing.assert_allclose(_np(first[m]["share_obs"][t + 1]), share, err_msg=f"share_obs, step {t}, agent {m}", **TOL)
            np.testing.assert_allclose(_np(first[m]["rewards"][t, :, 0]), rew[:, m].astype(np.float32), err_msg=f"rewards, step {t}, agent {m}",
                                       **TOL)
            np.testing.assert_array_equal(_np(first[m]["masks"][t + 1, :, 0]), 1.0 - dones[:, m].astype(np.float32))
    assert tuple(first[3]["obs"].shape) == (T + 1, N, 14) and tuple(first[0]["share_obs"].shape) == (T + 1, N, 62)
    assert len(torch.unique(torch.cat([first[m]["actions"] for m in range(4)]))) > 1
