"""MPE `simple_reference` on the GPU (csrc/mpe_ref_core.h, mpe_ref_env.hip, rollout_reference.h; mappo_amd/envs/mpe_reference.py):
  1. the step kernel against episodes stepped by the reference's own environment (tests/golden/mpe_envs.npz), both action modes:
     obs and rewards EQUAL the fp32 cast of the reference's float64 values (adds and multiplies only, contraction off);
  2. mappo_mpe_spread_step against the reference's simple_spread episodes (1e-6, the tolerance of tests/test_mpe_env.py);
  3. the reset draws;
  4. the one-launch episode (mappo_rollout_episode_reference) bit-identical to the stepwise path, buffer and env state;
  5. the recorded actions are what moved the agents and what the other agent heard;
  6. two training iterations."""
import numpy as np
import pytest
import torch

import mpe_ref_np
from conftest import golden, sub

BUF_NAMES = ("obs", "share_obs", "rewards", "masks", "actions", "action_log_probs", "value_preds", "returns")
ENV_NAMES = ("agent_pos", "agent_vel", "landmark_pos", "goal", "tstep", "episode")
COLORS = np.array([[0.75, 0.25, 0.25], [0.25, 0.75, 0.25], [0.25, 0.25, 0.75]], np.float32)


@pytest.fixture(scope="module")
def fx():
    g = golden("mpe_envs")
    return sub(g, "ref"), sub(g, "spread")


# ---- 1. the kernel against the reference, step by step ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_step_kernel_equals_the_reference_in_both_action_modes(gpu_device, fx):
    from mappo_amd.envs.mpe_reference import SimpleReferenceVecEnv
    ref, _ = fx
    N, T = ref["obs"].shape[:2]
    envs = [SimpleReferenceVecEnv(N, episode_length=T, seed=3, device=gpu_device) for _ in range(2)]
    for env in envs:
        env.set_state(ref["pos0"], ref["vel0"], ref["lpos"], ref["goals"])
    for t in range(T):
        idx = ref["actions"][:, t]
        acts = [torch.from_numpy(mpe_ref_np.onehot_actions(idx).astype(np.float32)).to(gpu_device),       # mode 0: [N, 2, 15]
                torch.from_numpy(idx.astype(np.float32)).to(gpu_device)]                                  # mode 1: [N, 2, 2]
        outs = []
        for env, a in zip(envs, acts):
            obs, rew, dones, _ = env.step(a)
            outs.append((obs.cpu().numpy(), rew.cpu().numpy(), dones.cpu().numpy()))
        for k in range(3):
            np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=f"mode 0 vs mode 1, step {t}, output {k}")
        for n in ENV_NAMES:
            assert torch.equal(getattr(envs[0], n), getattr(envs[1], n)), f"mode 0 vs mode 1, step {t}, state {n}"
        obs, rew, dones = outs[1]
        np.testing.assert_array_equal(dones, ref["dones"][:, t], err_msg=f"dones, step {t}")
        np.testing.assert_array_equal(rew[..., 0], ref["rewards"][:, t].astype(np.float32), err_msg=f"rewards, step {t}")
        env = envs[1]
        if not dones.all():
            np.testing.assert_array_equal(obs, ref["obs"][:, t].astype(np.float32), err_msg=f"obs, step {t}")
            assert int(env.tstep.min()) == t + 1 == int(env.tstep.max()) and int(env.episode.max()) == 0
        else:                                                   # the done step: the state was reset, the obs are the reset obs
            assert t == T - 1
            # before the reset the state was the reference's: the rewards above say so; now
            assert int(env.tstep.abs().max()) == 0 and int(env.episode.min()) == 1 == int(env.episode.max())
            assert float(env.agent_vel.abs().max()) == 0.0 and float(np.abs(obs[..., :2]).max()) == 0.0
            ap, lp = env.agent_pos.cpu().numpy(), env.landmark_pos.cpu().numpy()
            assert np.abs(ap).max() < 1.0 and np.abs(lp).max() < 0.8
            assert len(np.unique(ap)) == ap.size and len(np.unique(lp)) == lp.size
            assert (obs[..., 11:] == 0.0).all()
            goal = env.goal.cpu().numpy()
            assert goal.min() >= 0 and goal.max() <= 2
            np.testing.assert_array_equal(obs[..., 8:11], COLORS[goal])
            np.testing.assert_array_equal(obs[..., 2:8], (lp[:, None, :, :] - ap[:, :, None, :]).reshape(N, 2, 6).astype(np.float32))


# ---- 2. the spread kernel against the reference's spread episodes -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["onehot", "index"])
def test_spread_kernel_matches_the_reference(gpu_device, fx, mode):
    from mappo_amd.envs.mpe_spread import SimpleSpreadVecEnv
    _, sp = fx
    N, T = sp["obs"].shape[:2]
    env = SimpleSpreadVecEnv(N, 3, 3, T, seed=5, device=gpu_device)
    env.reset()
    env.set_state(sp["pos0"], sp["vel0"], sp["lpos"])
    for t in range(T):
        idx = sp["actions"][:, t]
        a = torch.from_numpy(np.eye(5, dtype=np.float32)[idx]) if mode == "onehot" else torch.from_numpy(idx.astype(np.float32)).view(N, 3, 1)
        obs, rew, dones, _ = env.step(a.to(gpu_device))
        np.testing.assert_array_equal(dones.cpu().numpy(), sp["dones"][:, t])
        np.testing.assert_allclose(rew.cpu().numpy()[..., 0], sp["rewards"][:, t], rtol=1e-6, atol=1e-6, err_msg=f"rewards, step {t}")
        if t < T - 1:                                           # (the done step returns the reset observations)
            np.testing.assert_allclose(obs.cpu().numpy(), sp["obs"][:, t], rtol=1e-6, atol=1e-6, err_msg=f"obs, step {t}")
    assert bool(dones.all())


# ---- 3. resets ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reset_draws(gpu_device):
    from mappo_amd.envs.mpe_reference import SimpleReferenceVecEnv
    N = 4096
    e1, e2, e3 = (SimpleReferenceVecEnv(N, seed=s, device=gpu_device) for s in (3, 3, 4))
    o1, o2, o3 = e1.reset().clone(), e2.reset().clone(), e3.reset().clone()
    assert torch.equal(o1, o2) and not torch.equal(o1, o3)     # same (seed, episode, env): same draw
    for n in ENV_NAMES:
        assert torch.equal(getattr(e1, n), getattr(e2, n)), n
    p, l, g = e1.agent_pos.cpu().numpy(), e1.landmark_pos.cpu().numpy(), e1.goal.cpu().numpy()
    assert np.abs(p).max() < 1.0 and np.abs(l).max() < 0.8 and float(e1.agent_vel.abs().max()) == 0.0
    assert abs(p.mean()) < 0.03 and abs(p.var() - 1 / 3) < 0.02 and abs(l.var() - 0.64 / 3) < 0.02
    vals = np.concatenate([p.ravel(), l.ravel() / 0.8])
    assert len(np.unique(vals)) == vals.size                   # no two draws share an index: different envs, entities, coordinates
    sigma = np.sqrt(2 * N / 9)
    for i in range(2):
        counts = np.bincount(g[:, i], minlength=3)
        assert counts.sum() == N and len(counts) == 3
        assert (np.abs(counts - N / 3) < 5 * sigma).all(), counts
    assert 0.2 < (g[:, 0] == g[:, 1]).mean() < 0.47            # independent goals agree a third of the time, not always
    assert float(o1[..., :2].abs().max()) == 0.0 and float(o1[..., 11:].abs().max()) == 0.0
    np.testing.assert_array_equal(o1[..., 8:11].cpu().numpy(), COLORS[g])
    o4 = e1.reset()
    assert int(e1.episode.min()) == 2 and not torch.equal(o4, o1)      # next episode, new draw
    assert not np.array_equal(e1.goal.cpu().numpy(), g)


# ---- 4. the one-launch episode equals the stepwise path ---------------------------------------------------------------------------------
def _runner(episode, centralized=True, layer_N=1, relu=True, N=11, T=6, env_T=4, graph=False, ppo_epoch=None):
    from mappo_amd.config import get_config
    from mappo_amd.envs.mpe_reference import SimpleReferenceVecEnv
    from mappo_amd.runner.shared.mpe_runner import MPERunner
    dev = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.use_centralized_V, a.layer_N, a.use_ReLU = centralized, layer_N, relu
    a.use_hip_graph, a.fuse_rollout_episode = graph, episode
    if ppo_epoch:
        a.ppo_epoch = ppo_epoch
    torch.manual_seed(1)
    env = SimpleReferenceVecEnv(N, episode_length=env_T, seed=1, device=dev)
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=2, device=dev, run_dir=None))
    g = torch.Generator(device=dev).manual_seed(7)             # affines away from (1, 0), larger weights: the same on both sides
    fp = r.policy.flat_params
    fp.add_(torch.randn(fp.shape, device=dev, generator=g) * 0.1)
    r.warmup()
    return r, env


def _state(r, env, names=BUF_NAMES):
    b = r.buffer
    out = {n: getattr(b, n).clone() for n in names}
    out["next_values"] = r._next_values.clone()
    out["counter"] = r.policy.actor._counter_dev.clone()
    for n in ENV_NAMES:
        out["env." + n] = getattr(env, n).clone()
    return out


def _assert_same(s0, s1, what=""):
    for k in s0:
        assert torch.equal(s0[k], s1[k]), f"{what}{k}: max |diff| {(s0[k].double() - s1[k].double()).abs().max().item()}"


def _counting(names):
    from mappo_amd import ops
    calls = {n: 0 for n in names}
    orig = {n: getattr(ops, n) for n in names}

    def wrap(n):
        def f(*a, **k):
            calls[n] += 1
            return orig[n](*a, **k)
        return f
    for n in names:
        setattr(ops, n, wrap(n))

    def restore():
        for n in names:
            setattr(ops, n, orig[n])
    return calls, restore


OPS = ("rollout_episode_reference", "rollout_episode_spread", "rollout_episode", "rollout_step_md", "rollout_step", "mpe_reference_step")


@pytest.mark.gpu
@pytest.mark.parametrize("centralized", [True, False], ids=["cent", "decent"])
@pytest.mark.parametrize("layer_N", [0, 1])
@pytest.mark.parametrize("relu", [False, True], ids=["tanh", "relu"])
def test_episode_launch_equals_stepwise(gpu_device, relu, layer_N, centralized):
    """Two eager rollouts through each path, N = 11 (two tiles of 8 environments, the second partial), T = 6 against an env episode
    of 4 (a reset inside every rollout, a non-zero tstep at the start of the second): every buffer array, the bootstrap values, the
    counter word and the env's six state tensors agree bit for bit — and the runner took the branch it was asked for."""
    runs, counts = [], []
    for episode in (False, True):
        calls, restore = _counting(OPS)
        try:
            r, env = _runner(episode, centralized, layer_N, relu)
            assert not r.policy.can_fuse_episode() and r.policy.can_fuse_episode_reference()
            states = []
            for _ in range(2):
                r.rollout()
                states.append(_state(r, env))
            torch.cuda.synchronize()
        finally:
            restore()
        runs.append(states)
        counts.append(dict(calls))
    assert counts[0] == dict(rollout_episode_reference=0, rollout_episode_spread=0, rollout_episode=0, rollout_step_md=12, rollout_step=2,
                             mpe_reference_step=12), counts[0]
    assert counts[1] == dict(rollout_episode_reference=2, rollout_episode_spread=0, rollout_episode=0, rollout_step_md=0, rollout_step=0,
                             mpe_reference_step=0), counts[1]
    for e in range(2):
        _assert_same(runs[0][e], runs[1][e], what=f"rollout {e}: ")
    s = runs[1][0]
    assert not torch.equal(s["actions"], runs[1][1]["actions"]) and not torch.equal(s["obs"], runs[1][1]["obs"])
    assert float(s["masks"][4].max()) == 0.0 and float(s["masks"][1:4].min()) == 1.0 and float(s["masks"][5:].min()) == 1.0
    assert int(s["env.tstep"].min()) == 2 == int(s["env.tstep"].max()) and int(s["env.episode"].min()) == 2
    assert int(runs[1][1]["env.tstep"].max()) == 0 and int(runs[1][1]["env.episode"].min()) == 4        # 12 = 3 x 4
    a = s["actions"]
    assert float(a[..., 0].max()) <= 4 and float(a[..., 1].max()) <= 9 and float(a.min()) >= 0 and len(torch.unique(a[..., 1])) > 5


@pytest.mark.gpu
def test_episode_launch_equals_stepwise_deterministic(gpu_device):
    """The argmax path of both heads, through the policy's own entry points (the runner always samples)."""
    T = 6
    outs = []
    for episode in (False, True):
        r, env = _runner(episode)
        b, pol = r.buffer, r.policy
        r._next_values = torch.empty(b.n_rollout_threads * b.num_agents, device=b.device)
        for _ in range(2):
            pol.actor._counter_dev.add_(T)
            if episode:
                pol.collect_episode_reference_fused(b, env.episode_state_reference(), r._next_values, True, deterministic=True)
            else:
                pending = None
                for step in range(T):
                    actions = pol.collect_step_fused(b, step, pending, True, deterministic=True)
                    obs, rew, dones, _ = env.step(actions)
                    pending = (obs, rew, dones)
                pol.collect_step_fused(b, T, pending, True, values_only=r._next_values)
            b.obs[0].copy_(b.obs[T]); b.share_obs[0].copy_(b.share_obs[T]); b.masks[0].copy_(b.masks[T])      # after_update
        torch.cuda.synchronize()
        outs.append(_state(r, env, names=BUF_NAMES[:-1]))
    _assert_same(outs[0], outs[1])
    assert len(torch.unique(outs[1]["actions"])) > 2


@pytest.mark.gpu
def test_episode_launch_equals_stepwise_under_the_hip_graph(gpu_device):
    """Eager rollout, capture, replay: the replayed third rollout of both runners leaves identical buffers and env states, sees new
    observations and draws from a fresh sampling stream."""
    runs = []
    for episode in (False, True):
        r, env = _runner(episode, graph=True)
        states = []
        for _ in range(3):
            r.rollout()
            torch.cuda.synchronize()
            states.append(_state(r, env))
        assert isinstance(r._rollout_graph, torch.cuda.CUDAGraph)
        runs.append(states)
    for e in range(3):
        _assert_same(runs[0][e], runs[1][e], what=f"call {e}: ")
    assert not torch.equal(runs[1][2]["obs"], runs[1][1]["obs"]) and not torch.equal(runs[1][2]["actions"], runs[1][1]["actions"])
    assert runs[1][2]["counter"].item() == runs[1][1]["counter"].item() + 6


# ---- 5. the actions are consumed ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_recorded_actions_move_the_agents_and_reach_the_other_agent(gpu_device):
    r, env = _runner(True, N=32, T=12, env_T=5)
    r.rollout()
    torch.cuda.synchronize()
    b = r.buffer
    obs, acts, masks = b.obs.cpu().numpy(), b.actions.cpu().numpy().astype(np.int64), b.masks.cpu().numpy()[..., 0]
    T = 12
    U = np.array([[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]], np.float32)               # move index -> direction
    n_live = n_reset = 0
    for t in range(T):
        live = masks[t + 1] == 1.0                                                    # [N, 2]
        heard = np.eye(10, dtype=np.float32)[acts[t][:, ::-1, 1]]                     # agent i hears the OTHER agent's head 1
        comm = obs[t + 1][..., 11:]
        np.testing.assert_array_equal(comm[live], heard[live], err_msg=f"comm, step {t}")
        assert (comm[~live] == 0.0).all(), f"comm after a reset, step {t}"
        vel = 0.75 * obs[t][..., :2] + 0.5 * U[acts[t][..., 0]]
        np.testing.assert_allclose(obs[t + 1][..., :2][live], vel[live], rtol=0, atol=2e-6, err_msg=f"velocity, step {t}")
        assert (obs[t + 1][..., :2][~live] == 0.0).all()
        n_live += int(live.sum()); n_reset += int((~live).sum())
    assert n_reset == 2 * 32 * 2 and n_live == 12 * 64 - n_reset                       # resets at steps 5 and 10
    rew = b.rewards.cpu().numpy()
    assert (rew < 0).all() and (rew[:, :, 0] == rew[:, :, 1]).all()


# ---- 6. training ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_training_iterations(gpu_device):
    r, env = _runner(True, N=16, T=10, env_T=10, ppo_epoch=2)
    p0 = r.policy.flat_params.clone()
    calls, restore = _counting(("rollout_episode_reference",))
    try:
        for it in range(2):
            info, _ = r.run_episode(it, 2)
            torch.cuda.synchronize()
            assert all(np.isfinite(v) for v in info.values()), info
    finally:
        restore()
    assert calls["rollout_episode_reference"] == 2
    assert not torch.equal(p0, r.policy.flat_params) and bool(torch.isfinite(r.policy.flat_params).all())
    average_episode_rewards = float(r.buffer.rewards.mean().item()) * r.episode_length
    assert np.isfinite(average_episode_rewards) and average_episode_rewards < 0
