"""GPU-vectorised MPE simple_adversary: the env kernel (csrc/mpe_ragged_env.hip) against the fixture stepped by the reference's own
environment (tests/golden/mpe_adversary.npz) — outputs EQUAL the fp32 cast —, its reset against the host Philox, the one-launch
episode (mappo_rollout_episode_adversary) bit for bit against the stepwise path, sampling against float64 and the host Philox, and
the separated runner on three agents of two observation widths and per-agent rewards."""
import itertools

import numpy as np
import pytest
import torch

from conftest import golden
import adversary_rollout_ref as AR
import mpe_adversary_np as MA
import rollout_ref as R

pytestmark = pytest.mark.gpu

OBS = ("adversary", "good1", "good2")
NAMES = ("share_obs", "obs", "rnn_states", "rnn_states_critic", "value_preds", "returns", "actions", "action_log_probs", "rewards",
         "masks", "bad_masks", "active_masks")


def _fx(tag):
    g = golden("mpe_adversary")
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}


def _env(N, T=25, seed=3):
    from mappo_amd.envs import SimpleAdversaryVecEnv
    return SimpleAdversaryVecEnv(N, episode_length=T, seed=seed)


def _np(t):
    return t.detach().cpu().numpy()


def _act(a, mode):
    """Recorded indices [N, 3] in one of the forms step() takes."""
    if mode == "onehot":
        return torch.eye(5)[torch.from_numpy(a.astype(np.int64))].cuda()
    if mode == "onehot_list":
        return [torch.eye(5)[torch.from_numpy(a[:, m].astype(np.int64))].cuda() for m in range(3)]
    if mode == "index_list":
        return [torch.from_numpy(a[:, m].astype(np.float32)).cuda() for m in range(3)]
    return torch.from_numpy(a.astype(np.float32)).cuda()


MODES = ["onehot", "onehot_list", "index_list", "index_tensor"]


# ---- the env kernel against the fixture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_fixture_parity_long_episodes(gpu_device, mode):
    g = _fx("long")
    E, T = 12, 25
    env = _env(E, T=T + 1)                                        # the reference env does not reset itself: keep the stepped state
    env.set_state(g["pos0"], g["vel0"], g["lpos"], g["goal"])
    for t in range(T):
        obs, rew, dones, _ = env.step(_act(g["actions"][:, t], mode))
        for m in range(3):
            np.testing.assert_array_equal(_np(obs[m]), g["obs_" + OBS[m]][:, t].astype(np.float32), err_msg=f"obs of agent {m}, step {t}")
        np.testing.assert_array_equal(_np(rew)[..., 0], g["rewards"][:, t].astype(np.float32), err_msg=f"rewards, step {t}")
        assert tuple(rew.shape) == (E, 3, 1) and dones.dtype == torch.bool and not bool(dones.any())
    np.testing.assert_array_equal(_np(env.agent_pos), g["pos1"])
    np.testing.assert_array_equal(_np(env.agent_vel), g["vel1"])
    np.testing.assert_array_equal(_np(env.landmark_pos), g["lpos"])
    assert int(env.tstep.min()) == T and int(env.tstep.max()) == T


@pytest.mark.parametrize("mode", ["onehot", "index_tensor"])
def test_fixture_parity_across_reset_on_done(gpu_device, mode):
    """episode_length 7, 14 steps.  Rewards and dones equal the fixture's at every step, the ending ones included; a step that ends
    an episode returns the observation of the env's OWN reset state (its Philox draws, not NumPy's), at rest, step 0; the fixture's
    reset state is then loaded and the second episode must follow the fixture again."""
    g = _fx("short")
    E = 2
    env = _env(E, T=7, seed=5)
    env.set_state(g["pos0"], g["vel0"], g["lpos"], g["goal"])
    resets = 0
    for t in range(14):
        obs, rew, dones, _ = env.step(_act(g["actions"][:, t], mode))
        np.testing.assert_array_equal(_np(dones), g["dones"][:, t])
        np.testing.assert_array_equal(_np(rew)[..., 0], g["rewards"][:, t].astype(np.float32), err_msg=f"rewards, step {t}")
        if g["dones"][:, t].all():
            resets += 1
            assert int(env.tstep.abs().max()) == 0 and _np(env.episode).tolist() == [resets] * E and float(env.agent_vel.abs().max()) == 0.0
            want = MA.observation(_np(env.agent_pos), _np(env.landmark_pos), _np(env.goal).astype(np.int64))
            for m in range(3):
                np.testing.assert_array_equal(_np(obs[m]), want[m].astype(np.float32), err_msg=f"reset obs of agent {m}")
            k = resets - 1
            env.set_state(g["reset_pos"][:, k], np.zeros((E, 3, 2)), g["reset_lpos"][:, k], g["reset_goal"][:, k])
        else:
            for m in range(3):
                np.testing.assert_array_equal(_np(obs[m]), g["obs_" + OBS[m]][:, t].astype(np.float32), err_msg=f"obs of agent {m}, step {t}")
    assert resets == 2


def test_index_actions_are_clamped(gpu_device):
    a, b = _env(4), _env(4)
    a.reset(); b.reset()
    (oa, _, _), ra, _, _ = a.step(torch.tensor([[-3.0, 9.0, 4.0]] * 4).cuda())
    (ob, _, _), rb, _, _ = b.step(torch.tensor([[0.0, 4.0, 4.0]] * 4).cuda())
    assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(a.agent_pos, b.agent_pos)


# ---- reset ----------------------------------------------------------------------------------------------------------------------------------
def test_reset_draws_equal_the_host_philox(gpu_device):
    N, seed = 37, 11
    env = _env(N, seed=seed)
    obs = env.reset()
    pos, lpos, goal = MA.reset_draws(seed, 1, N)
    np.testing.assert_array_equal(_np(env.agent_pos), pos)
    np.testing.assert_array_equal(_np(env.landmark_pos), lpos)
    np.testing.assert_array_equal(_np(env.goal), goal)
    assert sorted(np.unique(_np(env.goal))) == [0, 1]
    for t in (env.agent_pos, env.landmark_pos):
        assert float(t.min()) >= -1.0 and float(t.max()) < 1.0
    assert float(env.agent_vel.abs().max()) == 0.0 and _np(env.episode).tolist() == [1] * N and int(env.tstep.abs().max()) == 0
    want = MA.observation(pos, lpos, goal)
    for m in range(3):
        assert tuple(obs[m].shape) == (N, MA.OBS_DIMS[m])
        np.testing.assert_array_equal(_np(obs[m]), want[m].astype(np.float32))
    env.reset()                                                    # the second reset draws stream (seed, 2)
    np.testing.assert_array_equal(_np(env.agent_pos), MA.reset_draws(seed, 2, N)[0])
    # reset-on-done inside step() draws the same way
    e2 = _env(N, T=1, seed=seed)
    e2.step(torch.zeros(N, 3).cuda())
    np.testing.assert_array_equal(_np(e2.agent_pos), pos)
    np.testing.assert_array_equal(_np(e2.goal), goal)


@pytest.mark.parametrize("N", [1, 37])
def test_partial_block_writes_nothing_beyond_N(gpu_device, N):
    """Every output and state array sits in front of a NaN (or sentinel) guard region; reset and both step modes leave it alone."""
    from mappo_amd import ops
    G = 64
    f64 = lambda *s: torch.full((N + G, *s), float("nan"), dtype=torch.float64, device="cuda")
    f32 = lambda *s: torch.full((N + G, *s), float("nan"), dtype=torch.float32, device="cuda")
    i32 = lambda: torch.full((N + G,), -77, dtype=torch.int32, device="cuda")
    pos, vel, lpos, goal, tstep = f64(3, 2), f64(3, 2), f64(2, 2), i32(), i32()
    ep = torch.full((N + G,), -77, dtype=torch.int64, device="cuda")
    ep[:N] = 0
    o0, o1, o2, rew = f32(8), f32(10), f32(10), f32(3)
    dones = torch.full((N + G, 3), 9, dtype=torch.uint8, device="cuda")
    ops.mpe_adversary_reset(pos, vel, lpos, goal, tstep, ep, o0, o1, o2, N, 11)
    idx = torch.stack([(torch.arange(N) + m) % 5 for m in range(3)], dim=1).float().cuda().contiguous()
    ops.mpe_adversary_step(pos, vel, lpos, goal, tstep, ep, idx, 1, o0, o1, o2, rew, dones, N, 2, 11)
    ops.mpe_adversary_step(pos, vel, lpos, goal, tstep, ep, torch.eye(5, device="cuda")[idx.long()].contiguous(), 0, o0, o1, o2, rew, dones, N,
                           2, 11)
    torch.cuda.synchronize()
    for name, t in (("pos", pos), ("vel", vel), ("lpos", lpos), ("o0", o0), ("o1", o1), ("o2", o2), ("rew", rew)):
        assert bool(torch.isnan(t[N:]).all()), name
        assert bool(torch.isfinite(t[:N]).all()), name
    for name, t in (("goal", goal), ("tstep", tstep), ("episode", ep)):
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


def _runner(env, T, N, **kw):
    from mappo_amd.runner.separated.mpe_runner import MPERunner
    a = _args(episode_length=T, n_rollout_threads=N, env_name="MPE", share_policy=False, use_hip_graph=False, seed=AR.SEED,
              algorithm_name="mappo", ppo_epoch=2, num_mini_batch=1, **kw)
    torch.manual_seed(1)
    return MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=3, device=torch.device("cuda"), run_dir=None))


def _snapshot(r):
    out = {}
    for m, b in enumerate(r.buffer):
        for n in NAMES:
            if getattr(b, n) is not None:
                out[f"agent{m}/{n}"] = getattr(b, n).clone()
        out[f"agent{m}/next_values"] = r._next_values[m].clone()
    out.update({f"env/{k}": v.clone() for k, v in r.envs.state_tensors().items()})
    return out


def _assert_equal(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs ({(a[k] != b[k]).sum().item()} of {a[k].numel()} elements)"


def _count_calls(monkeypatch):
    from mappo_amd import ops
    calls = []
    real = ops.rollout_episode_adversary
    monkeypatch.setattr(ops, "rollout_episode_adversary", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


# ---- one launch == stepwise --------------------------------------------------------------------------------------------------------------------
#        N: one ragged tile | two full tiles and a ragged one; (T, env T): resets inside the rollout | the short case
CASES = list(itertools.product((5, 37), ((25, 7), (4, 25)), (0, 1), (True, False), (True, False)))


@pytest.mark.parametrize("N,TT,layer_N,relu,cen", CASES, ids=[f"N{c[0]}-T{c[1][0]}-envT{c[1][1]}-L{c[2]}-{'relu' if c[3] else 'tanh'}-"
                                                              f"{'cen' if c[4] else 'dec'}" for c in CASES])
def test_one_launch_equals_stepwise(gpu_device, monkeypatch, N, TT, layer_N, relu, cen):
    T, env_T = TT
    calls = _count_calls(monkeypatch)
    runs = {}
    for flag in ("1", "1 again", "0"):
        monkeypatch.setenv("MAPPO_ADV_EPISODE", flag[0])
        r = _runner(_env(N, env_T), T, N, layer_N=layer_N, use_ReLU=relu, use_centralized_V=cen)
        assert r._ragged and r._fused_ff() and r._adversary_episode_ready() == (flag[0] == "1")
        r.warmup()
        snaps = []
        for it in range(2):                                        # the second episode continues from the first one's state
            n0 = len(calls)
            r.rollout()
            assert len(calls) - n0 == (1 if flag[0] == "1" else 0)
            snaps.append(_snapshot(r))
            for b in r.buffer:
                b.after_update()
        runs[flag] = snaps
    for it in range(2):
        _assert_equal(runs["1"][it], runs["0"][it], f"episode {it}, one launch vs stepwise")
        _assert_equal(runs["1"][it], runs["1 again"][it], f"episode {it}, repeated launch")
    s = runs["1"][1]
    assert all(bool(torch.isfinite(v).all()) for k, v in s.items() if v.is_floating_point())
    assert tuple(s["agent0/obs"].shape) == (T + 1, N, 8) and tuple(s["agent2/obs"].shape) == (T + 1, N, 10)
    assert tuple(s["agent1/share_obs"].shape) == (T + 1, N, 28 if cen else 10)
    if env_T < T:                                                  # resets fell inside the rollout
        assert int(s["env/episode"].min()) >= 2 * (T // env_T) and float(s["agent0/masks"][1:].min()) == 0.0
    assert not torch.equal(s["agent0/rewards"], s["agent1/rewards"]) and torch.equal(s["agent1/rewards"], s["agent2/rewards"])
    for m in range(3):
        assert len(torch.unique(s[f"agent{m}/actions"])) > 1


@pytest.mark.parametrize("layer_N,cen", [(1, True), (0, False)])
def test_one_launch_writes_nothing_outside_the_buffers(gpu_device, layer_N, cen):
    from mappo_amd import ops
    N, T, G = 37, 3, 64
    env = _env(N, 2)
    r = _runner(env, T, N, layer_N=layer_N, use_centralized_V=cen)
    obs = env.reset()
    fulls = []

    def guarded(*shape):
        n = int(np.prod(shape))
        full = torch.full((n + 2 * G,), float("nan"), device="cuda")
        fulls.append((full, n))
        return full[G:G + n].view(*shape)
    ags, views = [], []
    for m, p in enumerate(r.policy):
        D = MA.OBS_DIMS[m]
        v = dict(obs=guarded(T + 1, N, D), share=guarded(T + 1, N, 28 if cen else D), rew=guarded(T, N, 1), mask=guarded(T + 1, N, 1),
                 act=guarded(T, N, 1), logp=guarded(T, N, 1), val=guarded(T + 1, N, 1), nv=guarded(N))
        v["obs"][0].copy_(obs[m]); v["share"][0].copy_(torch.cat(obs, dim=1) if cen else obs[m]); v["mask"][0].fill_(1.0)
        views.append(v)
        ags.append(ops.comm_agent(p.actor.flat, p.actor.desc, p.critic.flat, p.critic.desc, p.actor._seed, None, v["obs"], v["share"], v["rew"],
                                  v["mask"], v["act"], v["logp"], v["val"], v["nv"]))
    st = env.episode_state_adversary()
    ops.rollout_episode_adversary(ags, T, N, st["T"], st["seed"], st["agent_pos"], st["agent_vel"], st["landmark_pos"], st["goal"],
                                  st["tstep"], st["episode"], False, 0, cen)
    torch.cuda.synchronize()
    for full, n in fulls:
        assert bool(torch.isnan(full[:G]).all()) and bool(torch.isnan(full[G + n:]).all())
    for v in views:
        for k in ("obs", "share", "rew", "mask", "act", "logp", "nv"):
            assert bool(torch.isfinite(v[k]).all()), k
        assert bool(torch.isfinite(v["val"][:T]).all()) and bool(torch.isnan(v["val"][T]).all())     # slot T belongs to nobody here


# ---- sampling against float64 + the host Philox ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["0", "1"], ids=["stepwise", "one-launch"])
def test_rollout_against_float64_and_host_philox(gpu_device, monkeypatch, flag):
    monkeypatch.setenv("MAPPO_ADV_EPISODE", flag)
    N, T = AR.N, AR.T
    env = _env(N, AR.ENV_T)
    r = _runner(env, T, N)
    tw = AR.twins()
    for m in range(3):
        r.policy[m].actor.load_state_dict(tw[m].actor.state_dict())
        r.policy[m].critic.load_state_dict(tw[m].critic.state_dict())
        assert r.policy[m].actor._seed == AR.agent_seed(m)
    r.warmup()
    env.set_state(*AR.initial_state())
    mirror = MA.SimpleAdversaryNp(*AR.initial_state(), episode_length=AR.ENV_T)
    o0 = mirror.obs()
    for m in range(3):                                             # warmup's slot 0, from the loaded state
        r.buffer[m].obs[0].copy_(torch.from_numpy(o0[m].astype(np.float32)))
        r.buffer[m].share_obs[0].copy_(torch.from_numpy(np.concatenate(o0, axis=1).astype(np.float32)))
    r.rollout()
    fails, near, pairs = [], 0, 0
    for t in range(T):
        acts = []
        for m in range(3):
            b = r.buffer[m]
            e, tol = AR.expected_step(tw[m].actor, _np(b.obs[t]), m, t)
            a, lp = _np(b.actions[t, :, 0]), _np(b.action_log_probs[t, :, 0])
            print(f"step {t} agent {m}: tol {tol:.2e}, max log-prob error {R.max_logp_err(e, a, lp):.2e}, near rows {int(e.near.sum())}")
            near += int(e.near.sum()); pairs += e.near.size
            fails += R.check_actions(e, None, a, lp, tol, f"step {t} agent {m}")
            v64, _ = R.critic_eval(tw[m].critic, _np(b.share_obs[t]), dtype=torch.float64)
            v32, _ = R.critic_eval(tw[m].critic, _np(b.share_obs[t]), dtype=torch.float32)
            _, tol_v = R.err_and_tol(v64, v32)
            dv = float(np.abs(_np(b.value_preds[t, :, 0]) - v64).max())
            print(f"step {t} agent {m}: value tol {tol_v:.2e}, max error {dv:.2e}")
            if dv > tol_v:
                fails.append(f"step {t} agent {m}: value off by {dv:.3e} > {tol_v:.3e}")
            acts.append(a.astype(np.int64))
        obs, rew, dones = mirror.step(np.stack(acts, axis=1))
        share = np.concatenate(obs, axis=1).astype(np.float32)
        for m in range(3):
            b = r.buffer[m]
            np.testing.assert_array_equal(_np(b.obs[t + 1]), obs[m].astype(np.float32), err_msg=f"obs, step {t}, agent {m}")
            np.testing.assert_array_equal(_np(b.share_obs[t + 1]), share, err_msg=f"share_obs, step {t}, agent {m}")
            np.testing.assert_array_equal(_np(b.rewards[t, :, 0]), rew[:, m].astype(np.float32), err_msg=f"rewards, step {t}, agent {m}")
            np.testing.assert_array_equal(_np(b.masks[t + 1, :, 0]), 1.0 - dones[:, m].astype(np.float32))
    assert near <= AR.NEAR_CAP * pairs, f"{near} of {pairs} (row, agent) pairs left out"
    assert not fails, "\n".join(fails)
    np.testing.assert_array_equal(_np(env.agent_pos), mirror.pos)
    np.testing.assert_array_equal(_np(env.agent_vel), mirror.vel)


# ---- training ---------------------------------------------------------------------------------------------------------------------------------
def test_runner_trains_three_agents_either_way(gpu_device, monkeypatch):
    """N = 8, T = 25, two iterations, stepwise and the default path: the buffers of the first rollout are identical, replaying their
    actions through the NumPy mirror from the initial state reproduces the stored observations and per-agent rewards, all three
    policies change and stay finite, and train_infos has one entry per agent."""
    N, T = 8, 25
    first = {}
    for flag in ("0", None):
        if flag is None:
            monkeypatch.delenv("MAPPO_ADV_EPISODE", raising=False)
        else:
            monkeypatch.setenv("MAPPO_ADV_EPISODE", flag)
        env = _env(N, T)
        r = _runner(env, T, N)
        r.warmup()
        state0 = {k: _np(v).copy() for k, v in env.state_tensors().items()}
        before = [p.flat_params.clone() for p in r.policy]
        assert r.policy[0].actor.desc.in_dim == 8 and r.policy[1].actor.desc.in_dim == 10 and r.policy[2].actor.desc.in_dim == 10
        for it in range(2):
            r.rollout()
            if it == 0:
                first[flag] = _snapshot(r)
            infos = r.train()
            assert len(infos) == 3
            for m, info in enumerate(infos):
                for k, v in info.items():
                    assert np.isfinite(float(v)), (flag, it, m, k, v)
        for m, p in enumerate(r.policy):
            a0, a1 = before[m][:p.actor.n_params], p.flat_params[:p.actor.n_params]
            lo = p.seg_bounds[1]
            c0, c1 = before[m][lo:lo + p.critic.n_params], p.flat_params[lo:lo + p.critic.n_params]
            assert not torch.equal(a0, a1) and not torch.equal(c0, c1), f"agent {m}: parameters did not change"
            assert bool(torch.isfinite(p.flat_params).all())
        # replay the first rollout's actions through the mirror
        s = first[flag]
        mirror = MA.SimpleAdversaryNp(state0["agent_pos"], state0["agent_vel"], state0["landmark_pos"], state0["goal"], episode_length=T)
        o = mirror.obs()
        for m in range(3):
            np.testing.assert_array_equal(_np(s[f"agent{m}/obs"][0]), o[m].astype(np.float32))
        for t in range(T):
            acts = np.stack([_np(s[f"agent{m}/actions"][t, :, 0]).astype(np.int64) for m in range(3)], axis=1)
            o, rew, dones = mirror.step(acts)
            assert bool(dones.all()) == (t == T - 1)
            if t == T - 1:                                         # the episode ended: slot T holds the reset state's observations
                o = MA.observation(_np(s["env/agent_pos"]), _np(s["env/landmark_pos"]), _np(s["env/goal"]).astype(np.int64))
            share = np.concatenate(o, axis=1).astype(np.float32)
            for m in range(3):
                np.testing.assert_array_equal(_np(s[f"agent{m}/obs"][t + 1]), o[m].astype(np.float32), err_msg=f"obs, step {t}, agent {m}")
                np.testing.assert_array_equal(_np(s[f"agent{m}/share_obs"][t + 1]), share, err_msg=f"share_obs, step {t}, agent {m}")
                np.testing.assert_array_equal(_np(s[f"agent{m}/rewards"][t, :, 0]), rew[:, m].astype(np.float32),
                                              err_msg=f"rewards, step {t}, agent {m}")
                np.testing.assert_array_equal(_np(s[f"agent{m}/masks"][t + 1, :, 0]), 1.0 - dones[:, m].astype(np.float32))
        assert not torch.equal(s["agent0/rewards"], s["agent1/rewards"])
    _assert_equal(first["0"], first[None], "first rollout, stepwise vs the default path")
