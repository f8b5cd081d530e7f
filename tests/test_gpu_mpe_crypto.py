"""GPU-vectorised MPE simple_crypto: the env kernel (csrc/mpe_ragged_env.hip) against the fixture stepped by the reference's own
environment (tests/golden/mpe_crypto.npz) — outputs EQUAL the fp32 cast —, its reset against the host Philox, the one-launch episode
(mappo_rollout_episode_crypto) bit for bit against the stepwise path, sampling against float64 and the host Philox, and the
separated runner on three agents of two observation widths (4 / 8 / 8) and per-agent rewards."""
import numpy as np
import pytest
import torch

from conftest import golden
import crypto_rollout_ref as CR
import mpe_crypto_np as MC
import rollout_ref as R

pytestmark = pytest.mark.gpu

OBS = ("eve", "bob", "alice")
NAMES = ("share_obs", "obs", "rnn_states", "rnn_states_critic", "value_preds", "returns", "actions", "action_log_probs", "rewards",
         "masks", "bad_masks", "active_masks")


def _fx(tag, L):
    """The fixture's episodes with L landmarks."""
    g = golden("mpe_crypto")
    rows = g[tag + "/num_landmarks"] == L
    return {k[len(tag) + 1:]: g[k][rows] for k in g.files if k.startswith(tag + "/")}


def _env(N, T=25, seed=3, L=2):
    from mappo_amd.envs import SimpleCryptoVecEnv
    return SimpleCryptoVecEnv(N, num_landmarks=L, episode_length=T, seed=seed)


def _np(t):
    return t.detach().cpu().numpy()


def _act(a, mode):
    """Recorded indices [N, 3] in one of the forms step() takes."""
    if mode == "onehot":
        return torch.eye(4)[torch.from_numpy(a.astype(np.int64))].cuda()
    if mode == "onehot_list":
        return [torch.eye(4)[torch.from_numpy(a[:, m].astype(np.int64))].cuda() for m in range(3)]
    if mode == "index_list":
        return [torch.from_numpy(a[:, m].astype(np.float32)).cuda() for m in range(3)]
    return torch.from_numpy(a.astype(np.float32)).cuda()


def _state_obs(env):
    """What the NumPy mirror observes in the env's own state."""
    return MC.observation(_np(env.goal).astype(np.int64), _np(env.key).astype(np.int64), _np(env.comm).astype(np.int64))


MODES = ["onehot", "onehot_list", "index_list", "index_tensor"]


# ---- the env kernel against the fixture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("mode", MODES)
def test_fixture_parity_long_episodes(gpu_device, mode, L):
    """Episode length 25 as in the fixture: observations, rewards and dones EQUAL the fp32 cast at every step; the last step is done
    for all three agents and returns the observation of the env's OWN reset state (its Philox draws, not NumPy's)."""
    g = _fx("long", L)
    E, T = 12, 25
    env = _env(E, T=T, L=L)
    env.set_state(g["goal"], g["key"])
    for m, o in enumerate(_state_obs(env)):                       # nothing said yet: what the reference's reset returned
        np.testing.assert_array_equal(o, g["obs0_" + OBS[m]])
    for t in range(T):
        obs, rew, dones, _ = env.step(_act(g["actions"][:, t], mode))
        np.testing.assert_array_equal(_np(rew)[..., 0], g["rewards"][:, t].astype(np.float32), err_msg=f"rewards, step {t}")
        np.testing.assert_array_equal(_np(dones), g["dones"][:, t], err_msg=f"dones, step {t}")
        assert tuple(rew.shape) == (E, 3, 1) and dones.dtype == torch.bool
        if t < T - 1:
            for m in range(3):
                np.testing.assert_array_equal(_np(obs[m]), g["obs_" + OBS[m]][:, t].astype(np.float32), err_msg=f"obs of agent {m}, step {t}")
            np.testing.assert_array_equal(_np(env.comm), g["actions"][:, t])
            np.testing.assert_array_equal(_np(env.goal), g["goal"])
            np.testing.assert_array_equal(_np(env.key), g["key"])
    assert _np(env.tstep).tolist() == [0] * E and _np(env.episode).tolist() == [1] * E and _np(env.comm).tolist() == [[-1] * 3] * E
    for m, o in enumerate(_state_obs(env)):
        np.testing.assert_array_equal(_np(obs[m]), o.astype(np.float32), err_msg=f"reset obs of agent {m}")


@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("mode", ["onehot", "index_tensor"])
def test_fixture_parity_across_reset_on_done(gpu_device, mode, L):
    """episode_length 7, 14 steps.  Rewards and dones equal the fixture's at every step, the ending ones included; a step that ends
    an episode returns the observation of the env's OWN reset state, nothing said, step 0; the fixture's reset state is then loaded
    and the second episode must follow the fixture again."""
    g = _fx("short", L)
    E = 1
    env = _env(E, T=7, seed=5, L=L)
    env.set_state(g["goal"], g["key"])
    resets = 0
    for t in range(14):
        obs, rew, dones, _ = env.step(_act(g["actions"][:, t], mode))
        np.testing.assert_array_equal(_np(dones), g["dones"][:, t])
        np.testing.assert_array_equal(_np(rew)[..., 0], g["rewards"][:, t].astype(np.float32), err_msg=f"rewards, step {t}")
        if g["dones"][:, t].all():
            resets += 1
            assert int(env.tstep.abs().max()) == 0 and _np(env.episode).tolist() == [resets] * E and _np(env.comm).tolist() == [[-1] * 3] * E
            assert 0 <= int(env.goal.min()) and int(env.goal.max()) < L and 0 <= int(env.key.min()) and int(env.key.max()) < L
            for m, o in enumerate(_state_obs(env)):
                np.testing.assert_array_equal(_np(obs[m]), o.astype(np.float32), err_msg=f"reset obs of agent {m}")
            k = resets - 1
            env.set_state(g["reset_goal"][:, k], g["reset_key"][:, k])
            for m, o in enumerate(_state_obs(env)):               # the forced state is the one whose observation the fixture kept
                np.testing.assert_array_equal(o, g["obs_" + OBS[m]][:, t])
        else:
            for m in range(3):
                np.testing.assert_array_equal(_np(obs[m]), g["obs_" + OBS[m]][:, t].astype(np.float32), err_msg=f"obs of agent {m}, step {t}")
    assert resets == 2


def test_index_actions_are_clamped(gpu_device):
    a, b = _env(4), _env(4)
    a.reset(); b.reset()
    oa, ra, _, _ = a.step(torch.tensor([[-3.0, 9.0, 3.0], [7.0, -1.0, 4.0]] * 2).cuda())
    ob, rb, _, _ = b.step(torch.tensor([[0.0, 3.0, 3.0], [3.0, 0.0, 3.0]] * 2).cuda())
    assert all(torch.equal(x, y) for x, y in zip(oa, ob)) and torch.equal(ra, rb) and torch.equal(a.comm, b.comm)
    assert _np(a.comm).tolist() == [[0, 3, 3], [3, 0, 3]] * 2


def test_onehot_rows_take_their_first_maximum(gpu_device):
    """Mode 0 on rows that are not one-hots: ties go to the lower index, as np.argmax."""
    env = _env(2)
    env.reset()
    rows = torch.tensor([[[0.2, 0.5, 0.5, 0.1], [0.0, 0.0, 0.0, 0.0], [0.1, 0.2, 0.3, 0.4]],
                         [[1.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0], [-1.0, -2.0, -0.5, -0.5]]]).cuda()
    env.step(rows)
    assert _np(env.comm).tolist() == [[1, 0, 3], [0, 2, 2]]


# ---- reset ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3, 4])
def test_reset_draws_equal_the_host_philox(gpu_device, L):
    N, seed = 4096, 11
    env = _env(N, seed=seed, L=L)
    obs = env.reset()
    goal, key = MC.reset_draws(seed, 1, N, L)
    np.testing.assert_array_equal(_np(env.goal), goal)
    np.testing.assert_array_equal(_np(env.key), key)
    assert sorted(np.unique(_np(env.goal))) == list(range(L)) and sorted(np.unique(_np(env.key))) == list(range(L))
    same = int((env.goal == env.key).sum())
    assert 0 < same < N                                            # two independent draws: equal somewhere, different somewhere
    assert _np(env.comm).tolist() == [[-1] * 3] * N and _np(env.episode).tolist() == [1] * N and int(env.tstep.abs().max()) == 0
    want = MC.observation(goal, key, np.full((N, 3), -1))
    for m in range(3):
        assert tuple(obs[m].shape) == (N, MC.OBS_DIMS[m])
        np.testing.assert_array_equal(_np(obs[m]), want[m].astype(np.float32))
    env.reset()                                                    # the second reset draws stream (seed, 2)
    g2, k2 = MC.reset_draws(seed, 2, N, L)
    np.testing.assert_array_equal(_np(env.goal), g2)
    np.testing.assert_array_equal(_np(env.key), k2)
    # reset-on-done inside step() draws the same way
    e2 = _env(N, T=1, seed=seed, L=L)
    e2.step(torch.zeros(N, 3).cuda())
    np.testing.assert_array_equal(_np(e2.goal), goal)
    np.testing.assert_array_equal(_np(e2.key), key)


@pytest.mark.parametrize("N", [1, 37])
def test_partial_block_writes_nothing_beyond_N(gpu_device, N):
    """Every output and state array sits in front of a NaN (or sentinel) guard region; reset and both step modes leave it alone."""
    from mappo_amd import ops
    G = 64
    f32 = lambda *s: torch.full((N + G, *s), float("nan"), dtype=torch.float32, device="cuda")
    i32 = lambda *s: torch.full((N + G, *s), -77, dtype=torch.int32, device="cuda")
    goal, key, comm, tstep = i32(), i32(), i32(3), i32()
    ep = torch.full((N + G,), -77, dtype=torch.int64, device="cuda")
    ep[:N] = 0
    o0, o1, o2, rew = f32(4), f32(8), f32(8), f32(3)
    dones = torch.full((N + G, 3), 9, dtype=torch.uint8, device="cuda")
    ops.mpe_crypto_reset(goal, key, comm, tstep, ep, o0, o1, o2, N, 11, num_landmarks=3)
    idx = torch.stack([(torch.arange(N) + m) % 4 for m in range(3)], dim=1).float().cuda().contiguous()
    ops.mpe_crypto_step(goal, key, comm, tstep, ep, idx, 1, o0, o1, o2, rew, dones, N, 2, 11, num_landmarks=3)
    ops.mpe_crypto_step(goal, key, comm, tstep, ep, torch.eye(4, device="cuda")[idx.long()].contiguous(), 0, o0, o1, o2, rew, dones, N, 2, 11,
                        num_landmarks=3)
    torch.cuda.synchronize()
    for name, t in (("o0", o0), ("o1", o1), ("o2", o2), ("rew", rew)):
        assert bool(torch.isnan(t[N:]).all()), name
        assert bool(torch.isfinite(t[:N]).all()), name
    for name, t in (("goal", goal), ("key", key), ("comm", comm), ("tstep", tstep), ("episode", ep)):
        assert bool((t[N:] == -77).all()), name
    assert bool((dones[N:] == 9).all()) and bool((dones[:N] == 1).all())                            # episode length 2: done at the second step
    assert _np(ep[:N]).tolist() == [2] * N and _np(tstep[:N]).tolist() == [0] * N and _np(comm[:N]).tolist() == [[-1] * 3] * N
    assert int(goal[:N].min()) >= 0 and int(goal[:N].max()) < 3 and int(key[:N].min()) >= 0 and int(key[:N].max()) < 3


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
    a = _args(episode_length=T, n_rollout_threads=N, env_name="MPE", share_policy=False, use_hip_graph=False, seed=CR.SEED,
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
    real = ops.rollout_episode_crypto
    monkeypatch.setattr(ops, "rollout_episode_crypto", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


# ---- one launch == stepwise --------------------------------------------------------------------------------------------------------------------
# (N, (T, env T), layer_N, relu, centralized, L).  N: a partial tile | one short of a tile | a tile | one over | two tiles and one.
# (T, env T): one step | the episode ends on the rollout's last step | two resets inside the launch.  Every N takes the
# reset-crossing shape; every value of every other axis occurs with it and at least once more.
CASES = [
    (1, (14, 7), 1, True, True, 2),
    (15, (14, 7), 0, False, False, 4),
    (16, (14, 7), 1, False, True, 3),
    (17, (14, 7), 0, True, False, 2),
    (33, (14, 7), 1, True, False, 4),
    (33, (14, 7), 0, False, True, 2),
    (1, (1, 25), 0, False, True, 4),
    (17, (1, 25), 1, True, False, 3),
    (16, (25, 25), 1, False, False, 2),
    (33, (25, 25), 0, True, True, 4),
]


@pytest.mark.parametrize("N,TT,layer_N,relu,cen,L", CASES, ids=[f"N{c[0]}-T{c[1][0]}-envT{c[1][1]}-L{c[2]}-{'relu' if c[3] else 'tanh'}-"
                                                                f"{'cen' if c[4] else 'dec'}-{c[5]}lm" for c in CASES])
def test_one_launch_equals_stepwise(gpu_device, monkeypatch, N, TT, layer_N, relu, cen, L):
    T, env_T = TT
    calls = _count_calls(monkeypatch)
    runs = {}
    for flag in ("1", "1 again", "0"):
        monkeypatch.setenv("MAPPO_CRYPTO_EPISODE", flag[0])
        r = _runner(_env(N, env_T, L=L), T, N, layer_N=layer_N, use_ReLU=relu, use_centralized_V=cen)
        assert r._ragged and r._fused_ff() and r._episode_ready() == (flag[0] == "1")
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
    assert tuple(s["agent0/obs"].shape) == (T + 1, N, 4) and tuple(s["agent2/obs"].shape) == (T + 1, N, 8)
    assert tuple(s["agent1/share_obs"].shape) == (T + 1, N, 20 if cen else 8)
    assert set(s) >= {"env/goal", "env/key", "env/comm", "env/tstep", "env/episode"}
    resets = 2 * T // env_T                                        # over the two rollouts, besides warmup's
    assert _np(s["env/episode"]).tolist() == [1 + resets] * N and _np(s["env/tstep"]).tolist() == [2 * T % env_T] * N
    if resets:
        assert float(s["agent0/masks"][1:].min()) == 0.0
    assert torch.equal(s["agent1/rewards"], s["agent2/rewards"])
    vals = set(torch.cat([s[f"agent{m}/rewards"].flatten() for m in range(3)]).tolist())
    assert vals <= {-2.0, 0.0, 2.0}
    if N * T >= 64:
        assert not torch.equal(s["agent0/rewards"], s["agent1/rewards"])
        for m in range(3):
            assert len(torch.unique(s[f"agent{m}/actions"])) > 1


def _guarded_agents(r, obs, T, N, G, cen):
    """The three comm_agent(...) of runner r on buffers that sit between NaN guard regions -> (agents, views, [(full, n)])."""
    from mappo_amd import ops
    fulls = []

    def guarded(*shape):
        n = int(np.prod(shape))
        full = torch.full((n + 2 * G,), float("nan"), device="cuda")
        fulls.append((full, n))
        return full[G:G + n].view(*shape)
    ags, views = [], []
    for m, p in enumerate(r.policy):
        D = MC.OBS_DIMS[m]
        v = dict(obs=guarded(T + 1, N, D), share=guarded(T + 1, N, 20 if cen else D), rew=guarded(T, N, 1), mask=guarded(T + 1, N, 1),
                 act=guarded(T, N, 1), logp=guarded(T, N, 1), val=guarded(T + 1, N, 1), nv=guarded(N))
        v["obs"][0].copy_(obs[m]); v["share"][0].copy_(torch.cat(obs, dim=1) if cen else obs[m]); v["mask"][0].fill_(1.0)
        views.append(v)
        ags.append(ops.comm_agent(p.actor.flat, p.actor.desc, p.critic.flat, p.critic.desc, p.actor._seed, None, v["obs"], v["share"], v["rew"],
                                  v["mask"], v["act"], v["logp"], v["val"], v["nv"]))
    return ags, views, fulls


@pytest.mark.parametrize("N,layer_N,cen", [(37, 1, True), (37, 0, False), (1, 1, False)])
def test_one_launch_writes_nothing_outside_the_buffers(gpu_device, N, layer_N, cen):
    T, G = 3, 64
    env = _env(N, 2, L=3)
    r = _runner(env, T, N, layer_N=layer_N, use_centralized_V=cen)
    obs = env.reset()
    ags, views, fulls = _guarded_agents(r, obs, T, N, G, cen)
    # the env state behind sentinels as well: the launch loads and stores it
    st = {k: torch.full((v.shape[0] + G, *v.shape[1:]), -77, dtype=v.dtype, device="cuda") for k, v in env.state_tensors().items()}
    for k, v in env.state_tensors().items():
        st[k][:N].copy_(v)
    from mappo_amd import ops
    ops.rollout_episode_crypto(ags, T, N, env.T, env.seed, st["goal"], st["key"], st["comm"], st["tstep"], st["episode"], False, 0, cen,
                               num_landmarks=env.L)
    torch.cuda.synchronize()
    for full, n in fulls:
        assert bool(torch.isnan(full[:G]).all()) and bool(torch.isnan(full[G + n:]).all())
    for k, v in st.items():
        assert bool((v[N:] == -77).all()), k
    assert _np(st["episode"][:N]).tolist() == [2] * N and _np(st["tstep"][:N]).tolist() == [1] * N      # env length 2, 3 steps, from reset 1
    for v in views:
        for k in ("obs", "share", "rew", "mask", "act", "logp", "nv"):
            assert bool(torch.isfinite(v[k]).all()), k
        assert bool(torch.isfinite(v["val"][:T]).all()) and bool(torch.isnan(v["val"][T]).all())     # slot T belongs to nobody here


# ---- sampling against float64 + the host Philox ------------------------------------------------------------------------------------------
def _load_twins(r, tw):
    for m in range(3):
        r.policy[m].actor.load_state_dict(tw[m].actor.state_dict())
        r.policy[m].critic.load_state_dict(tw[m].critic.state_dict())
        assert r.policy[m].actor._seed == CR.agent_seed(m)


def _start_from_fixture(r, env):
    """The fixture's start in the env and in the mirror; warmup's slot 0 from the loaded state."""
    env.set_state(*CR.initial_state())
    mirror = MC.SimpleCryptoNp(*CR.initial_state(), episode_length=CR.ENV_T)
    o0 = mirror.obs()
    for m in range(3):
        r.buffer[m].obs[0].copy_(torch.from_numpy(o0[m].astype(np.float32)))
        r.buffer[m].share_obs[0].copy_(torch.from_numpy(np.concatenate(o0, axis=1).astype(np.float32)))
    return mirror


@pytest.mark.parametrize("flag", ["0", "1"], ids=["stepwise", "one-launch"])
def test_rollout_against_float64_and_host_philox(gpu_device, monkeypatch, flag):
    monkeypatch.setenv("MAPPO_CRYPTO_EPISODE", flag)
    N, T = CR.N, CR.T
    env = _env(N, CR.ENV_T, L=CR.L)
    r = _runner(env, T, N)
    tw = CR.twins()
    _load_twins(r, tw)
    r.warmup()
    mirror = _start_from_fixture(r, env)
    r.rollout()
    fails, near, pairs = [], 0, 0
    for t in range(T):
        acts = []
        for m in range(3):
            b = r.buffer[m]
            e, tol = CR.expected_step(tw[m].actor, _np(b.obs[t]), m, t)
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
    assert near <= CR.NEAR_CAP * pairs, f"{near} of {pairs} (row, agent) pairs left out"
    assert not fails, "\n".join(fails)
    np.testing.assert_array_equal(_np(env.comm), mirror.comm)
    np.testing.assert_array_equal(_np(env.goal), mirror.goal)
    np.testing.assert_array_equal(_np(env.key), mirror.key)


def test_deterministic_rollout_takes_the_argmax_in_both_paths(gpu_device, monkeypatch):
    N, T = CR.N, CR.T
    tw = CR.twins()
    snaps = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("MAPPO_CRYPTO_EPISODE", flag)
        env = _env(N, CR.ENV_T, L=CR.L)
        r = _runner(env, T, N)
        _load_twins(r, tw)
        r.warmup()
        _start_from_fixture(r, env)
        r.rollout(deterministic=True)
        snaps[flag] = _snapshot(r)
        fails = []
        for t in range(T):
            for m in range(3):
                b = r.buffer[m]
                e, tol = CR.expected_step(tw[m].actor, _np(b.obs[t]), m, t, deterministic=True)
                fails += R.check_actions(e, None, _np(b.actions[t, :, 0]), _np(b.action_log_probs[t, :, 0]), tol, f"step {t} agent {m}")
        assert not fails, "\n".join(fails)
    _assert_equal(snaps["0"], snaps["1"], "deterministic rollout, stepwise vs one launch")


# ---- training ---------------------------------------------------------------------------------------------------------------------------------
def test_runner_trains_three_agents_either_way(gpu_device, monkeypatch):
    """N = 8, T = 25, two iterations, stepwise and the default path: the buffers of the first rollout are identical, replaying their
    actions through the NumPy mirror from the initial state reproduces the stored observations and per-agent rewards, all three
    policies change and stay finite, train_infos has one entry per agent, and the two paths end in the same parameters, bit for bit."""
    N, T = 8, 25
    first, final = {}, {}
    for flag in ("0", None):
        if flag is None:
            monkeypatch.delenv("MAPPO_CRYPTO_EPISODE", raising=False)
        else:
            monkeypatch.setenv("MAPPO_CRYPTO_EPISODE", flag)
        env = _env(N, T, L=3)
        r = _runner(env, T, N)
        assert r._episode_ready() == (flag is None)                # the one-launch path is the default
        r.warmup()
        state0 = {k: _np(v).copy() for k, v in env.state_tensors().items()}
        before = [p.flat_params.clone() for p in r.policy]
        assert [p.actor.desc.in_dim for p in r.policy] == [4, 8, 8] and [p.actor.desc.out_dim for p in r.policy] == [4, 4, 4]
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
        final[flag] = [p.flat_params.clone() for p in r.policy]
        # replay the first rollout's actions through the mirror
        s = first[flag]
        mirror = MC.SimpleCryptoNp(state0["goal"], state0["key"], episode_length=T, comm=state0["comm"])
        o = mirror.obs()
        for m in range(3):
            np.testing.assert_array_equal(_np(s[f"agent{m}/obs"][0]), o[m].astype(np.float32))
        for t in range(T):
            acts = np.stack([_np(s[f"agent{m}/actions"][t, :, 0]).astype(np.int64) for m in range(3)], axis=1)
            o, rew, dones = mirror.step(acts)
            assert bool(dones.all()) == (t == T - 1)
            if t == T - 1:                                         # the episode ended: slot T holds the reset state's observations
                o = MC.observation(_np(s["env/goal"]).astype(np.int64), _np(s["env/key"]).astype(np.int64), _np(s["env/comm"]).astype(np.int64))
            share = np.concatenate(o, axis=1).astype(np.float32)
            for m in range(3):
                np.testing.assert_array_equal(_np(s[f"agent{m}/obs"][t + 1]), o[m].astype(np.float32), err_msg=f"obs, step {t}, agent {m}")
                np.testing.assert_array_equal(_np(s[f"agent{m}/share_obs"][t + 1]), share, err_msg=f"share_obs, step {t}, agent {m}")
                np.testing.assert_array_equal(_np(s[f"agent{m}/rewards"][t, :, 0]), rew[:, m].astype(np.float32),
                                              err_msg=f"rewards, step {t}, agent {m}")
                np.testing.assert_array_equal(_np(s[f"agent{m}/masks"][t + 1, :, 0]), 1.0 - dones[:, m].astype(np.float32))
        assert not torch.equal(s["agent0/rewards"], s["agent1/rewards"])
    _assert_equal(first["0"], first[None], "first rollout, stepwise vs the default path")
    for m in range(3):
        assert torch.equal(final["0"][m], final[None][m]), f"agent {m}: the two paths end in different parameters"
