"""The separated MPE runner on simple_speaker_listener — two agents of different shapes: the stepwise rollout against float64 and
the host Philox (tests/rollout_ref.py through tests/comm_rollout_ref.py), the reference's ragged host contract against the device
env, the one-launch episode (mappo_rollout_episode_comm) bit for bit against the stepwise path, when it is taken, training, and
per-agent save / restore."""
import os

import numpy as np
import pytest
import torch

import comm_rollout_ref as CR
import mpe_comm_np as MC
import rollout_ref as R

pytestmark = pytest.mark.gpu

NAMES = ("share_obs", "obs", "rnn_states", "rnn_states_critic", "value_preds", "returns", "actions", "action_log_probs", "rewards",
         "masks", "bad_masks", "active_masks")
STATE = ("listener_pos", "listener_vel", "landmark_pos", "goal", "symbol", "tstep", "episode")


def _args(**kw):
    from mappo_amd.config import get_config
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = False
    a.use_naive_recurrent_policy = False
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def _env(N, T, seed=3):
    from mappo_amd.envs import SimpleSpeakerListenerVecEnv
    return SimpleSpeakerListenerVecEnv(N, episode_length=T, seed=seed)


def _runner(env, T, N, algo="mappo", run_dir=None, **kw):
    from mappo_amd.runner.separated.mpe_runner import MPERunner
    a = _args(episode_length=T, n_rollout_threads=N, env_name="MPE", share_policy=False, use_hip_graph=False, seed=CR.SEED,
              algorithm_name=algo, use_recurrent_policy=(algo == "rmappo"), ppo_epoch=2, num_mini_batch=1, **kw)
    torch.manual_seed(1)
    return MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=2, device=torch.device("cuda"), run_dir=run_dir))


def _snapshot(r):
    out = {}
    for m, b in enumerate(r.buffer):
        for n in NAMES:
            if getattr(b, n) is not None:
                out[f"agent{m}/{n}"] = getattr(b, n).clone()
        out[f"agent{m}/next_values"] = r._next_values[m].clone()
    if hasattr(r.envs, "state_tensors"):
        out.update({f"env/{k}": v.clone() for k, v in r.envs.state_tensors().items()})
    return out


def _assert_equal(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs ({(a[k] != b[k]).sum().item()} of {a[k].numel()} elements)"


# ---- stepwise rollout against float64 + host Philox ----------------------------------------------------------------------------------
def test_stepwise_rollout_against_float64(gpu_device, monkeypatch):
    monkeypatch.setenv("MAPPO_COMM_EPISODE", "0")
    N, T = CR.N, CR.T
    env = _env(N, CR.ENV_T)
    r = _runner(env, T, N)
    tw = CR.twins()
    for m in range(2):
        r.policy[m].actor.load_state_dict(tw[m].actor.state_dict())
        r.policy[m].critic.load_state_dict(tw[m].critic.state_dict())
        assert r.policy[m].actor._seed == CR.agent_seed(m)
    assert r._ragged and r._fused_ff()
    r.warmup()
    env.set_state(*CR.initial_state())
    mirror = MC.SimpleSpeakerListenerNp(*CR.initial_state(), episode_length=CR.ENV_T)
    o0 = mirror.obs()
    for m in range(2):                                             # warmup's slot 0, from the loaded state
        r.buffer[m].obs[0].copy_(torch.from_numpy(o0[m].astype(np.float32)))
        r.buffer[m].share_obs[0].copy_(torch.from_numpy(np.concatenate(o0, axis=1).astype(np.float32)))
    r.rollout()
    fails = []
    for t in range(T):
        acts = []
        for m in range(2):
            b = r.buffer[m]
            obs = b.obs[t].cpu().numpy()
            e, tol = CR.expected_step(tw[m].actor, obs, m, t)
            a, lp = b.actions[t, :, 0].cpu().numpy(), b.action_log_probs[t, :, 0].cpu().numpy()
            print(f"step {t} agent {m}: tol {tol:.2e}, max log-prob error {R.max_logp_err(e, a, lp):.2e}, near rows {int(e.near.sum())}")
            fails += R.check_actions(e, None, a, lp, tol, f"step {t} agent {m}")
            v64, _ = R.critic_eval(tw[m].critic, b.share_obs[t].cpu().numpy(), dtype=torch.float64)
            v32, _ = R.critic_eval(tw[m].critic, b.share_obs[t].cpu().numpy(), dtype=torch.float32)
            _, tol_v = R.err_and_tol(v64, v32)
            dv = float(np.abs(b.value_preds[t, :, 0].cpu().numpy() - v64).max())
            print(f"step {t} agent {m}: value tol {tol_v:.2e}, max error {dv:.2e}")
            if dv > tol_v:
                fails.append(f"step {t} agent {m}: value off by {dv:.3e} > {tol_v:.3e}")
            acts.append(a.astype(np.int64))
        os_, ol, rew, dones = mirror.step(np.eye(3)[acts[0]], np.eye(5)[acts[1]])
        share = np.concatenate([os_, ol], axis=1).astype(np.float32)
        for m, o in enumerate((os_, ol)):
            b = r.buffer[m]
            np.testing.assert_array_equal(b.obs[t + 1].cpu().numpy(), o.astype(np.float32), err_msg=f"obs, step {t}, agent {m}")
            np.testing.assert_array_equal(b.share_obs[t + 1].cpu().numpy(), share, err_msg=f"share_obs, step {t}, agent {m}")
            np.testing.assert_array_equal(b.rewards[t, :, 0].cpu().numpy(), rew[:, m].astype(np.float32), err_msg=f"rewards, step {t}")
            np.testing.assert_array_equal(b.masks[t + 1, :, 0].cpu().numpy(), 1.0 - dones[:, m].astype(np.float32))
    assert not fails, "\n".join(fails)
    np.testing.assert_array_equal(env.listener_pos.cpu().numpy(), mirror.pos)
    np.testing.assert_array_equal(env.listener_vel.cpu().numpy(), mirror.vel)


@pytest.mark.parametrize("flag", ["0", "1"], ids=["stepwise", "one-launch"])
def test_every_rollout_draws_from_a_fresh_counter(gpu_device, monkeypatch, flag):
    """The runner advances each agent's counter word by T before a rollout: step t of the k-th rollout samples with counter
    k T + t — held against the host Philox and the float64 policy on the rows the buffer holds, in both paths."""
    monkeypatch.setenv("MAPPO_COMM_EPISODE", flag)
    N, T = CR.N, CR.T
    r = _runner(_env(N, CR.ENV_T), T, N)
    tw = CR.twins()
    for m in range(2):
        r.policy[m].actor.load_state_dict(tw[m].actor.state_dict())
        r.policy[m].critic.load_state_dict(tw[m].critic.state_dict())
    r.warmup()
    fails, drawn = [], []
    for k in (1, 2):
        r.rollout()
        assert [int(p.actor._counter_dev.item()) for p in r.policy] == [k * T, k * T]
        for m in range(2):
            b = r.buffer[m]
            for t in range(T):
                e, tol = CR.expected_step(tw[m].actor, b.obs[t].cpu().numpy(), m, t, rollout=k)
                assert e.near.mean() <= CR.NEAR_CAP
                fails += R.check_actions(e, None, b.actions[t, :, 0].cpu().numpy(), b.action_log_probs[t, :, 0].cpu().numpy(), tol,
                                         f"rollout {k} step {t} agent {m}")
        drawn.append(np.stack([R.uniform24(CR.agent_seed(0), k * T + t, np.arange(N)) for t in range(T)]))
        for b in r.buffer:
            b.after_update()
    assert not fails, "\n".join(fails)
    assert not np.array_equal(drawn[0], drawn[1])


# ---- the reference's ragged host contract ----------------------------------------------------------------------------------------------
class HostSpeakerListener:
    """The NumPy mirror behind the reference's vec-env contract for agents of different shapes: observations are an object array
    [N, M] of per-agent arrays, actions a per-agent list of NumPy one-hots."""

    def __init__(self, dev_env):
        self.N, self.M = dev_env.N, 2
        self.observation_space, self.share_observation_space = dev_env.observation_space, dev_env.share_observation_space
        self.action_space = dev_env.action_space
        self.env = MC.SimpleSpeakerListenerNp(dev_env.listener_pos.cpu().numpy(), dev_env.listener_vel.cpu().numpy(),
                                              dev_env.landmark_pos.cpu().numpy(), dev_env.goal.cpu().numpy(), dev_env.T)
        self.seen = []

    def _pack(self, os_, ol):
        obs = np.empty((self.N, self.M), dtype=object)
        for n in range(self.N):
            obs[n, 0], obs[n, 1] = os_[n], ol[n]
        return obs

    def reset(self):
        return self._pack(*self.env.obs())

    def step(self, actions):
        assert isinstance(actions, list) and len(actions) == 2 and all(isinstance(a, np.ndarray) for a in actions)
        assert actions[0].shape == (self.N, 3) and actions[1].shape == (self.N, 5)
        self.seen.append([a.copy() for a in actions])
        os_, ol, rew, dones = self.env.step(*actions)
        return self._pack(os_, ol), rew[..., None], dones, [{} for _ in range(self.N)]


@pytest.mark.parametrize("cen", [True, False])
def test_host_env_equals_device_env(gpu_device, monkeypatch, cen):
    monkeypatch.setenv("MAPPO_COMM_EPISODE", "0")
    N, T = 5, 4
    dev_env = _env(N, 25)
    rd = _runner(dev_env, T, N, use_centralized_V=cen)
    rd.warmup()
    host = HostSpeakerListener(dev_env)
    rh = _runner(host, T, N, use_centralized_V=cen)
    assert rh._ragged and rh._fused_ff() and not rh._comm_episode_ready()
    rh.warmup()
    rd.rollout(); rh.rollout()
    a, b = _snapshot(rd), _snapshot(rh)
    a = {k: v for k, v in a.items() if not k.startswith("env/")}
    _assert_equal(a, b, "host env vs device env")
    assert len(host.seen) == T and all((s[0].sum(1) == 1).all() and (s[1].sum(1) == 1).all() for s in host.seen)
    np.testing.assert_array_equal(dev_env.listener_pos.cpu().numpy(), host.env.pos)


# ---- one launch == stepwise ------------------------------------------------------------------------------------------------------------
#        N   T  envT  layer_N  relu   cen    det
CASES = [(5, 3, 25, 1, True, True, False),
         (16, 3, 25, 0, True, True, False),
         (37, 3, 25, 1, False, True, False),
         (37, 6, 4, 0, False, False, False),
         (5, 6, 4, 1, True, False, True),
         (16, 3, 25, 1, False, True, True),
         (37, 6, 4, 1, True, True, False),
         (5, 3, 25, 0, False, False, True)]


@pytest.mark.parametrize("N,T,env_T,layer_N,relu,cen,det", CASES, ids=[f"N{c[0]}-T{c[1]}-envT{c[2]}-L{c[3]}-{'relu' if c[4] else 'tanh'}-"
                                                                       f"{'cen' if c[5] else 'dec'}-{'det' if c[6] else 'sample'}" for c in CASES])
def test_one_launch_equals_stepwise(gpu_device, monkeypatch, N, T, env_T, layer_N, relu, cen, det):
    from mappo_amd import ops
    calls = []
    real = ops.rollout_episode_comm
    monkeypatch.setattr(ops, "rollout_episode_comm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    runs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("MAPPO_COMM_EPISODE", flag)
        r = _runner(_env(N, env_T), T, N, layer_N=layer_N, use_ReLU=relu, use_centralized_V=cen)
        r.warmup()
        snaps = []
        for it in range(2):                                        # the second episode continues from the first one's state
            n0 = len(calls)
            r.rollout(deterministic=det)
            assert len(calls) - n0 == (1 if flag == "1" else 0)
            snaps.append(_snapshot(r))
            for b in r.buffer:
                b.after_update()
        runs[flag] = snaps
    for it in range(2):
        _assert_equal(runs["1"][it], runs["0"][it], f"episode {it}")
    s = runs["1"][1]
    assert all(bool(torch.isfinite(v).all()) for k, v in s.items() if v.is_floating_point())
    if env_T < T:                                                  # a reset fell inside the rollout
        assert int(s["env/episode"].min()) >= 2 and float(s["agent0/masks"][1:].min()) == 0.0
    if not det:
        assert len(torch.unique(s["agent0/actions"])) > 1 and len(torch.unique(s["agent1/actions"])) > 1


def test_one_launch_writes_nothing_outside_the_buffers(gpu_device):
    from mappo_amd import ops
    N, T, G = 37, 3, 64
    env = _env(N, 2)
    r = _runner(env, T, N)
    obs = env.reset()
    fulls = []

    def guarded(*shape):
        n = int(np.prod(shape))
        full = torch.full((n + 2 * G,), float("nan"), device="cuda")
        fulls.append((full, n))
        return full[G:G + n].view(*shape)
    ags, views = [], []
    for m, p in enumerate(r.policy):
        D = (3, 11)[m]
        v = dict(obs=guarded(T + 1, N, D), share=guarded(T + 1, N, 14), rew=guarded(T, N, 1), mask=guarded(T + 1, N, 1), act=guarded(T, N, 1),
                 logp=guarded(T, N, 1), val=guarded(T + 1, N, 1), nv=guarded(N))
        v["obs"][0].copy_(obs[m]); v["share"][0].copy_(torch.cat(obs, dim=1)); v["mask"][0].fill_(1.0)
        views.append(v)
        ags.append(ops.comm_agent(p.actor.flat, p.actor.desc, p.critic.flat, p.critic.desc, p.actor._seed, None, v["obs"], v["share"], v["rew"],
                                  v["mask"], v["act"], v["logp"], v["val"], v["nv"]))
    st = env.episode_state_comm()
    ops.rollout_episode_comm(ags[0], ags[1], T, N, st["T"], st["seed"], st["listener_pos"], st["listener_vel"], st["landmark_pos"], st["goal"],
                             st["symbol"], st["tstep"], st["episode"], False, 0, True)
    torch.cuda.synchronize()
    for full, n in fulls:
        assert bool(torch.isnan(full[:G]).all()) and bool(torch.isnan(full[G + n:]).all())
    for v in views:
        for k in ("obs", "share", "rew", "mask", "act", "logp", "nv"):
            assert bool(torch.isfinite(v[k]).all()), k
        assert bool(torch.isfinite(v["val"][:T]).all()) and bool(torch.isnan(v["val"][T]).all())     # slot T belongs to nobody here


# ---- when the fast path is taken ---------------------------------------------------------------------------------------------------------
def test_fast_path_is_taken_only_where_it_applies(gpu_device, monkeypatch):
    from mappo_amd import ops
    calls = []
    real = ops.rollout_episode_comm
    monkeypatch.setattr(ops, "rollout_episode_comm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.delenv("MAPPO_COMM_EPISODE", raising=False)
    N, T = 8, 6

    def run(env=None, **kw):
        env = env or _env(N, T)
        r = _runner(env, T, N, **kw)
        r.warmup()
        n0 = len(calls)
        infos, _ = r.run_episode()
        assert len(infos) == 2
        return len(calls) - n0
    assert run() == 1
    assert run(layer_N=2) == 0
    assert run(algo="rmappo", data_chunk_length=3) == 0
    dev_env = _env(N, T)
    dev_env.reset()
    assert run(env=HostSpeakerListener(dev_env)) == 0
    monkeypatch.setenv("MAPPO_COMM_EPISODE", "0")
    assert run() == 0


# ---- eval ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True], ids=["device-env", "host-object-arrays"])
def test_eval_on_agents_of_different_shapes(gpu_device, capsys, host):
    """eval() follows the rules of the rollout: per-agent observations, per-agent action widths, indices for the device env and a
    per-agent list of NumPy one-hots for a host env.  Deterministic, so the host mirror started from the device env's state sees the
    same episode: equal rewards."""
    N, T = 6, 4
    r = _runner(_env(N, 25), T, N)
    dev_eval = _env(N, 25, seed=9)
    dev_eval.reset()
    host_eval = HostSpeakerListener(dev_eval)
    state0 = {k: v.clone() for k, v in dev_eval.state_tensors().items()}
    seen = []
    step = dev_eval.step
    dev_eval.step = lambda a: (seen.append(a), step(a))[1]
    reset = dev_eval.reset

    def same_reset():                                              # eval() resets its envs: keep the state the mirror was built from
        obs = reset()
        for k, v in state0.items():
            getattr(dev_eval, k).copy_(v)
        o = host_eval.env.obs()
        obs[0].copy_(torch.from_numpy(o[0].astype(np.float32))); obs[1].copy_(torch.from_numpy(o[1].astype(np.float32)))
        return obs
    dev_eval.reset = same_reset
    r.eval_envs = host_eval if host else dev_eval
    r.eval(0)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("eval average episode rewards of agent")]
    assert len(lines) == 2 and lines[0].startswith("eval average episode rewards of agent0") and lines[1].startswith(
        "eval average episode rewards of agent1")
    avg = [float(l.split(": ")[1]) for l in lines]
    assert all(np.isfinite(avg)) and avg[0] < 0 and avg[0] == avg[1]                               # collaborative: the same reward
    if host:
        assert len(host_eval.seen) == T
        test_eval_on_agents_of_different_shapes.host_avg = avg
    else:
        assert len(seen) == T and all(torch.is_tensor(a) and tuple(a.shape) == (N, 2) for a in seen)
        # the same deterministic episode on the mirror, driven by the indices the device env was handed
        total = np.zeros(N)
        for a in seen:
            a = a.cpu().numpy().astype(np.int64)
            _, _, rew, _ = host_eval.env.step(np.eye(3)[a[:, 0]], np.eye(5)[a[:, 1]])
            total += rew[:, 0].astype(np.float32)
        assert abs(avg[0] - float(total.mean())) < 1e-4 * abs(avg[0])


# ---- training ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["mappo", "rmappo"])
def test_training_two_iterations(gpu_device, algo):
    N, T = 8, 6
    env = _env(N, T)
    r = _runner(env, T, N, algo=algo, data_chunk_length=3)
    r.warmup()
    before = [p.flat_params.clone() for p in r.policy]
    assert before[0].numel() != before[1].numel() or r.policy[0].actor.n_params != r.policy[1].actor.n_params
    assert r.policy[0].actor.n_params != r.policy[1].actor.n_params and r.policy[0].actor.desc.in_dim == 3
    for it in range(2):
        infos, _ = r.run_episode(it, 2)
        assert len(infos) == 2
        for m, info in enumerate(infos):
            for k, v in info.items():
                assert np.isfinite(float(v)), (algo, it, m, k, v)
    for m, p in enumerate(r.policy):
        a0, a1 = before[m][:p.actor.n_params], p.flat_params[:p.actor.n_params]
        lo = p.seg_bounds[1]
        c0, c1 = before[m][lo:lo + p.critic.n_params], p.flat_params[lo:lo + p.critic.n_params]
        assert not torch.equal(a0, a1) and not torch.equal(c0, c1), f"agent {m}: parameters did not change"
        assert bool(torch.isfinite(p.flat_params).all())
    assert 0 <= int(env.tstep.min()) and int(env.tstep.max()) < T
    for k, v in env.state_tensors().items():
        if v.is_floating_point():
            assert bool(torch.isfinite(v).all()), k
    assert int(env.episode.min()) >= 2 and set(env.goal.cpu().tolist()) <= {0, 1, 2}


# ---- save / restore -------------------------------------------------------------------------------------------------------------------------
def test_save_and_restore_per_agent_files(gpu_device, tmp_path):
    N, T = 4, 3
    r = _runner(_env(N, T), T, N)
    r.save_dir = str(tmp_path)
    for p in r.policy:
        p.flat_params.add_(torch.randn_like(p.flat_params) * 0.01)
    r.save()
    for m in range(2):
        assert os.path.exists(tmp_path / f"actor_agent{m}.pt") and os.path.exists(tmp_path / f"critic_agent{m}.pt")
    sd0 = torch.load(tmp_path / "actor_agent0.pt", weights_only=True)
    sd1 = torch.load(tmp_path / "actor_agent1.pt", weights_only=True)
    assert sd0["base.mlp.fc1.0.weight"].shape[1] == 3 and sd1["base.mlp.fc1.0.weight"].shape[1] == 11
    r2 = _runner(_env(N, T), T, N, model_dir=str(tmp_path))
    for m in range(2):
        for net in ("actor", "critic"):
            a, b = getattr(r.policy[m], net).state_dict(), getattr(r2.policy[m], net).state_dict()
            assert a.keys() == b.keys()
            for k in a:
                assert torch.equal(a[k], b[k]), (m, net, k)
