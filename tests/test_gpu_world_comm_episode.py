"""The one-launch rollout episode on MPE simple_world_comm (mappo_rollout_episode_world_comm, csrc/rollout_world_comm.h): bit for bit
against the stepwise twin built from the C ABI (tests/world_comm_rollout_ref.py) from states with a contact, a speed clamp, a shared
forest and a good agent out of bounds in the first steps; actions, log-probs, observations and rewards against float64 oracle
actors, the host Philox and the NumPy mirror; the values against the policy's own critic forward and a float64 critic;
guard floats around every output; the leader's word in the adversaries' observations; the opt-in runner path; the host's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import rollout_ref as R
import world_comm_rollout_ref as WR

pytestmark = pytest.mark.gpu

FLAG = "MAPPO_WORLD_COMM_EPISODE"


def _env(N, T=25, seed=3):
    from mappo_amd.envs import SimpleWorldCommVecEnv
    return SimpleWorldCommVecEnv(N, episode_length=T, seed=seed)


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
    a = _args(episode_length=T, n_rollout_threads=N, env_name="MPE", share_policy=False, use_hip_graph=False, seed=1, algorithm_name="mappo",
              ppo_epoch=2, num_mini_batch=1, **kw)
    torch.manual_seed(1)
    return MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=6, device=torch.device("cuda"), run_dir=None))


def _load_state(r, env, state, cen):
    """Explicit state into the env and its observations into slot 0 of the buffers (what warmup() did for the reset state)."""
    env.set_state(*state)
    o, share = WR.slot0(state)
    for m in range(6):
        r.buffer[m].obs[0].copy_(torch.from_numpy(o[m]))
        r.buffer[m].share_obs[0].copy_(torch.from_numpy(share if cen else o[m]))


def _count_calls(monkeypatch):
    from mappo_amd import ops
    calls = []
    real = ops.rollout_episode_world_comm
    monkeypatch.setattr(ops, "rollout_episode_world_comm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


# N: one row | a full tile | a full tile + one row | two tiles + a partial one; (T, env T): no reset | two resets inside the rollout;
# every value of layer_N, activation and critic input at least once
CASES = [(1, (3, 25), 1, True, True), (16, (5, 2), 0, False, False), (17, (3, 25), 1, False, True), (37, (5, 2), 1, True, False),
         (37, (3, 25), 0, True, True), (17, (5, 2), 1, False, False), (16, (3, 25), 0, False, True), (1, (5, 2), 0, True, False)]


@pytest.mark.parametrize("N,TT,layer_N,relu,cen", CASES, ids=[f"N{c[0]}-T{c[1][0]}-envT{c[1][1]}-L{c[2]}-{'relu' if c[3] else 'tanh'}-"
                                                              f"{'cen' if c[4] else 'dec'}" for c in CASES])
def test_one_launch_equals_stepwise_twin(gpu_device, monkeypatch, N, TT, layer_N, relu, cen):
    T, env_T = TT
    calls = _count_calls(monkeypatch)
    monkeypatch.setenv(FLAG, "1")
    env = _env(N, env_T)
    r = _runner(env, T, N, layer_N=layer_N, use_ReLU=relu, use_centralized_V=cen)
    assert r._ragged and not r._fused_ff() and r._episode_ready()
    if cen:         # a throwaway narrow critic per agent, of the same layer_N and activation
        rd = _runner(_env(N, env_T), T, N, layer_N=layer_N, use_ReLU=relu, use_centralized_V=False)
        narrow = [(p.critic.flat, p.critic.desc) for p in rd.policy]
    else:
        narrow = [(p.critic.flat, p.critic.desc) for p in r.policy]
    r.warmup()
    _load_state(r, env, WR.start_state(N), cen)
    twin = WR.Twin(r, env.state_tensors(), narrow)
    for it in range(2):                                            # the second episode continues from the first one's state
        r.rollout()                                                # advances every agent's counter word, then launches
        assert len(calls) == it + 1
        twin.rollout(T, env_T, env.seed, cen)
        for m, b in enumerate(r.buffer):
            for n in WR.NAMES:
                x, y = getattr(b, n), twin.buf[m][n]
                assert torch.equal(x, y), f"episode {it}, agent {m}: {n} differs ({(x != y).sum().item()} of {x.numel()} elements)"
            # the values: the policy's critic forward, called once on the same (T + 1) N rows
            rows = (T + 1) * N
            v = torch.empty(rows, 1, device="cuda")
            r.policy[m].critic(b.share_obs.view(rows, -1), b.rnn_states_critic[-1], b.masks[-1], out=v)
            assert torch.equal(b.value_preds.view(rows, 1), v), f"episode {it}, agent {m}: value_preds"
            assert bool(torch.isfinite(b.value_preds).all()) and bool(torch.isfinite(b.returns).all())
        for k, v in env.state_tensors().items():
            assert torch.equal(v, twin.state[k]), f"episode {it}: env state {k} differs"
        for b in r.buffer:
            b.after_update()
        twin.after_update()
    b0, b1 = r.buffer[0], r.buffer[1]
    assert tuple(b0.actions.shape) == (T, N, 2) and tuple(b1.actions.shape) == (T, N, 1)
    assert tuple(b0.obs.shape) == (T + 1, N, 34) and tuple(r.buffer[5].share_obs.shape) == (T + 1, N, 192 if cen else 28)
    if env_T < T:
        assert int(env.episode.min()) >= 2 * (T // env_T) and float(b0.masks[1:].min()) == 0.0


def test_the_first_steps_hold_the_physics_they_were_built_for(gpu_device, monkeypatch):
    """The start states' contact, clamp, shared forest and out-of-bounds good agent show in slot 1 of the launch's buffers, and the
    leader's word of step t is the last four features of every adversary's obs[t + 1] — zeros where the env reset."""
    N, T, env_T = 17, 5, 3
    monkeypatch.setenv(FLAG, "1")
    env = _env(N, env_T)
    r = _runner(env, T, N, use_centralized_V=True)
    r.warmup()
    _load_state(r, env, WR.start_state(N), True)
    r.rollout()
    b = r.buffer
    v1 = b[1].obs[1, :, 0:2].double()
    assert float((v1.norm(dim=1) - 1.0).abs().max()) < 1e-6                    # adversary 1 was clamped to speed 1
    # slot 1, the launch's own output: adversaries 2 and 3 moved 0.1 at the most from 0.05 / 0.07 off forest 0's centre (radius 0.3 +
    # 0.075), adversary 1 from 0.6 off it — two inside, the third outside
    assert bool((b[2].obs[1, :, 28] == 1.0).all()) and bool((b[3].obs[1, :, 28] == 1.0).all()) and bool((b[1].obs[1, :, 28] == -1.0).all())
    # the contact: the leader started 0.1 from good agent 4 (contact distance 0.12) at rest relative to nothing: the pair moved, and
    # wherever it is still within 0.12 after the step every adversary was paid 5 for it.  (The force itself is held to the NumPy
    # mirror from these same start states in test_launch_against_float64_actors_host_philox_and_the_mirror.)
    d1 = b[0].obs[1, :, 20:22].double().norm(dim=1)                             # good agent 4 relative to the leader, slot 1
    assert bool(((d1 - 0.1).abs() > 1e-4).all())
    for m in range(4):
        assert bool((b[m].rewards[0, :, 0][d1 < 0.12] > 4.0).all()), f"adversary {m}"
    assert float(b[5].rewards[0].max()) < -2.0                                 # beyond 1 on y: the penalty's exp branch
    word = torch.nn.functional.one_hot(b[0].actions[:, :, 1].long(), 4).float()
    word = word * b[0].masks[1:]                                               # zeros where the env reset
    assert float(b[0].masks[1:].min()) == 0.0 and float(b[0].masks[1:].max()) == 1.0
    for m in range(4):
        assert torch.equal(b[m].obs[1:, :, 30:34], word), f"adversary {m}"
    # the critics ran after the launch: against the float64 oracle critic on the launch's share rows, within rollout_ref's tolerance
    from oracle import mappo_oracle as O
    oa = O.default_args(episode_length=T, n_rollout_threads=N, use_centralized_V=True)
    for m in range(6):
        ref = O.CriticRef(oa, 192)
        ref.load_state_dict(r.policy[m].critic.state_dict())
        x = b[m].share_obs.view((T + 1) * N, -1).cpu().numpy()
        v64, _ = R.critic_eval(ref, x, dtype=torch.float64)
        v32, _ = R.critic_eval(ref, x, dtype=torch.float32)
        _, tol = R.err_and_tol(v64, v32)
        dv = float(np.abs(b[m].value_preds.view(-1).cpu().numpy() - v64).max())
        print(f"agent {m}: value tol {tol:.2e}, max error {dv:.2e}")
        assert dv <= tol, f"agent {m}: value off by {dv:.3e} > {tol:.3e}"


def test_launch_against_float64_actors_host_philox_and_the_mirror(gpu_device, monkeypatch):
    """Nothing here shares code with the kernels: float64 oracle actors (the leader's two heads over logits [0, 5) and [5, 9)), the
    host Philox with counter rollout * T + t and index (k << 32) | n, the NumPy mirror of the env.  Rows within the exclusion margin
    may take the boundary's neighbour; at most NEAR_CAP of the (row, agent) pairs are such rows."""
    monkeypatch.setenv(FLAG, "1")
    N, T = WR.REF_N, WR.REF_T
    env = _env(N, WR.REF_ENV_T)
    r = _runner(env, T, N)
    tw = WR.oracle_twins()
    for m in range(6):
        r.policy[m].actor.load_state_dict(WR.runner_actor_state(tw[m].actor, m))
        r.policy[m].critic.load_state_dict(tw[m].critic.state_dict())
        assert r.policy[m].actor._seed == WR.agent_seed(m)
    assert r._episode_ready()
    r.warmup()
    state = WR.start_state(N)
    _load_state(r, env, state, True)
    mirror = WR.MW.SimpleWorldCommNp(*state, episode_length=WR.REF_ENV_T)
    r.rollout()
    TOL = dict(rtol=1e-6, atol=1e-6)                               # env outputs against the mirror: tests/test_gpu_mpe_world_comm.py
    fails, near, pairs = [], 0, 0
    for t in range(T):
        cols = []
        for m in range(6):
            b = r.buffer[m]
            es, tol = WR.expected_step(tw[m].actor, b.obs[t].cpu().numpy(), m, t)
            row_near = np.zeros(N, bool)
            for k, e in enumerate(es):
                a, lp = b.actions[t, :, k].cpu().numpy(), b.action_log_probs[t, :, k].cpu().numpy()
                print(f"step {t} agent {m} head {k}: tol {tol:.2e}, max log-prob error {R.max_logp_err(e, a, lp):.2e}, near rows {int(e.near.sum())}")
                fails += R.check_actions(e, None, a, lp, tol, f"step {t} agent {m} head {k}")
                row_near |= e.near
                cols.append(a.astype(np.int64))
            near += int(row_near.sum()); pairs += N
        obs, rew, dones = mirror.step(np.stack(cols, axis=1))
        share = np.concatenate(obs, axis=1).astype(np.float32)
        for m in range(6):
            b = r.buffer[m]
            np.testing.assert_allclose(b.obs[t + 1].cpu().numpy(), obs[m].astype(np.float32), err_msg=f"obs, step {t}, agent {m}", **TOL)
            np.testing.assert_allclose(b.share_obs[t + 1].cpu().numpy(), share, err_msg=f"share_obs, step {t}, agent {m}", **TOL)
            np.testing.assert_allclose(b.rewards[t, :, 0].cpu().numpy(), rew[:, m].astype(np.float32), err_msg=f"rewards, step {t}, agent {m}", **TOL)
            np.testing.assert_array_equal(b.masks[t + 1, :, 0].cpu().numpy(), 1.0 - dones[:, m].astype(np.float32))
    assert near <= WR.NEAR_CAP * pairs, f"{near} of {pairs} (row, agent) pairs left out"
    assert not fails, "\n".join(fails)


def test_one_launch_writes_nothing_outside_the_buffers(gpu_device, monkeypatch):
    from mappo_amd import ops
    monkeypatch.setenv(FLAG, "1")                                   # the env has episode_launch only where the run opted in
    N, T, G, cen = 17, 3, 64, True
    env = _env(N, 2)
    r = _runner(env, T, N, layer_N=1, use_centralized_V=cen)
    obs = env.reset()
    fulls = []

    def guarded(*shape):
        n = int(np.prod(shape))
        full = torch.full((n + 2 * G,), float("nan"), device="cuda")
        fulls.append((full, n))
        return full[G:G + n].view(*shape)
    ags, views = [], []
    for m, p in enumerate(r.policy):
        D, K = WR.OBS_DIMS[m], 2 if m == 0 else 1
        v = dict(obs=guarded(T + 1, N, D), share=guarded(T + 1, N, 192), rew=guarded(T, N, 1), mask=guarded(T + 1, N, 1),
                 act=guarded(T, N, K), logp=guarded(T, N, K), val=guarded(T + 1, N, 1), nv=guarded(N))
        v["obs"][0].copy_(obs[m]); v["share"][0].copy_(torch.cat(obs, dim=1)); v["mask"][0].fill_(1.0)
        views.append(v)
        ags.append(ops.comm_agent(p.actor.flat, p.actor.desc, p.critic.flat, p.critic.desc, p.actor._seed, None, v["obs"], v["share"], v["rew"],
                                  v["mask"], v["act"], v["logp"], v["val"], v["nv"]))
    env.episode_launch(ags, T, False, 0, cen)
    torch.cuda.synchronize()
    for full, n in fulls:
        assert bool(torch.isnan(full[:G]).all()) and bool(torch.isnan(full[G + n:]).all())
    for v in views:
        for k in ("obs", "share", "rew", "mask", "act", "logp"):
            assert bool(torch.isfinite(v[k]).all()), k
        assert bool(torch.isnan(v["val"]).all()) and bool(torch.isnan(v["nv"]).all())      # the launch leaves the values to the caller


def test_runner_takes_the_launch_only_when_asked_and_trains(gpu_device, monkeypatch):
    N, T = 16, 5
    calls = _count_calls(monkeypatch)
    monkeypatch.setenv(FLAG, "1")
    r = _runner(_env(N, T), T, N)
    assert r._episode_ready()
    r.warmup()
    before = [p.flat_params.clone() for p in r.policy]
    for it in range(2):
        r.rollout()
        assert len(calls) == it + 1
        infos = r.train()
        assert len(infos) == 6
        for m, info in enumerate(infos):
            for k, v in info.items():
                assert np.isfinite(float(v)), (it, m, k, v)
    for m, p in enumerate(r.policy):
        a0, a1 = before[m][:p.actor.n_params], p.flat_params[:p.actor.n_params]
        lo = p.seg_bounds[1]
        c0, c1 = before[m][lo:lo + p.critic.n_params], p.flat_params[lo:lo + p.critic.n_params]
        assert not torch.equal(a0, a1) and not torch.equal(c0, c1), f"agent {m}: parameters did not change"
        assert bool(torch.isfinite(p.flat_params).all())
    n = len(calls)
    # unset or "0": stepwise
    for flag in (None, "0"):
        monkeypatch.delenv(FLAG, raising=False) if flag is None else monkeypatch.setenv(FLAG, flag)
        r = _runner(_env(N, T), T, N)
        assert not r._episode_ready(), flag
        r.warmup()
        r.rollout()
        assert len(calls) == n, flag
    # layer_N = 2 or a recurrent policy never reach the launch, whatever the flag: the leader's MultiDiscrete actor refuses both at
    # construction (the multi-head kernels' limits), and a runner whose policies were swapped for such ones is not ready either
    monkeypatch.setenv(FLAG, "1")
    for kw in (dict(layer_N=2), dict(use_recurrent_policy=True)):
        with pytest.raises(NotImplementedError, match="MultiDiscrete"):
            _runner(_env(N, T), T, N, **kw)
    r = _runner(_env(N, T), T, N)
    assert r._episode_ready()
    for field, value in (("layer_N", 2), ("recurrent", 1)):
        d = r.policy[3].critic.desc
        old = getattr(d, field)
        setattr(d, field, value)
        assert not r._episode_ready(), field
        setattr(d, field, old)
    assert r._episode_ready() and len(calls) == n


def test_bad_arguments_are_refused_by_name(gpu_device):
    from mappo_amd import _lib, ops
    N, T = 4, 2
    env = _env(N)
    r = _runner(env, T, N)
    lib = _lib.load()

    def agents():
        return [ops.comm_agent(p.actor.flat, p.actor.desc, p.critic.flat, p.critic.desc, p.actor._seed, None, b.obs, b.share_obs, b.rewards,
                               b.masks, b.actions, b.action_log_probs, b.value_preds, torch.empty(N, device="cuda"))
                for p, b in zip(r.policy, r.buffer)]

    def call(ags, T_=T):
        before = {k: v.clone() for k, v in env.state_tensors().items()}
        arr = (_lib.CommAgent * 6)(*ags)
        st = [C.c_void_p(env.state_tensors()[k].data_ptr()) for k in WR.STATE]
        rc = lib.mappo_rollout_episode_world_comm(arr, *st, T_, N, 25, 1, 0, 0, 1, None)
        torch.cuda.synchronize()
        for k, v in env.state_tensors().items():
            assert torch.equal(v, before[k]), "a refused call launched"
        return rc, lib.mappo_last_error().decode()
    a = agents()
    a[4], a[3] = a[3], a[4]                                         # a 28-wide actor where a 34-wide one belongs
    rc, msg = call(a)
    assert rc == -1 and "adversary 3" in msg and "in_dim 28" in msg, msg
    a = agents()
    d = type(a[2].actor_desc)()
    C.memmove(C.byref(d), C.byref(a[2].actor_desc), C.sizeof(d))
    d.recurrent = 1
    a[2].actor_desc = d
    rc, msg = call(a)
    assert rc == -1 and "adversary 2" in msg and "recurrent" in msg, msg
    rc, msg = call(agents(), 0)
    assert rc == -1 and "T=0" in msg, msg
    a = agents()
    a[5].rew_buf = None
    rc, msg = call(a)
    assert rc == -1 and "null pointer" in msg and "good agent 5" in msg, msg
