"""The one-launch rollout episode on MPE simple_push (mappo_rollout_episode_push, csrc/rollout_push.h): bit for bit against the
stepwise path from states with the two agents in contact, guard floats around every output, sampling and values against float64
oracle networks, the NumPy mirror and the host Philox on both paths, and the separated runner training two agents either way."""
import numpy as np
import pytest
import torch

from conftest import golden
import mpe_push_np as MP
import rollout_ref as R
import push_rollout_ref as PR

pytestmark = pytest.mark.gpu

NAMES = ("share_obs", "obs", "value_preds", "returns", "actions", "action_log_probs", "rewards", "masks", "bad_masks", "active_masks")
TOL = dict(rtol=1e-6, atol=1e-6)          # env outputs against the mirror: tests/test_gpu_mpe_push.py


def _np(t):
    return t.detach().cpu().numpy()


def _env(N, T=25, seed=3):
    from mappo_amd.envs import SimplePushVecEnv
    return SimplePushVecEnv(N, episode_length=T, seed=seed)


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
    a = _args(episode_length=T, n_rollout_threads=N, env_name="MPE", share_policy=False, use_hip_graph=False, seed=PR.SEED,
              algorithm_name="mappo", ppo_epoch=2, num_mini_batch=1, **kw)
    torch.manual_seed(1)
    return MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=2, device=torch.device("cuda"), run_dir=None))


def _contact_state(N):
    """Fixture start states tiled to N, then: the adversary inside the good agent's contact distance (0.06 < 0.1, another direction
    per environment), the good agent moving."""
    g = golden("mpe_push")
    k = np.arange(N) % 12
    pos, vel, lpos, goal = g["long/pos0"][k].copy(), g["long/vel0"][k].copy(), g["long/lpos"][k].copy(), g["long/goal"][k].copy()
    ang = 0.7 * np.arange(N)
    pos[:, 0] = pos[:, 1] + 0.06 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    vel[:, 1] = np.array([0.2, -0.1])
    return pos, vel, lpos, goal


def _load_state(r, env, state, cen):
    """Explicit state into the env and its observations into slot 0 of the buffers (what warmup() did for the reset state)."""
    env.set_state(*state)
    o = MP.observation(state[0], state[1], state[2], np.asarray(state[3], np.int64))
    share = np.concatenate(o, axis=1).astype(np.float32)
    for m in range(2):
        r.buffer[m].obs[0].copy_(torch.from_numpy(o[m].astype(np.float32)))
        r.buffer[m].share_obs[0].copy_(torch.from_numpy(share if cen else o[m].astype(np.float32)))


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


# N: one row | a full tile | a full tile + one row | two tiles + a partial one; (T, env T): no reset | two resets inside the rollout;
# every value of layer_N, activation and critic input at least once
CASES = [(1, (3, 25), 1, True, True), (16, (5, 2), 0, False, False), (17, (3, 25), 1, False, True), (37, (5, 2), 1, True, False),
         (37, (3, 25), 0, True, True), (17, (5, 2), 1, False, False), (16, (3, 25), 0, False, True), (1, (5, 2), 0, True, False)]


@pytest.mark.parametrize("N,TT,layer_N,relu,cen", CASES, ids=[f"N{c[0]}-T{c[1][0]}-envT{c[1][1]}-L{c[2]}-{'relu' if c[3] else 'tanh'}-"
                                                              f"{'cen' if c[4] else 'dec'}" for c in CASES])
def test_one_launch_equals_stepwise(gpu_device, monkeypatch, N, TT, layer_N, relu, cen):
    from mappo_amd import ops
    T, env_T = TT
    calls = []
    real = ops.rollout_episode_push
    monkeypatch.setattr(ops, "rollout_episode_push", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    runs = {}
    state = _contact_state(N)
    assert MP.in_contact(state[0]).all()
    for flag in ("1", "0"):
        monkeypatch.setenv("MAPPO_PUSH_EPISODE", flag)
        env = _env(N, env_T)
        r = _runner(env, T, N, layer_N=layer_N, use_ReLU=relu, use_centralized_V=cen)
        assert r._ragged and r._fused_ff() and r._episode_ready() == (flag == "1")
        r.warmup()
        _load_state(r, env, state, cen)
        snaps = []
        for it in range(2):                                        # the second episode continues from the first one's state
            n0 = len(calls)
            r.rollout()
            assert len(calls) - n0 == (1 if flag == "1" else 0)
            snaps.append(_snapshot(r))
            for b in r.buffer:
                b.after_update()
        runs[flag] = snaps
    for it in range(2):
        _assert_equal(runs["1"][it], runs["0"][it], f"episode {it}, one launch vs stepwise")
    s = runs["1"][0]
    assert all(bool(torch.isfinite(v).all()) for v in s.values() if v.is_floating_point())
    assert tuple(s["agent0/obs"].shape) == (T + 1, N, 8) and tuple(s["agent1/obs"].shape) == (T + 1, N, 19)
    assert tuple(s["agent1/share_obs"].shape) == (T + 1, N, 27 if cen else 19) and tuple(s["agent0/share_obs"].shape) == (T + 1, N, 27 if cen else 8)
    # the contact force ran inside the launch: from rest an action alone leaves the adversary with one of five velocities; the contact
    # at 0.06 of 0.1 adds 100 x 0.04 x 0.1 = 0.4 along the line between the two, which puts it at least 0.1 away from all five
    if env_T > 1:
        v0 = s["agent0/obs"][1, :, 0:2].double().cpu()
        free = torch.tensor([[0.0, 0.0], [0.5, 0.0], [-0.5, 0.0], [0.0, 0.5], [0.0, -0.5]], dtype=torch.float64)
        assert float((v0[:, None] - free[None]).norm(dim=2).min()) > 0.05
    if env_T < T:
        assert int(s["env/episode"].min()) >= T // env_T and float(s["agent0/masks"][1:].min()) == 0.0


@pytest.mark.parametrize("N", [1, 17])
def test_one_launch_writes_nothing_outside_the_buffers(gpu_device, N):
    from mappo_amd import ops
    T, G, cen = 3, 64, True
    env = _env(N, 2)
    r = _runner(env, T, N, layer_N=1, use_centralized_V=cen)
    obs = env.reset()
    fulls = []

    def guarded(*shape, dtype=torch.float32, fill=float("nan")):
        n = int(np.prod(shape))
        full = torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")
        fulls.append((full, n, fill))
        return full[G:G + n].view(*shape)
    ags, views = [], []
    for m, p in enumerate(r.policy):
        D = MP.OBS_DIMS[m]
        v = dict(obs=guarded(T + 1, N, D), share=guarded(T + 1, N, 27), rew=guarded(T, N, 1), mask=guarded(T + 1, N, 1),
                 act=guarded(T, N, 1), logp=guarded(T, N, 1), val=guarded(T + 1, N, 1), nv=guarded(N))
        v["obs"][0].copy_(obs[m]); v["share"][0].copy_(torch.cat(obs, dim=1)); v["mask"][0].fill_(1.0)
        views.append(v)
        ags.append(ops.comm_agent(p.actor.flat, p.actor.desc, p.critic.flat, p.critic.desc, p.actor._seed, None, v["obs"], v["share"], v["rew"],
                                  v["mask"], v["act"], v["logp"], v["val"], v["nv"]))
    # the env state, guarded too: the launch stores it back
    st = {}
    for k, t in env.state_tensors().items():
        fill = float("nan") if t.is_floating_point() else -77
        st[k] = guarded(*t.shape, dtype=t.dtype, fill=fill)
        st[k].copy_(t)
    ops.rollout_episode_push(ags, T, N, env.T, env.seed, st["agent_pos"], st["agent_vel"], st["landmark_pos"], st["goal"], st["tstep"],
                             st["episode"], False, 0, cen)
    torch.cuda.synchronize()
    for full, n, fill in fulls:
        for side in (full[:G], full[G + n:]):
            assert bool(torch.isnan(side).all()) if fill != fill else bool((side == fill).all())
    for v in views:
        for k in ("obs", "share", "rew", "mask", "act", "logp", "nv"):
            assert bool(torch.isfinite(v[k]).all()), k
        assert bool(torch.isfinite(v["val"][:T]).all()) and bool(torch.isnan(v["val"][T]).all())     # slot T belongs to nobody here
    assert bool(torch.isfinite(st["agent_pos"]).all()) and _np(st["episode"]).tolist() == [2] * N    # reset + one reset-on-done (T = 3, env T = 2)
    assert _np(st["tstep"]).tolist() == [1] * N


@pytest.mark.parametrize("flag", ["0", "1"], ids=["stepwise", "one-launch"])
def test_rollout_against_float64_and_host_philox(gpu_device, monkeypatch, flag):
    monkeypatch.setenv("MAPPO_PUSH_EPISODE", flag)
    N, T = PR.N, PR.T
    env = _env(N, PR.ENV_T)
    r = _runner(env, T, N)
    tw = PR.twins()
    for m in range(2):
        r.policy[m].actor.load_state_dict(tw[m].actor.state_dict())
        r.policy[m].critic.load_state_dict(tw[m].critic.state_dict())
        assert r.policy[m].actor._seed == PR.agent_seed(m)
    r.warmup()
    _load_state(r, env, PR.initial_state(), True)
    mirror = MP.SimplePushNp(*PR.initial_state(), episode_length=PR.ENV_T)
    assert MP.in_contact(mirror.pos).sum() == 3
    r.rollout()
    fails, near, pairs = [], 0, 0
    for t in range(T):
        acts = []
        for m in range(2):
            b = r.buffer[m]
            e, tol = PR.expected_step(tw[m].actor, _np(b.obs[t]), m, t)
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
        for m in range(2):
            b = r.buffer[m]
            np.testing.assert_allclose(_np(b.obs[t + 1]), obs[m].astype(np.float32), err_msg=f"obs, step {t}, agent {m}", **TOL)
            np.testing.assert_allclose(_np(b.share_obs[t + 1]), share, err_msg=f"share_obs, step {t}, agent {m}", **TOL)
            np.testing.assert_allclose(_np(b.rewards[t, :, 0]), rew[:, m].astype(np.float32), err_msg=f"rewards, step {t}, agent {m}", **TOL)
            np.testing.assert_array_equal(_np(b.masks[t + 1, :, 0]), 1.0 - dones[:, m].astype(np.float32))
    assert near <= PR.NEAR_CAP * pairs, f"{near} of {pairs} (row, agent) pairs left out"
    assert not fails, "\n".join(fails)


def test_runner_trains_both_agents_either_way(gpu_device, monkeypatch):
    """N = 16, T = 5, two iterations with MAPPO_PUSH_EPISODE 0 and 1: the first rollout's buffers are identical, every value stays
    finite and both policies change."""
    N, T = 16, 5
    first = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("MAPPO_PUSH_EPISODE", flag)
        env = _env(N, T)
        r = _runner(env, T, N)
        assert r._episode_ready() == (flag == "1")
        r.warmup()
        before = [p.flat_params.clone() for p in r.policy]
        for it in range(2):
            r.rollout()
            if it == 0:
                first[flag] = _snapshot(r)
            infos = r.train()
            assert len(infos) == 2
            for m, info in enumerate(infos):
                for k, v in info.items():
                    assert np.isfinite(float(v)), (flag, it, m, k, v)
        for m, p in enumerate(r.policy):
            a0, a1 = before[m][:p.actor.n_params], p.flat_params[:p.actor.n_params]
            lo = p.seg_bounds[1]
            c0, c1 = before[m][lo:lo + p.critic.n_params], p.flat_params[lo:lo + p.critic.n_params]
            assert not torch.equal(a0, a1) and not torch.equal(c0, c1), f"agent {m}: parameters did not change"
            assert bool(torch.isfinite(p.flat_params).all())
    _assert_equal(first["0"], first["1"], "first rollout, stepwise vs one launch")
