"""The one-launch rollout episode on MPE simple_tag (mappo_rollout_episode_tag, csrc/rollout_tag.h): bit for bit against the stepwise
path from states with a contact and a speed clamp in the first steps, guard floats around every output, sampling and values against
float64 oracle networks, the NumPy mirror and the host Philox on both paths, and the separated runner training four agents either
way."""
import numpy as np
import pytest
import torch

from conftest import golden
import mpe_tag_np as MT
import rollout_ref as R
import tag_rollout_ref as TR

pytestmark = pytest.mark.gpu

NAMES = ("share_obs", "obs", "value_preds", "returns", "actions", "action_log_probs", "rewards", "masks", "bad_masks", "active_masks")
TOL = dict(rtol=1e-6, atol=1e-6)          # env outputs against the mirror: tests/test_gpu_mpe_tag.py


def _np(t):
    return t.detach().cpu().numpy()


def _env(N, T=25, seed=3):
    from mappo_amd.envs import SimpleTagVecEnv
    return SimpleTagVecEnv(N, episode_length=T, seed=seed)


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
    a = _args(episode_length=T, n_rollout_threads=N, env_name="MPE", share_policy=False, use_hip_graph=False, seed=TR.SEED,
              algorithm_name="mappo", ppo_epoch=2, num_mini_batch=1, **kw)
    torch.manual_seed(1)
    return MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=4, device=torch.device("cuda"), run_dir=None))


def _contact_state(N):
    """Fixture start states tiled to N, then: adversary 0 inside the good agent's contact distance, adversary 1 at speed 3 (0.75 x 3 - 0.9 > 1: clamped
    at the first step whatever it does), a landmark inside adversary 2's contact distance."""
    g = golden("mpe_tag")
    k = np.arange(N) % 12
    pos, vel, lpos = g["long/pos0"][k].copy(), g["long/vel0"][k].copy(), g["long/lpos"][k].copy()
    pos[:, 0] = pos[:, 3] + np.array([0.1, 0.0])
    vel[:, 1] = np.array([3.0, 0.0])
    lpos[:, 0] = pos[:, 2] + np.array([0.2, 0.05])
    return pos, vel, lpos


def _load_state(r, env, state, cen):
    """Explicit state into the env and its observations into slot 0 of the buffers (what warmup() did for the reset state)."""
    env.set_state(*state)
    o = MT.observation(state[0], state[1], state[2])
    share = np.concatenate(o, axis=1).astype(np.float32)
    for m in range(4):
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
    real = ops.rollout_episode_tag
    monkeypatch.setattr(ops, "rollout_episode_tag", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    runs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("MAPPO_TAG_EPISODE", flag)
        env = _env(N, env_T)
        r = _runner(env, T, N, layer_N=layer_N, use_ReLU=relu, use_centralized_V=cen)
        assert r._ragged and r._fused_ff() and r._tag_episode_ready() == (flag == "1")
        r.warmup()
        _load_state(r, env, _contact_state(N), cen)
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
    assert tuple(s["agent0/obs"].shape) == (T + 1, N, 16) and tuple(s["agent3/obs"].shape) == (T + 1, N, 14)
    assert tuple(s["agent3/share_obs"].shape) == (T + 1, N, 62 if cen else 14)
    # the new physics ran inside the launch: the contact pays at step 0 or pushed the pair apart, and adversary 1 was clamped to speed 1
    v1 = s["agent1/obs"][1, :, 0:2].double()
    if env_T > 1:
        assert float((v1.norm(dim=1) - 1.0).abs().max()) < 1e-6
    if env_T < T:
        assert int(s["env/episode"].min()) >= T // env_T and float(s["agent0/masks"][1:].min()) == 0.0


def test_one_launch_writes_nothing_outside_the_buffers(gpu_device):
    from mappo_amd import ops
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
        D = MT.OBS_DIMS[m]
        v = dict(obs=guarded(T + 1, N, D), share=guarded(T + 1, N, 62), rew=guarded(T, N, 1), mask=guarded(T + 1, N, 1),
                 act=guarded(T, N, 1), logp=guarded(T, N, 1), val=guarded(T + 1, N, 1), nv=guarded(N))
        v["obs"][0].copy_(obs[m]); v["share"][0].copy_(torch.cat(obs, dim=1)); v["mask"][0].fill_(1.0)
        views.append(v)
        ags.append(ops.comm_agent(p.actor.flat, p.actor.desc, p.critic.flat, p.critic.desc, p.actor._seed, None, v["obs"], v["share"], v["rew"],
                                  v["mask"], v["act"], v["logp"], v["val"], v["nv"]))
    st = env.episode_state_tag()
    ops.rollout_episode_tag(ags, T, N, st["T"], st["seed"], st["agent_pos"], st["agent_vel"], st["landmark_pos"], st["tstep"], st["episode"],
                            False, 0, cen)
    torch.cuda.synchronize()
    for full, n in fulls:
        assert bool(torch.isnan(full[:G]).all()) and bool(torch.isnan(full[G + n:]).all())
    for v in views:
        for k in ("obs", "share", "rew", "mask", "act", "logp", "nv"):
            assert bool(torch.isfinite(v[k]).all()), k
        assert bool(torch.isfinite(v["val"][:T]).all()) and bool(torch.isnan(v["val"][T]).all())     # slot T belongs to nobody here


@pytest.mark.parametrize("flag", ["0", "1"], ids=["stepwise", "one-launch"])
def test_rollout_against_float64_and_host_philox(gpu_device, monkeypatch, flag):
    monkeypatch.setenv("MAPPO_TAG_EPISODE", flag)
    N, T = TR.N, TR.T
    env = _env(N, TR.ENV_T)
    r = _runner(env, T, N)
    tw = TR.twins()
    for m in range(4):
        r.policy[m].actor.load_state_dict(tw[m].actor.state_dict())
        r.policy[m].critic.load_state_dict(tw[m].critic.state_dict())
        assert r.policy[m].actor._seed == TR.agent_seed(m)
    r.warmup()
    _load_state(r, env, TR.initial_state(), True)
    mirror = MT.SimpleTagNp(*TR.initial_state(), episode_length=TR.ENV_T)
    r.rollout()
    fails, near, pairs = [], 0, 0
    for t in range(T):
        acts = []
        for m in range(4):
            b = r.buffer[m]
            e, tol = TR.expected_step(tw[m].actor, _np(b.obs[t]), m, t)
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
        for m in range(4):
            b = r.buffer[m]
            np.testing.assert_allclose(_np(b.obs[t + 1]), obs[m].astype(np.float32), err_msg=f"obs, step {t}, agent {m}", **TOL)
            np.testing.assert_allclose(_np(b.share_obs[t + 1]), share, err_msg=f"share_obs, step {t}, agent {m}", **TOL)
            np.testing.assert_allclose(_np(b.rewards[t, :, 0]), rew[:, m].astype(np.float32), err_msg=f"rewards, step {t}, agent {m}", **TOL)
            np.testing.assert_array_equal(_np(b.masks[t + 1, :, 0]), 1.0 - dones[:, m].astype(np.float32))
    assert near <= TR.NEAR_CAP * pairs, f"{near} of {pairs} (row, agent) pairs left out"
    assert not fails, "\n".join(fails)


def test_runner_trains_four_agents_either_way(gpu_device, monkeypatch):
    """N = 16, T = 5, two iterations with MAPPO_TAG_EPISODE 0 and 1: the first rollout's buffers are identical, every value stays
    finite and all four policies change."""
    N, T = 16, 5
    first = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("MAPPO_TAG_EPISODE", flag)
        env = _env(N, T)
        r = _runner(env, T, N)
        assert r._tag_episode_ready() == (flag == "1")
        r.warmup()
        before = [p.flat_params.clone() for p in r.policy]
        for it in range(2):
            r.rollout()
            if it == 0:
                first[flag] = _snapshot(r)
            infos = r.train()
            assert len(infos) == 4
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
