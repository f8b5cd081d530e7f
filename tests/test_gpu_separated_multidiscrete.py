"""One MultiDiscrete agent among Discrete ones under the separated runner (share_policy = False), on the GPU-resident
simple_world_comm env: construction (refused before this env declared `accepts_multidiscrete_agents`), K-wide action columns in
the leader's buffer, the leader's update equal to the shared path's with num_agents = 1, two training iterations with a centralized
(192-wide) and a decentralized critic, the leader's word arriving in the adversaries' next observations, eval, and the old refusal
for an env without the flag."""
import numpy as np
import pytest
import torch

import mpe_world_comm_np as MW

pytestmark = pytest.mark.gpu

N, T = 16, 5
NAMES = ("share_obs", "obs", "value_preds", "returns", "actions", "action_log_probs", "rewards", "masks")


def _args(**kw):
    from mappo_amd.config import get_config
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = False
    a.use_naive_recurrent_policy = False
    base = dict(episode_length=T, n_rollout_threads=N, env_name="MPE", share_policy=False, use_hip_graph=False, seed=1, algorithm_name="mappo",
                ppo_epoch=2, num_mini_batch=1, layer_N=1)
    base.update(kw)
    for k, v in base.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def _env(seed=3):
    from mappo_amd.envs import SimpleWorldCommVecEnv
    return SimpleWorldCommVecEnv(N, episode_length=T, seed=seed)


def _runner(centralized=True, eval_env=None, **kw):
    from mappo_amd.runner.separated.mpe_runner import MPERunner
    torch.manual_seed(1)
    a = _args(use_centralized_V=centralized, **kw)
    return MPERunner(dict(all_args=a, envs=_env(), eval_envs=eval_env, num_agents=6, device=torch.device("cuda"), run_dir=None))


def test_runner_constructs_with_k_wide_leader_buffers(gpu_device):
    r = _runner()
    assert r._multi and r._ragged and not r._fused_ff() and not r._episode_ready()
    assert [p.actor.desc.in_dim for p in r.policy] == [34] * 4 + [28] * 2 and [p.critic.desc.in_dim for p in r.policy] == [192] * 6
    assert tuple(r.policy[0].actor.head_dims) == (5, 4) and all(p.actor.head_dims is None for p in r.policy[1:])
    assert [p.actor.desc.out_dim for p in r.policy] == [9] + [5] * 5
    assert tuple(r.buffer[0].actions.shape) == (T, N, 2) and tuple(r.buffer[0].action_log_probs.shape) == (T, N, 2)
    for b in r.buffer[1:]:
        assert tuple(b.actions.shape) == (T, N, 1) and tuple(b.action_log_probs.shape) == (T, N, 1)
    assert tuple(r.buffer[0].obs.shape) == (T + 1, N, 34) and tuple(r.buffer[5].obs.shape) == (T + 1, N, 28)
    assert tuple(r.buffer[0].share_obs.shape) == (T + 1, N, 192)
    r2 = _runner(centralized=False)
    assert [p.critic.desc.in_dim for p in r2.policy] == [34] * 4 + [28] * 2


def test_env_without_the_flag_is_still_refused(gpu_device):
    """The refusal of tests/test_gpu_multidiscrete.py, word for word, for an env that does not declare the capability — and for this
    env with the declaration taken away."""
    from mappo_amd.envs.synthetic import SyntheticMPEEnv
    from mappo_amd.runner.separated.mpe_runner import MPERunner
    d = torch.device("cuda:0")
    a = _args(n_rollout_threads=4)
    env = SyntheticMPEEnv(4, 2, 21, episode_length=T, seed=1, device=d, action_dims=(5, 10))
    assert not getattr(env, "accepts_multidiscrete_agents", False)
    msg = (r"MultiDiscrete action space under the separated runner \(share_policy = False\): the K-wide action columns are built for the "
           r"shared MPERunner only")
    with pytest.raises(NotImplementedError, match=msg):
        MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=2, device=d, run_dir=None))
    env = _env()
    env.accepts_multidiscrete_agents = False
    with pytest.raises(NotImplementedError, match="MultiDiscrete.*separated"):
        MPERunner(dict(all_args=_args(), envs=env, eval_envs=None, num_agents=6, device=d, run_dir=None))


def test_rmappo_stays_refused_for_the_leader(gpu_device):
    from mappo_amd.runner.separated.mpe_runner import MPERunner
    a = _args(algorithm_name="rmappo")
    a.use_recurrent_policy = True
    with pytest.raises(NotImplementedError, match="MultiDiscrete action space with a recurrent policy"):
        MPERunner(dict(all_args=a, envs=_env(), eval_envs=None, num_agents=6, device=torch.device("cuda"), run_dir=None))


@pytest.mark.parametrize("share_dim", [192, 34], ids=["centralized", "decentralized"])
def test_leader_update_equals_the_shared_path_with_one_agent(gpu_device, share_dim):
    """A MultiDiscrete agent's SeparatedReplayBuffer and trainer against a SharedReplayBuffer with num_agents = 1 and a policy with the
    same parameters, filled with the same data: the same kernels run on the same rows, so flat_params are equal to the bit after
    one train()."""
    from mappo_amd.algorithms.r_mappo.r_mappo import R_MAPPO
    from mappo_amd.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    from mappo_amd.utils.separated_buffer import SeparatedReplayBuffer
    from mappo_amd.utils.shared_buffer import SharedReplayBuffer
    from mappo_amd.utils.util import MultiDiscrete
    d = torch.device("cuda")
    a = _args()
    space = MultiDiscrete([[0, 4], [0, 3]])
    torch.manual_seed(7)
    pol_s = R_MAPPOPolicy(a, [34], [share_dim], space, device=d)
    pol_j = R_MAPPOPolicy(a, [34], [share_dim], space, device=d)
    pol_j.flat_params.copy_(pol_s.flat_params)
    sep = SeparatedReplayBuffer(a, [34], [share_dim], space, device=d)
    joint = SharedReplayBuffer(a, 1, [34], [share_dim], space, device=d)
    assert tuple(sep.actions.shape) == (T, N, 2) and tuple(joint.actions.shape) == (T, N, 1, 2)
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g)
    data = dict(obs=rnd(T + 1, N, 34), share_obs=rnd(T + 1, N, share_dim), value_preds=rnd(T + 1, N, 1), returns=rnd(T + 1, N, 1),
                rewards=rnd(T, N, 1), action_log_probs=-rnd(T, N, 2).abs() - 0.5,
                actions=torch.stack([torch.randint(0, 5, (T, N), generator=g), torch.randint(0, 4, (T, N), generator=g)], dim=-1).float())
    for k, v in data.items():
        getattr(sep, k).copy_(v.cuda())
        getattr(joint, k).copy_(v.cuda().unsqueeze(2))
    tr_s, tr_j = R_MAPPO(a, pol_s, device=d), R_MAPPO(a, pol_j, device=d)
    before = pol_s.flat_params.clone()
    infos = []
    for tr, buf in ((tr_s, sep), (tr_j, joint)):
        torch.manual_seed(11)
        tr.prep_training()
        infos.append(tr.train(buf))
    torch.cuda.synchronize()
    assert not torch.equal(pol_s.flat_params, before) and bool(torch.isfinite(pol_s.flat_params).all())
    assert torch.equal(pol_s.flat_params, pol_j.flat_params)
    for k in infos[0]:
        assert float(infos[0][k]) == float(infos[1][k]), k


def _iterate(r, iterations=2):
    """-> per iteration, a snapshot of every agent's buffer after the rollout, and the train infos."""
    r.warmup()
    snaps, infos = [], []
    for _ in range(iterations):
        r.rollout()
        snaps.append([{n: getattr(b, n).clone() for n in NAMES} for b in r.buffer])
        infos.append(r.train())
    torch.cuda.synchronize()
    return snaps, infos


@pytest.mark.parametrize("centralized", [True, False], ids=["centralized", "decentralized"])
def test_two_iterations_train_all_six_agents(gpu_device, centralized):
    r = _runner(centralized)
    before = [p.flat_params.clone() for p in r.policy]
    snaps, infos = _iterate(r)
    for it in range(2):
        assert len(infos[it]) == 6
        for m, info in enumerate(infos[it]):
            for k, v in info.items():
                assert np.isfinite(float(v)), (it, m, k, v)
        for m, s in enumerate(snaps[it]):
            for n in NAMES:
                assert bool(torch.isfinite(s[n]).all()), (it, m, n)
        lead = snaps[it][0]["actions"]
        assert tuple(lead.shape) == (T, N, 2)
        assert float(lead[..., 0].min()) >= 0 and float(lead[..., 0].max()) <= 4 and float(lead[..., 1].min()) >= 0 and float(lead[..., 1].max()) <= 3
        assert bool((lead == lead.round()).all())
        for m in range(1, 6):
            a = snaps[it][m]["actions"]
            assert tuple(a.shape) == (T, N, 1) and float(a.min()) >= 0 and float(a.max()) <= 4
        # the leader's word of step t stands in every adversary's observation t + 1 — except where the env was reset (mask 0): zero
        word = torch.eye(4, device="cuda")[lead[..., 1].long()]                               # [T, N, 4]
        alive = snaps[it][0]["masks"][1:]                                                     # [T, N, 1]
        assert float(alive.min()) == 0.0 and float(alive.max()) == 1.0                        # both cases occur
        for m in range(4):
            heard = snaps[it][m]["obs"][1:, :, MW.COMM]
            assert torch.equal(heard, word * alive), (it, m)
            assert float(snaps[it][m]["obs"][0, :, MW.COMM].abs().max()) == (0.0 if it == 0 else float((word * alive)[-1].abs().max()))
        # the share row is the six observations side by side
        if centralized:
            share = torch.cat([snaps[it][m]["obs"] for m in range(6)], dim=-1)
            for m in range(6):
                assert torch.equal(snaps[it][m]["share_obs"], share), (it, m)
        else:
            for m in range(6):
                assert torch.equal(snaps[it][m]["share_obs"], snaps[it][m]["obs"]), (it, m)
    assert len(torch.unique(snaps[0][0]["actions"][..., 1])) > 1 and len(torch.unique(snaps[0][0]["actions"][..., 0])) > 1
    for m, p in enumerate(r.policy):
        a0, a1 = before[m][:p.actor.n_params], p.flat_params[:p.actor.n_params]
        lo = p.seg_bounds[1]
        c0, c1 = before[m][lo:lo + p.critic.n_params], p.flat_params[lo:lo + p.critic.n_params]
        assert not torch.equal(a0, a1) and not torch.equal(c0, c1), f"agent {m}: parameters did not change"
        assert bool(torch.isfinite(p.flat_params).all())
    # a second run from the same seed gives equal buffers
    again, _ = _iterate(_runner(centralized))
    for it in range(2):
        for m in range(6):
            for n in NAMES:
                assert torch.equal(snaps[it][m][n], again[it][m][n]), (it, m, n)


def test_first_rollout_follows_the_mirror(gpu_device):
    """The stored observations and per-agent rewards of the first rollout against the NumPy mirror stepped on the stored actions."""
    TOL = dict(rtol=1e-6, atol=1e-6)
    r = _runner(True)
    r.warmup()
    env = r.envs
    state0 = {k: v.detach().cpu().numpy().copy() for k, v in env.state_tensors().items()}
    r.rollout()
    mirror = MW.SimpleWorldCommNp(state0["agent_pos"], state0["agent_vel"], state0["landmark_pos"], episode_length=T)
    o = mirror.obs()
    for m in range(6):
        np.testing.assert_array_equal(r.buffer[m].obs[0].cpu().numpy(), o[m].astype(np.float32))
    for t in range(T - 1):                                           # the last step ends the episode: slot T holds the reset state's
        acts = np.concatenate([r.buffer[m].actions[t].cpu().numpy().astype(np.int64) for m in range(6)], axis=1)
        assert acts.shape == (N, 7)
        o, rew, dones = mirror.step(acts)
        assert not dones.any()
        for m in range(6):
            np.testing.assert_allclose(r.buffer[m].obs[t + 1].cpu().numpy(), o[m].astype(np.float32), err_msg=f"obs, step {t}, agent {m}", **TOL)
            np.testing.assert_allclose(r.buffer[m].rewards[t, :, 0].cpu().numpy(), rew[:, m].astype(np.float32),
                                       err_msg=f"rewards, step {t}, agent {m}", **TOL)


def test_eval_runs_on_a_second_env_and_logs_six_rewards(gpu_device, capsys):
    r = _runner(True, eval_env=_env(seed=9))
    r.warmup()
    logged = {}
    r.log_env = lambda infos, steps: logged.update(infos)
    state = {k: v.clone() for k, v in r.envs.state_tensors().items()}
    r.eval(0)
    torch.cuda.synchronize()
    out = capsys.readouterr().out
    assert sorted(logged) == sorted(f"agent{m}/eval_average_episode_rewards" for m in range(6))
    for m in range(6):
        assert f"eval average episode rewards of agent{m}: " in out
        assert np.isfinite(logged[f"agent{m}/eval_average_episode_rewards"][0])
    assert len({round(v[0], 6) for v in logged.values()}) > 1          # per-agent rewards, not one shared number
    for k, v in r.envs.state_tensors().items():                       # the training env was not stepped
        assert torch.equal(v, state[k]), k
    assert int(r.eval_envs.episode.min()) >= 1
