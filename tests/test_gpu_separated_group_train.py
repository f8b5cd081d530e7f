"""MAPPO_SEPARATED_GROUP_TRAIN=1: the separated runner's grouped train() (runner/separated/base_runner.py) against its sequential one.

simple_adversary (3 agents) and simple_tag (4 agents), N = 4, T = 5, ppo_epoch = 2: two iterations of rollout(); train() from the
same seed with the flag and without — every agent's flat_params, Adam moments, step counters, ValueNorm state, train_infos and the
buffers' slot 0 equal to the bit after each iteration.  The second iteration of a run with hipGraphs IS the captured graph's
replay, and it is also held against the all-eager grouped run.  Runs whose agents do not qualify (simple_world_comm: 192-wide
critics and a MultiDiscrete leader; rmappo; num_mini_batch = 2) train sequentially with the flag on — the grouped op is never
called, one warning says so, and the results are those of the run without the flag."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLAG = "MAPPO_SEPARATED_GROUP_TRAIN"
N, T = 4, 5


def _args(**kw):
    from mappo_amd.config import get_config
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = False
    a.use_naive_recurrent_policy = False
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def _env(name, n=N, t=T):
    from mappo_amd import envs
    return getattr(envs, name)(n, episode_length=t, seed=3)


def _runner(env, n=N, t=T, **kw):
    from mappo_amd.runner.separated.mpe_runner import MPERunner
    kw = dict(dict(use_hip_graph=True, algorithm_name="mappo", num_mini_batch=1), **kw)
    a = _args(episode_length=t, n_rollout_threads=n, env_name="MPE", share_policy=False, seed=1, ppo_epoch=2,
              use_recurrent_policy=(kw["algorithm_name"] == "rmappo"), **kw)
    torch.manual_seed(1)
    return MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=env.M if hasattr(env, "M") else len(env.action_space),
                          device=torch.device("cuda"), run_dir=None))


def _count(monkeypatch):
    from mappo_amd import ops
    calls = []
    real_u, real_o = ops.actor_critic_update_group, ops.reduce_clip_adam_group
    monkeypatch.setattr(ops, "actor_critic_update_group", lambda jobs: (calls.append(("update", len(jobs))), real_u(jobs))[1])
    monkeypatch.setattr(ops, "reduce_clip_adam_group", lambda jobs: (calls.append(("optim", len(jobs))), real_o(jobs))[1])
    return calls


def _state(r, infos):
    out = {}
    for m, (p, tr, b) in enumerate(zip(r.policy, r.trainer, r.buffer)):
        out[f"agent{m}/flat_params"] = p.flat_params.clone()
        out[f"agent{m}/exp_avg"] = p.exp_avg.clone()
        out[f"agent{m}/exp_avg_sq"] = p.exp_avg_sq.clone()
        out[f"agent{m}/opt_step"] = p.opt_step.clone()
        out[f"agent{m}/grad_norms"] = p.grad_norms.clone()
        if tr.value_normalizer is not None:
            out[f"agent{m}/valuenorm"] = tr.value_normalizer.state.clone()
        for n in ("obs", "share_obs", "masks", "active_masks"):
            out[f"agent{m}/{n}[0]"] = getattr(b, n)[0].clone()
        assert sorted(infos[m]) == sorted(["value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm", "ratio"])
        out[f"agent{m}/train_info"] = torch.tensor([infos[m][k] for k in sorted(infos[m])], dtype=torch.float64)
    return out


def _run(monkeypatch, env_name, flag, iters=2, n=N, t=T, **kw):
    """`iters` iterations of rollout(); train() from the seed; the state after each."""
    if flag is None:
        monkeypatch.delenv(FLAG, raising=False)
    else:
        monkeypatch.setenv(FLAG, flag)
    r = _runner(_env(env_name, n, t), n, t, **kw)
    r.warmup()
    states = []
    for _ in range(iters):
        r.rollout()
        infos = r.train()
        assert len(infos) == len(r.trainer)
        states.append(_state(r, infos))
    torch.cuda.synchronize()
    return r, states


def _assert_equal(a, b, what):
    assert len(a) == len(b)
    for it, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), f"{what}, iteration {it}: {k} differs ({(x[k] != y[k]).sum().item()} of {x[k].numel()} elements)"


@pytest.mark.parametrize("env_name,M", [("SimpleAdversaryVecEnv", 3), ("SimpleTagVecEnv", 4)])
def test_grouped_train_equals_sequential(gpu_device, monkeypatch, env_name, M):
    calls = _count(monkeypatch)
    r0, seq = _run(monkeypatch, env_name, None)
    assert not calls and len(r0.trainer) == M and not r0._group_train_ready()
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                # a qualifying run says nothing
        r1, grp = _run(monkeypatch, env_name, "1")
    assert r1._group_train_ready() and all(tr.phase_ready() for tr in r1.trainer)
    # eager pass + capture: ppo_epoch (update, optim) pairs each, all M agents in each call; the replay calls nothing
    assert calls == [("update", M), ("optim", M)] * 4, calls
    assert isinstance(next(iter(r1._group_graphs.values())), torch.cuda.CUDAGraph)
    _assert_equal(grp, seq, f"{env_name}: grouped (graph) vs sequential")
    for st in grp:                                                    # it trained: finite, and the parameters moved
        for k, v in st.items():
            assert bool(torch.isfinite(v.double()).all()), k
    assert not torch.equal(grp[0]["agent0/flat_params"], grp[1]["agent0/flat_params"])
    assert grp[1]["agent0/opt_step"].tolist() == [4, 4]
    del calls[:]
    r2, eager = _run(monkeypatch, env_name, "1", use_hip_graph=False)
    assert calls == [("update", M), ("optim", M)] * 4 and r2._group_graphs is None
    _assert_equal(eager, grp, f"{env_name}: grouped eager vs grouped graph replay")
    # "0" is unset
    del calls[:]
    r3, off = _run(monkeypatch, env_name, "0", iters=1)
    assert not calls
    _assert_equal(off, seq[:1], f"{env_name}: flag 0 vs unset")


def test_more_agents_than_a_group_holds_split_into_groups(gpu_device, monkeypatch):
    """No env here has more than 8 agents (the launch's limit), so the limit comes down instead: simple_tag's 4 agents in groups of
    at most 3 — (3, 1) per epoch — and decentralised critics, against the sequential run."""
    from mappo_amd.runner.separated.base_runner import Runner
    calls = _count(monkeypatch)
    _, seq = _run(monkeypatch, "SimpleTagVecEnv", None, use_centralized_V=False)
    monkeypatch.setattr(Runner, "GROUP_MAX", 3)
    _, grp = _run(monkeypatch, "SimpleTagVecEnv", "1", use_centralized_V=False)
    assert calls == [("update", 3), ("optim", 3), ("update", 1), ("optim", 1)] * 4, calls
    _assert_equal(grp, seq, "groups of (3, 1): grouped vs sequential")


FALLBACKS = [("SimpleWorldCommVecEnv", dict(), N, T), ("SimpleSpeakerListenerVecEnv", dict(algorithm_name="rmappo", data_chunk_length=3), 8, 6),
             ("SimpleAdversaryVecEnv", dict(num_mini_batch=2), N, T)]


@pytest.mark.parametrize("env_name,kw,n,t", FALLBACKS, ids=["world_comm", "rmappo", "num_mini_batch2"])
def test_runs_that_do_not_qualify_train_sequentially(gpu_device, monkeypatch, env_name, kw, n, t):
    calls = _count(monkeypatch)
    _, seq = _run(monkeypatch, env_name, None, n=n, t=t, **kw)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r, on = _run(monkeypatch, env_name, "1", n=n, t=t, **kw)
    said = [x for x in w if FLAG in str(x.message)]
    assert len(said) == 1 and "sequentially" in str(said[0].message), [str(x.message) for x in w]      # once, not once per train()
    assert not calls and not r._group_train_ready() and r._group_graphs is None
    _assert_equal(on, seq, f"{env_name}: flag on (fallback) vs unset")
    for k, v in on[-1].items():
        assert bool(torch.isfinite(v.double()).all()), k
