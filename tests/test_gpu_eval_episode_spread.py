"""The one-launch evaluation episode on the GPU-resident simple_spread env (mappo_eval_episode_spread, csrc/eval_spread.h; opt-in in
the runner: MAPPO_SPREAD_EVAL_EPISODE=1).

Against the one-launch ROLLOUT episode (mappo_rollout_episode_spread) on the same weights, start state, seed and counter: the
actions and the env's five state tensors are bit-identical, and the returns are the fp32 sum of the rollout's rew_buf over t, added
on the host in step order.  Against float64 (eval_spread_ref.py): the NumPy env under the float64 actor, envs with an undecided
argmax left out.  Nothing besides returns / actions / the env state is written; the runner takes the launch only behind the flag;
an evaluation does not change the training that follows it."""
import numpy as np
import pytest
import torch

import eval_spread_ref as ER
from oracle import mappo_oracle as O
from test_gpu_episode_spread import ENV_NAMES, _counting
from test_gpu_kernels import _flat_from_module, _randomize, ops   # noqa: F401  (ops: the module-level fixture)

SEED, COUNTER, COUNTER_DEV = 2 ** 33 + 12345, 2 ** 32 + 7, 2 ** 32 + 3
ENV_SEED = 9


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _reset_env(ops, N, M, L):
    """A freshly reset env: ([agent_pos, agent_vel, landmark_pos, tstep, episode], the reset's observation rows)."""
    f64 = dict(dtype=torch.float64, device="cuda")
    st = [torch.zeros(N, M, 2, **f64), torch.zeros(N, M, 2, **f64), torch.zeros(N, L, 2, **f64),
          torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int64, device="cuda")]
    obs0 = _nan(N, M, ER.obs_dim(M, L))
    ops.mpe_spread_reset(*st, obs0, N, M, L, ENV_SEED)
    return st, obs0


SHAPES = [  # (N, M, L, T, env episode length)
    (1, 3, 3, 1, 25),
    (1, 3, 3, 25, 7),
    (17, 3, 3, 25, 7),            # 5 envs per tile: 4 tiles in one workgroup, the last one holds 2 envs
    (5, 7, 7, 9, 25),             # 2 envs per tile (14 of 16 rows), 3 tiles: a wave without a tile
    (40, 2, 2, 25, 7),            # 8 envs per tile, 5 tiles: a second workgroup with one busy wave
]


@pytest.mark.gpu
@pytest.mark.parametrize("layer_N", [0, 1])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "tanh"])
@pytest.mark.parametrize("N,M,L,T,env_T", SHAPES)
def test_eval_episode_matches_rollout_episode(ops, N, M, L, T, env_T, relu, layer_N):
    D = ER.obs_dim(M, L)
    B = N * M
    cen = M * D <= 64
    S = M * D if cen else D
    actor = ER.make_actor(M, L, relu, layer_N, 5)
    torch.manual_seed(6)
    critic = O.CriticRef(O.default_args(use_ReLU=relu, layer_N=layer_N), S)
    _randomize(critic, 7)
    da, dc = ops.net_desc(D, 5, layer_N, relu), ops.net_desc(S, 1, layer_N, relu)
    pa, pc = _flat_from_module(ops, actor, da, "act.action_out.linear")[0], _flat_from_module(ops, critic, dc, "v_out")[0]
    for det, cdev in ((1, None), (0, COUNTER_DEV), (0, None)):
        cd = torch.tensor([cdev], dtype=torch.int64, device="cuda") if cdev is not None else None
        # ---- the rollout episode into a scratch buffer ----
        st_r, obs0 = _reset_env(ops, N, M, L)
        obs_buf, share_buf = _nan(T + 1, B, D), _nan(T + 1, B, S)
        obs_buf[0] = obs0.view(B, D)
        share_buf[0] = obs0.view(N, 1, S).expand(N, M, S).reshape(B, S) if cen else obs0.view(B, D)
        rew_buf, mask_buf, act_r, logp, values, nxt = _nan(T, B), _nan(T + 1, B), _nan(T, B), _nan(T, B), _nan(T, B), _nan(B)
        ops.rollout_episode_spread(pa, da, pc, dc, T, N, M, L, env_T, ENV_SEED, *st_r, det, SEED, COUNTER, cd, obs_buf, share_buf, rew_buf,
                                   mask_buf, act_r, logp, values, nxt, cen)
        # ---- the evaluation episode from the same state ----
        st_e, _ = _reset_env(ops, N, M, L)
        returns, act_e = _nan(N, M), _nan(T, B)
        ops.eval_episode_spread(pa, da, T, N, M, L, env_T, ENV_SEED, *st_e, det, SEED, COUNTER, cd, returns, act_e)
        torch.cuda.synchronize()
        what = f"deterministic {det} counter_dev {cdev}"
        assert torch.equal(act_e, act_r), f"{what}: actions differ in {(act_e != act_r).sum().item()} of {T * B} places"
        for name, a, b in zip(ENV_NAMES, st_e, st_r):
            assert torch.equal(a, b), f"{what}: env {name}"
        rew = rew_buf.cpu().numpy()
        acc = np.zeros(B, np.float32)
        for t in range(T):
            acc = acc + rew[t]                               # fp32, in step order
        assert torch.equal(returns.cpu().view(B), torch.from_numpy(acc)), f"{what}: returns"
        if T > 1:
            assert len(torch.unique(act_e)) > 1
        if env_T < T:
            assert int(st_e[4].min()) == 1 + T // env_T and st_e[3].cpu().tolist() == [T % env_T] * N        # resets inside the episode


@pytest.mark.gpu
@pytest.mark.parametrize("case", ER.F64_CASES, ids=[f"N{c[0]}-M{c[1]}-T{c[3]}" for c in ER.F64_CASES])
def test_eval_episode_matches_float64(ops, case):
    """deterministic = 1 against the float64 reference.  Envs whose float64 top-two logit gap falls below ER.MARGIN at any step are
    left out (at most ER.NEAR_CAP of the envs; the CPU test holds the committed seeds to that).  The others' actions are equal and
    their returns within T x (rtol 1e-6, atol 1e-6), the per-step reward tolerance of the env tests (test_mpe_env.py,
    test_gpu_episode_spread.py); the final positions within 1e-6."""
    N, M, L, T, env_T, relu, layer_N, wseed = case
    ref = ER.reference_episode(case)
    keep = ~ref["near"]
    assert 1.0 - keep.mean() <= ER.NEAR_CAP
    da = ops.net_desc(ER.obs_dim(M, L), 5, layer_N, relu)
    pa = _flat_from_module(ops, ER.make_actor(M, L, relu, layer_N, wseed), da, "act.action_out.linear")[0]
    pos, lpos = ER.start_state(N, M, L)
    f64 = dict(dtype=torch.float64, device="cuda")
    st = [torch.as_tensor(pos, **f64).contiguous(), torch.zeros(N, M, 2, **f64), torch.as_tensor(lpos, **f64).contiguous(),
          torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int64, device="cuda")]
    returns, actions = _nan(N, M), _nan(T, N * M)
    ops.eval_episode_spread(pa, da, T, N, M, L, env_T, ER.ENV_SEED, *st, 1, SEED, COUNTER, None, returns, actions)
    torch.cuda.synchronize()
    a = actions.cpu().numpy().reshape(T, N, M)
    ret = returns.cpu().numpy().astype(np.float64)
    err = np.abs(ret[keep] - ref["returns"][keep])
    print(f"\nleft out {int((~keep).sum())} of {N} envs | actions differ in {int((a[:, keep] != ref['actions'][:, keep]).sum())} places | "
          f"returns: max err {err.max():.3e}, max |return| {np.abs(ref['returns']).max():.3e}")
    np.testing.assert_array_equal(a[:, keep], ref["actions"][:, keep])
    np.testing.assert_allclose(ret[keep], ref["returns"][keep], rtol=T * 1e-6, atol=T * 1e-6)
    np.testing.assert_allclose(st[0].cpu().numpy()[keep], ref["pos"][keep], rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(st[4].cpu().numpy(), ref["episode"])
    np.testing.assert_array_equal(st[3].cpu().numpy(), ref["tstep"])


# ---- runner level ------------------------------------------------------------------------------------------------------------------
def _runner(N=16, M=3, L=3, T=25, env_T=25, layer_N=1, recurrent=False):
    """An MPERunner on the device env with a second, identically built env to evaluate on."""
    from mappo_amd.config import get_config
    from mappo_amd.envs.mpe_spread import SimpleSpreadVecEnv
    from mappo_amd.runner.shared.mpe_runner import MPERunner
    dev = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy, a.use_naive_recurrent_policy = recurrent, False
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.layer_N, a.use_hip_graph = layer_N, False
    torch.manual_seed(1)
    env, eval_env = (SimpleSpreadVecEnv(N, M, L, env_T, seed=s, device=dev) for s in (1, 2))
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=eval_env, num_agents=M, device=dev, run_dir=None))
    g = torch.Generator(device=dev).manual_seed(7)
    fp = r.policy.flat_params
    fp.add_(torch.randn(fp.shape, device=dev, generator=g) * 0.1)
    r.warmup()
    logged = []
    r.log_env = lambda info, steps: logged.append(info["eval_average_episode_rewards"][0])
    return r, eval_env, logged


@pytest.mark.gpu
def test_nothing_else_is_written(ops, monkeypatch):
    """returns sits inside a NaN-filled block and actions is NULL: the block around returns stays NaN.  Through the policy: the
    training sampling stream (the actor's device counter word and its host counter) is where it was."""
    N, M, L, T = 7, 3, 3, 5
    B, pad = N * M, 64
    da = ops.net_desc(ER.obs_dim(M, L), 5)
    pa = _flat_from_module(ops, ER.make_actor(M, L, True, 1, 5), da, "act.action_out.linear")[0]
    params = pa.clone()
    st, _ = _reset_env(ops, N, M, L)
    pool = _nan(pad + B + pad)
    ops.eval_episode_spread(pa, da, T, N, M, L, 25, ENV_SEED, *st, 0, SEED, COUNTER, None, pool[pad:pad + B].view(N, M), None)
    torch.cuda.synchronize()
    assert torch.isfinite(pool[pad:pad + B]).all() and (pool[pad:pad + B] < 0).all()
    assert torch.isnan(pool[:pad]).all() and torch.isnan(pool[pad + B:]).all()
    assert torch.equal(pa, params)
    r, eval_env, _ = _runner(N=N, T=T)
    actor = r.policy.actor
    actor._counter_dev.fill_(COUNTER_DEV)
    host = actor._sample_counter
    eval_env.reset()
    for det in (True, False):
        ret = r.policy.eval_episode_env_fused(eval_env.episode_state(), T, deterministic=det)
        assert tuple(ret.shape) == (N, M) and ret.device == r.policy.device and torch.isfinite(ret).all()
    assert int(actor._counter_dev.item()) == COUNTER_DEV and actor._sample_counter == host
    assert r.policy._eval_counter == 2 * T


@pytest.mark.gpu
def test_runner_eval_takes_the_launch_behind_the_flag(gpu_device, monkeypatch):
    """Flag set: MPERunner.eval calls the op once and no stepwise kernel, and logs the value of the flag-off loop on an identically
    seeded runner up to fp32 summation error.  Both paths add the same N M T fp32 step rewards (all negative) into a mean: a sum of K
    fp32 terms is off by at most (K - 1) 2^-24 sum |x|, the loop sums T terms per row and then N M rows, the launch likewise, so
    each value is within (T + N M) 2^-24 |value| of the exact mean and the two within twice that of each other.  Flag unset, or a
    recurrent policy, or layer_N 2: the op is not called.  eval is eager in both paths (no graph)."""
    N, M, T = 16, 3, 25
    names = ("eval_episode_spread", "actor_act", "mpe_spread_step")
    calls, restore = _counting(names)
    try:
        monkeypatch.setenv("MAPPO_SPREAD_EVAL_EPISODE", "1")
        r, _, logged = _runner(N=N, T=T)
        r.eval(0)
        assert calls == dict(eval_episode_spread=1, actor_act=0, mpe_spread_step=0), calls
        on = logged[0]
        monkeypatch.delenv("MAPPO_SPREAD_EVAL_EPISODE")
        r, _, logged = _runner(N=N, T=T)
        r.eval(0)
        assert calls["eval_episode_spread"] == 1 and calls["mpe_spread_step"] == T, calls
        off = logged[0]
        bound = 2 * (T + N * M) * 2.0 ** -24 * abs(off)
        print(f"\neval value: launch {on!r}, loop {off!r}, |diff| {abs(on - off):.3e}, bound {bound:.3e}")
        assert off < 0 and abs(on - off) <= bound
        monkeypatch.setenv("MAPPO_SPREAD_EVAL_EPISODE", "1")
        for kw in (dict(recurrent=True), dict(layer_N=2)):
            r, _, logged = _runner(N=4, T=3, **kw)
            r.eval(0)
            assert calls["eval_episode_spread"] == 1 and len(logged) == 1, (kw, calls)
    finally:
        restore()


@pytest.mark.gpu
def test_training_after_an_eval_is_unchanged(gpu_device, monkeypatch):
    """One run_episode after an eval through the launch leaves the parameters a run that did not evaluate has."""
    monkeypatch.setenv("MAPPO_SPREAD_EVAL_EPISODE", "1")
    params = []
    for evaluate in (True, False):
        r, _, logged = _runner(N=16, T=25)
        if evaluate:
            r.eval(0)
            assert len(logged) == 1
        r.run_episode()
        torch.cuda.synchronize()
        params.append(r.policy.flat_params.clone())
    assert torch.equal(params[0], params[1])
    assert not torch.equal(params[0], torch.zeros_like(params[0]))
