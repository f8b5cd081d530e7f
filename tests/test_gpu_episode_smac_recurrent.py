"""The one-launch rollout episode of a RECURRENT shared policy on SMAC-shaped env output (mappo_rollout_episode_smac_recurrent,
csrc/rollout_smac_rec.h; opt-in: MAPPO_SMAC_REC_EPISODE=1).  Against the stepwise path (mappo_recurrent_step_dual on slot 0, T - 1 x
mappo_recurrent_rollout_step, mappo_insert_smac into slot T) on the same weights, buffer, env state and counter every buffer array,
the returns and the env's state must be bit-identical: both run each row through gru_step3_tiles and categorical_act_mask.  An
independent check recomputes every step in float64 torch (tests/rec_ref.py) with the -1e10 availability mask and the host Philox draw.
The cases and their env seeds: tests/smac_episode_cases.py (tests/test_smac_rec_episode.py holds each seed to reaching every mask
branch)."""
import numpy as np
import pytest
import torch

import smac_episode_cases as SC

BUF_NAMES = ("obs", "share_obs", "available_actions", "rewards", "masks", "bad_masks", "active_masks", "actions", "action_log_probs",
             "value_preds", "returns", "rnn_states", "rnn_states_critic")
FLAG = "MAPPO_SMAC_REC_EPISODE"


def _runner(M, N, T, D, S, A, relu=True, layer_N=1, fnorm=True, centralized=True, naive=False, seed=1, graph=False, pool=None,
            recurrent=True, nan_fill=True, host=False):
    """host: the weights and slot 0 are the host-built ones of smac_episode_cases (what the CPU suite runs the reference on)."""
    from mappo_amd.envs.synthetic import SyntheticSMACEnv
    from mappo_amd.runner.shared.smac_runner import SMACRunner
    dev = torch.device("cuda:0")
    a = SC.make_args(M, N, T, relu, layer_N, fnorm, centralized, naive, recurrent, graph)
    torch.manual_seed(1)
    env = SyntheticSMACEnv(N, M, D, S, A, p_death=SC.P_DEATH, p_term=SC.P_TERM, seed=seed, device=dev, pool_steps=T if pool is None else pool)
    r = SMACRunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=M, device=dev, run_dir=None))
    # LayerNorm / feature-norm affines away from (1, 0), GRU biases away from 0 and larger weights: the same on both sides
    fp = r.policy.flat_params
    fp.add_(SC.perturbation(fp.numel()).to(dev).view(fp.shape))
    r.warmup()
    if host:
        ha, hc = SC.host_networks(M, N, T, D, S, A, relu, layer_N, fnorm, centralized)
        r.policy.actor.flat.copy_(ha.flat)
        r.policy.critic.flat.copy_(hc.flat)
        obs0, share0, avail0 = SC.host_slot0(N, M, D, S, A)
        b = r.buffer
        b.obs[0].copy_(obs0); b.share_obs[0].copy_(share0 if centralized else obs0); b.available_actions[0].copy_(avail0)
    if nan_fill:                                             # what a rollout does not write stays NaN on both sides
        b = r.buffer
        for n in ("obs", "share_obs", "available_actions", "masks", "bad_masks", "active_masks", "rnn_states", "rnn_states_critic"):
            getattr(b, n)[1:].fill_(float("nan"))
        for n in ("rewards", "actions", "action_log_probs", "value_preds", "returns"):
            getattr(b, n).fill_(float("nan"))
    return r, env


def _state(r, env):
    b = r.buffer
    out = {n: getattr(b, n).clone() for n in BUF_NAMES}
    out["counter"] = r.policy.actor._counter_dev.clone()
    out["buffer_step"] = b.step
    out["env.dead"] = env.dead.clone()
    out["env.ctr"] = env._pool["ctr"].clone()
    out["env._t"] = env._t
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(s0, s1, what=""):
    for k in s0:
        if torch.is_tensor(s0[k]):
            assert torch.equal(_bits(s0[k]), _bits(s1[k])), f"{what}{k}: {int((_bits(s0[k]) != _bits(s1[k])).sum())} words differ"
        else:
            assert s0[k] == s1[k], f"{what}{k}: {s0[k]} != {s1[k]}"


def _both_paths(monkeypatch, n_rollouts=2, graph_on=False, **kw):
    """`n_rollouts` rollouts through each path (flag off, flag on), after_update() in between as train() does; returns the states
    [path][rollout].  The episode op is counted: never with the flag off, once per rollout body with it on (a graph replay runs no
    Python: eager pass + capture = 2), so no case can pass by comparing the stepwise path with itself."""
    runs = []
    calls, restore = _counting(("rollout_episode_smac_recurrent",))
    try:
        for flag in ("0", "1"):
            monkeypatch.setenv(FLAG, flag)
            graph = graph_on and flag == "1"
            r, env = _runner(graph=graph, **kw)
            calls["rollout_episode_smac_recurrent"] = 0
            states = []
            for _ in range(n_rollouts):
                assert r._episode_launch_ok() == (flag == "1")
                r.rollout()
                torch.cuda.synchronize()
                states.append(_state(r, env))
                r.buffer.after_update()
            runs.append(states)
            assert calls["rollout_episode_smac_recurrent"] == (0 if flag == "0" else (2 if graph else n_rollouts))
            if graph:
                assert isinstance(r._rollout_graph, torch.cuda.CUDAGraph)
    finally:
        restore()
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,T,D,S,A,relu,layer_N,fnorm,centralized,naive,seed", SC.CASES)
def test_smac_recurrent_episode_launch_matches_stepwise(gpu_device, monkeypatch, M, N, T, D, S, A, relu, layer_N, fnorm, centralized, naive,
                                                         seed):
    """Two consecutive rollouts through each path: every buffer array (NaN-filled untouched slots included), the returns, the env's
    `dead` and counter words and the actor's sampling counter are equal bit for bit."""
    assert N * M <= 1024
    runs = _both_paths(monkeypatch, M=M, N=N, T=T, D=D, S=S, A=A, relu=relu, layer_N=layer_N, fnorm=fnorm, centralized=centralized,
                       naive=naive, seed=seed)
    for e in range(2):
        _assert_same(runs[0][e], runs[1][e], what=f"rollout {e}: ")
    first, second = runs[1]
    assert second["counter"].item() == first["counter"].item() + T
    assert not torch.isnan(first["actions"]).any() and not torch.isnan(first["rnn_states"]).any()
    assert float(first["rnn_states"][1:].abs().max()) > 0 and float(first["rnn_states_critic"][1:].abs().max()) > 0
    assert torch.equal(second["rnn_states"][0], first["rnn_states"][T]) and torch.equal(second["obs"][0], first["obs"][T])
    # the mask branches the CPU suite holds the seed to are in the buffer: ended envs (masks 0, zeroed states), dead rows of live envs
    assert float(first["masks"][1:].min()) == 0.0 and float(first["masks"][1:].max()) == 1.0
    ended = first["masks"][1:] == 0
    assert float(first["rnn_states"][1:][ended.view(T, N, M)].abs().max()) == 0.0
    assert bool((first["active_masks"][1:][ended] == 1).all())
    if M >= 2:
        assert float(first["active_masks"][1:].min()) == 0.0
    # a sampled action is always an available one
    act = first["actions"].long()
    assert bool((first["available_actions"][:T].gather(-1, act) == 1).all())


@pytest.mark.gpu
def test_smac_recurrent_episode_graph_replay_matches_eager(gpu_device, monkeypatch):
    """Through the runner's hipGraph rollout(): an eager pass, the capture and three replays leave what five eager stepwise
    rollouts leave, and successive replays draw different actions."""
    M, N, T, D, S, A = 3, 7, 6, 30, 48, 9
    runs = _both_paths(monkeypatch, n_rollouts=5, graph_on=True, M=M, N=N, T=T, D=D, S=S, A=A, seed=2)
    for e in range(5):
        for s in (runs[0][e], runs[1][e]):
            s.pop("env._t")                                  # a host counter: a replay runs no Python (in either path)
        _assert_same(runs[0][e], runs[1][e], what=f"call {e}: ")
    for e in (2, 3, 4):                                      # replays: new env data and new samples
        assert not torch.equal(runs[1][e]["obs"], runs[1][e - 1]["obs"])
        assert not torch.equal(runs[1][e]["actions"], runs[1][e - 1]["actions"])
        assert runs[1][e]["counter"].item() == runs[1][e - 1]["counter"].item() + T


def _check_float64(r, env, M, N, T, A, centralized, use_avail=True, bad=None):
    """One episode launch on the runner's buffer, checked step by step in float64 (see the test below).  use_avail False: the env's
    avail and the buffer's available_actions are not handed over (no mask; the buffer's array stays untouched); bad: the env's
    bad_transition [N, M] bool."""
    import rec_ref
    from rollout_ref import philox_u32
    from mappo_amd import ops
    b, pol = r.buffer, r.policy
    ctr0 = int(pol.actor._counter_dev.item())
    block = env.episode_block()
    if bad is not None:
        block = block[:4] + (bad,) + block[5:]
    if use_avail:
        pol.collect_episode_smac_fused_recurrent(b, block, centralized)
    else:
        ops.rollout_episode_smac_recurrent(pol.actor.flat, pol.actor.desc, pol.critic.flat, pol.critic.desc, block[0],
                                           block[1] if centralized else None, None, block[2], block[3], block[4], False, pol.actor._seed,
                                           0, pol.actor._counter_dev, b.obs, b.share_obs, None, b.rewards, b.masks, b.bad_masks,
                                           b.active_masks, b.rnn_states, b.rnn_states_critic, b.actions, b.action_log_probs, b.value_preds,
                                           centralized)
    torch.cuda.synchronize()
    wa, wc = rec_ref.weights64(pol.actor, "act.action_out.linear"), rec_ref.weights64(pol.critic, "v_out")
    R = N * M
    d = lambda t: t.double().cpu()
    e_obs, e_share, e_rew, e_done, e_bad, e_avail = block
    skipped = 0
    for k in range(T):
        mask, keep = d(b.masks[k]).view(R, 1), d(b.masks[k + 1]).view(R, 1)
        ha, logits = rec_ref.step64(wa, pol.actor.desc, "act.action_out.linear", d(b.obs[k]).view(R, -1), d(b.rnn_states[k]).view(R, 64), mask)
        hc, value = rec_ref.step64(wc, pol.critic.desc, "v_out", d(b.share_obs[k]).view(R, -1), d(b.rnn_states_critic[k]).view(R, 64), mask)
        assert (d(b.rnn_states[k + 1]).view(R, 64) - ha * keep).abs().max().item() < 1e-5, f"actor state, step {k}"
        assert (d(b.rnn_states_critic[k + 1]).view(R, 64) - hc * keep).abs().max().item() < 1e-5, f"critic state, step {k}"
        assert (d(b.value_preds[k]).view(R, 1) - value).abs().max().item() < 1e-5, f"value, step {k}"
        avail = d(b.available_actions[k]).view(R, A) if use_avail else torch.ones(R, A, dtype=torch.float64)
        logits = torch.where(avail == 0, torch.full_like(logits, -1e10), logits)
        logp = torch.log_softmax(logits, dim=-1)
        act = d(b.actions[k]).view(R).long()
        assert int(act.min()) >= 0 and int(act.max()) < A
        assert bool((avail.gather(1, act.view(R, 1)) == 1).all()), f"an unavailable action was sampled, step {k}"
        assert (d(b.action_log_probs[k]).view(R) - logp.gather(1, act.view(R, 1)).view(R)).abs().max().item() < 1e-5, f"log-prob, step {k}"
        u = (philox_u32(pol.actor._seed, ctr0 + k, np.arange(R, dtype=np.int64)) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        cdf = logp.exp().cumsum(dim=-1).numpy()
        clear = (np.abs(cdf - u[:, None]) > 1e-5).all(axis=1)
        want = np.minimum((cdf <= u[:, None]).sum(axis=1), A - 1)
        skipped += int((~clear).sum())
        assert np.array_equal(act.numpy()[clear], want[clear]), f"sampled action, step {k}"
        # the insert of env output k into slot k + 1 (smac_runner.py:129-151)
        done = e_done[k].cpu()
        done_env = done.all(dim=1, keepdim=True)
        assert torch.equal(b.masks[k + 1].cpu().view(N, M), (~done_env).float().expand(N, M))
        assert torch.equal(b.active_masks[k + 1].cpu().view(N, M), torch.where(done_env, torch.ones(N, M), (~done).float()))
        assert torch.equal(b.bad_masks[k + 1].cpu().view(N, M), torch.ones(N, M) if bad is None else (~bad).float().cpu())
        assert torch.equal(b.obs[k + 1], e_obs[k]) and torch.equal(b.share_obs[k + 1], e_share[k] if centralized else e_obs[k])
        if use_avail:
            assert torch.equal(b.available_actions[k + 1], e_avail[k])
        else:
            assert bool(torch.isnan(b.available_actions[k + 1]).all())     # not handed over: not written
        assert torch.equal(b.rewards[k].view(N, M), e_rew[k].view(N, 1).expand(N, M))
    assert skipped <= 0.01 * T * R, skipped


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,T,D,S,A,relu,layer_N,fnorm,centralized,seed,pseed", SC.F64_CASES)
def test_smac_recurrent_episode_matches_float64_step_by_step(gpu_device, M, N, T, D, S, A, relu, layer_N, fnorm, centralized, seed, pseed):
    """Independent of the stepwise kernels: from the stored obs[k], share_obs[k], rnn_states[k], rnn_states_critic[k], masks[k] and
    available_actions[k] a float64 torch forward gives the next states, the log-prob of the stored action (logits of unavailable
    actions at -1e10) and the value to 1e-5 (the bar gru_step3.h states for its gate forms and tests/test_gpu_gru.py applies), and
    the stored action is the inverse-CDF draw of the host Philox uniform (seed, counter + k, buffer row) on the float64 CDF wherever
    the uniform is not within 1e-5 of a CDF edge (rows nearer: skipped, at most 1 %; on these host-built weights and slot-0 rows
    tests/test_smac_rec_episode.py holds the float64 reference alone to that cap).  The insert's masks are recomputed from the env's
    dones.  The second case has more than 1024 rows, where the stepwise path is another kernel."""
    r, env = _runner(M, N, T, D, S, A, relu=relu, layer_N=layer_N, fnorm=fnorm, centralized=centralized, seed=seed, host=True)
    _check_float64(r, env, M, N, T, A, centralized)


@pytest.mark.gpu
def test_smac_recurrent_episode_without_avail_and_with_bad_transitions(gpu_device):
    """The two branches the runner never reaches on the synthetic env, through a direct call: no available_actions (env_avail and
    the buffer's array NULL: no mask, the array untouched) and bad_transition bytes that are set (bad_masks = 0 on those rows, every
    slot) — checked in float64 as above."""
    M, N, T, D, S, A = 3, 7, 3, 30, 48, 9
    r, env = _runner(M, N, T, D, S, A, seed=2, host=True)
    bad = (torch.arange(N * M, device="cuda:0").view(N, M) % 4) == 1
    _check_float64(r, env, M, N, T, A, True, use_avail=False, bad=bad)
    assert float(r.buffer.bad_masks[1:].min()) == 0.0 and float(r.buffer.bad_masks[1:].max()) == 1.0


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


@pytest.mark.gpu
def test_smac_recurrent_episode_path_is_taken_only_with_the_flag(gpu_device, monkeypatch):
    """MAPPO_SMAC_REC_EPISODE=1 selects the one-launch episode, once per rollout and without any step op, for a qualifying policy and
    env; unset or 0 keeps the stepwise loop; pool_steps != episode_length, a 65-wide observation, layer_N = 2 and a feed-forward
    policy keep the ops — and the results — they have without the flag."""
    T = 4
    names = ("rollout_episode_smac_recurrent", "recurrent_step_dual", "recurrent_rollout_step", "insert_smac")
    calls, restore = _counting(names)
    shape = dict(M=3, N=5, T=T, D=30, S=48, A=9)

    def run(**kw):
        for n in names:
            calls[n] = 0
        r, env = _runner(**{**shape, **kw})
        r.rollout()
        torch.cuda.synchronize()
        return dict(calls), _state(r, env)
    try:
        monkeypatch.setenv(FLAG, "1")
        assert run()[0] == dict(rollout_episode_smac_recurrent=1, recurrent_step_dual=0, recurrent_rollout_step=0, insert_smac=0)
        stepwise = dict(rollout_episode_smac_recurrent=0, recurrent_step_dual=1, recurrent_rollout_step=T - 1, insert_smac=1)
        monkeypatch.setenv(FLAG, "0")
        assert run()[0] == stepwise
        monkeypatch.delenv(FLAG)
        assert run()[0] == stepwise
        others = [dict(pool=2), dict(D=65, S=65), dict(layer_N=2), dict(recurrent=False)]
        off = [run(**kw) for kw in others]
        monkeypatch.setenv(FLAG, "1")
        for kw, (c0, s0) in zip(others, off):
            c1, s1 = run(**kw)
            assert c1 == c0 and c1["rollout_episode_smac_recurrent"] == 0, kw
            _assert_same(s0, s1, what=f"{kw}: ")
    finally:
        restore()


@pytest.mark.gpu
def test_smac_recurrent_episode_training_iteration_matches_stepwise(gpu_device, monkeypatch):
    """run_episode() with the flag on equals the same iteration with the flag off, bit for bit: parameters, Adam state, ValueNorm
    state and train_infos."""
    out = []
    for flag in ("0", "1"):
        monkeypatch.setenv(FLAG, flag)
        r, env = _runner(3, 7, 6, 30, 48, 9, seed=2, nan_fill=False)
        infos, _ = r.run_episode(0, 2)
        torch.cuda.synchronize()
        pol = r.policy
        st = dict(params=pol.flat_params.clone(), exp_avg=pol.exp_avg.clone(), exp_avg_sq=pol.exp_avg_sq.clone(), opt_step=pol.opt_step.clone())
        if r.trainer._use_valuenorm:
            st["valuenorm"] = r.trainer.value_normalizer.state.clone()
        st.update(_state(r, env))
        out.append((st, {k: float(v) for k, v in infos.items()}))
    _assert_same(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]
    assert all(np.isfinite(v) for v in out[1][1].values())
