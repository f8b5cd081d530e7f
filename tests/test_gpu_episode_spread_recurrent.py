"""The one-launch rollout episode of a RECURRENT shared policy on the GPU-resident simple_spread env
(mappo_rollout_episode_spread_recurrent, csrc/rollout_spread_rec.h; opt-in: MAPPO_SPREAD_REC_EPISODE=1).  Against the stepwise path
(T x (mappo_recurrent_step_dual + mappo_mpe_spread_step + mappo_insert_mpe_rnn)) on the same weights, buffer, env state and counter
every buffer array, the returns and the env's state must be bit-identical: both run each row through gru_step3_tiles and each
environment through mpe_step_env.  An independent check recomputes every step in float64 torch (tests/rec_ref.py)."""
import pytest
import torch

BUF_NAMES = ("obs", "share_obs", "rewards", "masks", "bad_masks", "active_masks", "actions", "action_log_probs", "value_preds", "returns",
             "rnn_states", "rnn_states_critic")
ENV_NAMES = ("agent_pos", "agent_vel", "landmark_pos", "tstep", "episode")
FLAG = "MAPPO_SPREAD_REC_EPISODE"


def _runner(centralized=True, layer_N=1, relu=True, fnorm=True, N=16, M=3, L=3, T=8, env_T=25, graph=False, naive=False, recurrent=True,
            env_cls=None):
    from mappo_amd.config import get_config
    from mappo_amd.envs.mpe_spread import SimpleSpreadVecEnv
    from mappo_amd.runner.shared.mpe_runner import MPERunner
    dev = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy, a.use_naive_recurrent_policy = recurrent and not naive, recurrent and naive
    a.recurrent_N = 1
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.use_centralized_V, a.layer_N, a.use_ReLU, a.use_feature_normalization = centralized, layer_N, relu, fnorm
    a.use_hip_graph = graph
    torch.manual_seed(1)
    env = (env_cls or SimpleSpreadVecEnv)(N, M, L, env_T, seed=1, device=dev)
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=M, device=dev, run_dir=None))
    # LayerNorm / feature-norm affines away from (1, 0), GRU biases away from 0 and larger weights: the same on both sides
    g = torch.Generator(device=dev).manual_seed(7)
    fp = r.policy.flat_params
    fp.add_(torch.randn(fp.shape, device=dev, generator=g) * 0.1)
    r.warmup()
    return r, env


def _state(r, env):
    b = r.buffer
    out = {n: getattr(b, n).clone() for n in BUF_NAMES}
    out["counter"] = r.policy.actor._counter_dev.clone()
    out["buffer_step"] = b.step
    for n in ENV_NAMES:
        out["env." + n] = getattr(env, n).clone()
    return out


def _assert_same(s0, s1, what=""):
    for k in s0:
        if torch.is_tensor(s0[k]):
            assert torch.equal(s0[k], s1[k]), f"{what}{k}: max |diff| {(s0[k].double() - s1[k].double()).abs().max().item()}"
        else:
            assert s0[k] == s1[k], f"{what}{k}: {s0[k]} != {s1[k]}"


def _both_paths(monkeypatch, n_rollouts=2, **kw):
    """`n_rollouts` rollouts through each path (flag off, flag on), after_update() in between as train() does; returns the states
    [path][rollout]."""
    runs = []
    for flag in ("0", "1"):
        monkeypatch.setenv(FLAG, flag)
        r, env = _runner(**kw)
        states = []
        for _ in range(n_rollouts):
            r.rollout()
            torch.cuda.synchronize()
            states.append(_state(r, env))
            r.buffer.after_update()
        runs.append(states)
    return runs


CASES = [  # (M, L, centralized, N, layer_N, relu, feature norm, naive, env episode length, T)
    (3, 3, True, 16, 1, True, True, False, 25, 8),       # 15-row tiles, the last tile partial (one environment)
    (2, 2, True, 9, 0, False, False, False, 25, 6),      # full 16-row tiles, the last one partial
    (5, 2, False, 4, 1, False, True, False, 25, 6),      # G = 3
    (7, 1, False, 3, 0, True, False, False, 25, 6),      # G = 2: a 14-row tile
    (3, 3, False, 16, 0, True, True, False, 25, 5),
    (3, 3, True, 16, 1, False, False, False, 25, 5),
    (3, 3, True, 16, 1, True, True, True, 25, 5),        # use_naive_recurrent_policy
    (3, 3, True, 6, 1, True, True, False, 25, 1),        # T = 1
    (3, 3, True, 8, 1, True, True, False, 3, 7),         # resets, masks = 0 and zeroed states inside the rollout
    (3, 3, False, 8, 1, False, True, False, 3, 6),       # ... and on its last slot
]


@pytest.mark.gpu
@pytest.mark.parametrize("M,L,centralized,N,layer_N,relu,fnorm,naive,env_T,T", CASES)
def test_recurrent_episode_launch_matches_stepwise(gpu_device, monkeypatch, M, L, centralized, N, layer_N, relu, fnorm, naive, env_T, T):
    runs = _both_paths(monkeypatch, centralized=centralized, layer_N=layer_N, relu=relu, fnorm=fnorm, N=N, M=M, L=L, T=T, env_T=env_T,
                       naive=naive)
    for e in range(2):
        _assert_same(runs[0][e], runs[1][e], what=f"rollout {e}: ")
    first, second = runs[1]
    assert not torch.equal(first["actions"], second["actions"]) or T == 1            # fresh sampling stream
    assert second["counter"].item() == first["counter"].item() + T
    assert float(first["rnn_states"][1:].abs().max()) > 0 and float(first["rnn_states_critic"][1:].abs().max()) > 0
    assert torch.equal(second["rnn_states"][0], first["rnn_states"][T]) and torch.equal(second["obs"][0], first["obs"][T])
    if env_T == 3:
        done_slots = [3, 6]                                  # env steps 3 and 6 of the first rollout end an episode
        for s in range(1, T + 1):
            want = 0.0 if s in done_slots else 1.0
            assert float(first["masks"][s].min()) == want and float(first["masks"][s].max()) == want
            zeroed = float(first["rnn_states"][s].abs().max()) == 0.0 and float(first["rnn_states_critic"][s].abs().max()) == 0.0
            assert zeroed == (s in done_slots)
        assert int(first["env.tstep"].max()) == T % 3
    else:
        assert float(first["masks"].min()) == 1.0


@pytest.mark.gpu
def test_recurrent_episode_graph_replay_matches_eager(gpu_device, monkeypatch):
    """Through the runner's hipGraph rollout(): an eager pass, the capture and two replays leave what four eager stepwise
    rollouts leave."""
    runs = []
    for flag, graph in (("0", False), ("1", True)):
        monkeypatch.setenv(FLAG, flag)
        r, env = _runner(N=16, T=8, graph=graph)
        states = []
        for _ in range(4):
            r.rollout()
            torch.cuda.synchronize()
            states.append(_state(r, env))
            r.buffer.after_update()
        runs.append(states)
        if graph:
            assert isinstance(r._rollout_graph, torch.cuda.CUDAGraph)
    for e in range(4):
        _assert_same(runs[0][e], runs[1][e], what=f"call {e}: ")
    for e in (2, 3):                                         # replays: new env data and new samples
        assert not torch.equal(runs[1][e]["obs"], runs[1][e - 1]["obs"])
        assert runs[1][e]["counter"].item() == runs[1][e - 1]["counter"].item() + 8


@pytest.mark.gpu
@pytest.mark.parametrize("centralized,layer_N,relu,env_T", [(True, 1, True, 25), (False, 0, False, 3)])
def test_recurrent_episode_matches_float64_step_by_step(gpu_device, centralized, layer_N, relu, env_T):
    """Independent of the stepwise kernels: from the stored obs[t], share_obs[t], rnn_states[t], rnn_states_critic[t] and masks[t]
    a float64 torch forward gives the next states, the log-prob of the stored action and the value to 1e-5 (the bar gru_step3.h
    states for its gate forms and tests/test_gpu_gru.py applies); in this deterministic run the stored action is the float64
    argmax wherever the float64 top-two gap exceeds 1e-4 (rows below: skipped, at most 2 %)."""
    import rec_ref
    T, N, M = 8, 16, 3
    r, env = _runner(centralized=centralized, layer_N=layer_N, relu=relu, N=N, M=M, T=T, env_T=env_T)
    b, pol = r.buffer, r.policy
    pol.collect_episode_env_fused_recurrent(b, env.episode_state(), centralized, deterministic=True)
    torch.cuda.synchronize()
    wa, wc = rec_ref.weights64(pol.actor, "act.action_out.linear"), rec_ref.weights64(pol.critic, "v_out")
    R = N * M
    d = lambda t: t.double().cpu()
    skipped = 0
    for t in range(T):
        mask, keep = d(b.masks[t]).view(R, 1), d(b.masks[t + 1]).view(R, 1)
        ha, logits = rec_ref.step64(wa, pol.actor.desc, "act.action_out.linear", d(b.obs[t]).view(R, -1), d(b.rnn_states[t]).view(R, 64), mask)
        hc, value = rec_ref.step64(wc, pol.critic.desc, "v_out", d(b.share_obs[t]).view(R, -1), d(b.rnn_states_critic[t]).view(R, 64), mask)
        assert (d(b.rnn_states[t + 1]).view(R, 64) - ha * keep).abs().max().item() < 1e-5, f"actor state, step {t}"
        assert (d(b.rnn_states_critic[t + 1]).view(R, 64) - hc * keep).abs().max().item() < 1e-5, f"critic state, step {t}"
        assert (d(b.value_preds[t]).view(R, 1) - value).abs().max().item() < 1e-5, f"value, step {t}"
        logp = torch.log_softmax(logits, dim=-1)
        act = d(b.actions[t]).view(R).long()
        assert int(act.min()) >= 0 and int(act.max()) <= 4
        assert (d(b.action_log_probs[t]).view(R) - logp.gather(1, act.view(R, 1)).view(R)).abs().max().item() < 1e-5, f"log-prob, step {t}"
        top = logits.topk(2, dim=-1).values
        clear = (top[:, 0] - top[:, 1]) > 1e-4
        skipped += int((~clear).sum())
        assert torch.equal(act[clear], logits.argmax(dim=-1)[clear]), f"argmax, step {t}"
    assert skipped <= 0.02 * T * R, skipped
    if env_T == 3:
        assert float(b.masks[3].max()) == 0.0 and float(b.rnn_states[3].abs().max()) == 0.0


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
def test_recurrent_episode_path_is_taken_only_with_the_flag(gpu_device, monkeypatch):
    """MAPPO_SPREAD_REC_EPISODE=1 selects the one-launch episode for a qualifying recurrent policy; unset or 0 keeps the stepwise
    loop; layer_N = 2, a 65-wide observation and a feed-forward policy keep the paths they have without the flag."""
    from mappo_amd.envs.mpe_spread import SimpleSpreadVecEnv
    T = 4
    names = ("rollout_episode_spread_recurrent", "recurrent_step_dual", "rollout_episode_spread", "mpe_spread_step")
    calls, restore = _counting(names)

    def run(**kw):
        for n in names:
            calls[n] = 0
        r, _ = _runner(N=4, T=T, **kw)
        r.rollout()
        return dict(calls)
    try:
        monkeypatch.setenv(FLAG, "1")
        assert run() == dict(rollout_episode_spread_recurrent=1, recurrent_step_dual=0, rollout_episode_spread=0, mpe_spread_step=0)
        monkeypatch.setenv(FLAG, "0")
        assert run() == dict(rollout_episode_spread_recurrent=0, recurrent_step_dual=T, rollout_episode_spread=0, mpe_spread_step=T)
        monkeypatch.delenv(FLAG)
        assert run() == dict(rollout_episode_spread_recurrent=0, recurrent_step_dual=T, rollout_episode_spread=0, mpe_spread_step=T)
        off = run(layer_N=2)
        ff_off = run(recurrent=False)
        monkeypatch.setenv(FLAG, "1")
        assert run(layer_N=2) == off and off["rollout_episode_spread_recurrent"] == 0 and off["mpe_spread_step"] == T
        assert run(recurrent=False) == ff_off == dict(rollout_episode_spread_recurrent=0, recurrent_step_dual=0, rollout_episode_spread=1,
                                                      mpe_spread_step=0)

        class WideSpread(SimpleSpreadVecEnv):
            """Declares 65 observation features (the policy is built from the declared spaces; the env is never stepped here)."""
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                self.observation_space = [[65] for _ in range(self.M)]
                self.share_observation_space = [[65] for _ in range(self.M)]
        from mappo_amd.config import get_config
        from mappo_amd.runner.shared.mpe_runner import MPERunner
        dev = torch.device("cuda:0")
        a = get_config().parse_known_args([])[0]
        a.use_recurrent_policy, a.recurrent_N, a.episode_length, a.n_rollout_threads, a.env_name = True, 1, T, 4, "MPE"
        a.use_centralized_V = False
        wide = MPERunner(dict(all_args=a, envs=WideSpread(4, 3, 3, 25, seed=1, device=dev), eval_envs=None, num_agents=3, device=dev,
                              run_dir=None))
        assert wide.policy.actor.desc.in_dim == 65
        assert not wide.policy.can_fuse_episode_recurrent() and not wide._episode_state_env()
    finally:
        restore()
