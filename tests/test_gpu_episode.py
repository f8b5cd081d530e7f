"""The one-launch rollout episode (mappo_rollout_episode, csrc/mlp_fwd16.h episode16r_body): against the stepwise fused path
(T x mappo_rollout_step + the bootstrap launch) on the same weights, buffer, env pool and counter, every buffer array must be
bit-identical — both paths run each tile through the same tile16r_step.  Plus the argument checks, which need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

BUF_NAMES = ("obs", "share_obs", "rewards", "masks", "actions", "action_log_probs", "value_preds", "returns")


def _runner(episode, centralized=True, layer_N=1, relu=True, fnorm=True, N=16, M=3, D=18, A=5, T=25, graph=False):
    from mappo_amd.config import get_config
    from mappo_amd.envs.synthetic import SyntheticMPEEnv
    from mappo_amd.runner.shared.mpe_runner import MPERunner
    dev = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.use_centralized_V, a.layer_N, a.use_ReLU, a.use_feature_normalization = centralized, layer_N, relu, fnorm
    a.use_hip_graph, a.fuse_rollout_episode = graph, episode
    torch.manual_seed(1)
    env = SyntheticMPEEnv(N, M, D, A, T, seed=1, device=dev)
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=M, device=dev, run_dir=None))
    # LayerNorm / feature-norm affines away from (1, 0) and larger weights: the same perturbation on both sides
    g = torch.Generator(device=dev).manual_seed(7)
    fp = r.policy.flat_params
    fp.add_(torch.randn(fp.shape, device=dev, generator=g) * 0.1)
    r.warmup()
    return r, env


def _state(r, env):
    b = r.buffer
    out = {n: getattr(b, n).clone() for n in BUF_NAMES}
    out["next_values"] = r._next_values.clone()
    out["counter"] = r.policy.actor._counter_dev.clone()
    out["env_t"] = env.t
    out["buffer_step"] = b.step
    return out


def _assert_same(s0, s1, what=""):
    for k in s0:
        if torch.is_tensor(s0[k]):
            assert torch.equal(s0[k], s1[k]), f"{what}{k}: max |diff| {(s0[k].double() - s1[k].double()).abs().max().item()}"
        else:
            assert s0[k] == s1[k], f"{what}{k}: {s0[k]} != {s1[k]}"


CASES = [  # (centralized, layer_N, relu, feature norm, N)
    (True, 1, True, True, 1024),        # the bench shape (BASELINE configs[1])
    (False, 1, True, True, 8),
    (True, 0, False, True, 1000),
    (False, 2, True, False, 1000),
    (True, 2, False, True, 8),
    (False, 0, True, False, 8),
    (True, 1, False, False, 1000),
]


@pytest.mark.gpu
@pytest.mark.parametrize("centralized,layer_N,relu,fnorm,N", CASES)
def test_episode_launch_matches_stepwise(gpu_device, centralized, layer_N, relu, fnorm, N):
    """Two eager episodes through each path: every buffer array, the bootstrap values, the counter word and env.t agree bit for
    bit (B = 3 N rows: 8 and 1000 threads leave a partial last tile)."""
    runs = []
    for episode in (False, True):
        r, env = _runner(episode, centralized, layer_N, relu, fnorm, N)
        states = []
        for _ in range(2):
            r.rollout()
            states.append(_state(r, env))
        torch.cuda.synchronize()
        runs.append(states)
    for e in range(2):
        _assert_same(runs[0][e], runs[1][e], what=f"episode {e}: ")
    assert runs[1][1]["env_t"] == 2 * 25
    assert not torch.equal(runs[1][0]["actions"], runs[1][1]["actions"])          # fresh pool + fresh sampling stream


@pytest.mark.gpu
def test_episode_path_is_taken_and_flag_turns_it_off(gpu_device):
    """The runner takes the one-launch episode when the env hands out whole episodes (and only then); --fuse_rollout_episode
    selects the stepwise loop on the same build."""
    from mappo_amd import ops
    calls = {"episode": 0, "step": 0}
    orig_e, orig_s = ops.rollout_episode, ops.rollout_step

    def e(*a, **k):
        calls["episode"] += 1
        return orig_e(*a, **k)

    def s(*a, **k):
        calls["step"] += 1
        return orig_s(*a, **k)
    ops.rollout_episode, ops.rollout_step = e, s
    try:
        r, _ = _runner(True)
        r.rollout()
        assert calls == {"episode": 1, "step": 0}, calls
        r, _ = _runner(False)
        r.rollout()
        assert calls == {"episode": 1, "step": 26}, calls
    finally:
        ops.rollout_episode, ops.rollout_step = orig_e, orig_s


@pytest.mark.gpu
@pytest.mark.parametrize("centralized", [True, False])
def test_episode_graph_replay_matches_stepwise(gpu_device, centralized):
    """Runner level through the hipGraph path: eager episode, capture, then replays (n_warm = 2).  Both runners leave identical
    buffers after every call, and each replayed episode sees fresh pool data and a fresh sampling stream."""
    runs = []
    for episode in (False, True):
        r, env = _runner(episode, centralized, N=64, graph=True)
        states = []
        for _ in range(4):
            r.rollout()
            torch.cuda.synchronize()
            states.append(_state(r, env))
        assert isinstance(r._rollout_graph, torch.cuda.CUDAGraph)
        runs.append(states)
    for e in range(4):
        _assert_same(runs[0][e], runs[1][e], what=f"call {e}: ")
    for e in (2, 3):                                         # replays: new env data and new samples
        assert not torch.equal(runs[1][e]["obs"], runs[1][e - 1]["obs"])
        assert not torch.equal(runs[1][e]["actions"], runs[1][e - 1]["actions"])
        assert runs[1][e]["counter"].item() == runs[1][e - 1]["counter"].item() + 25


def test_rollout_episode_rejects_bad_arguments():
    """mappo_rollout_episode validates its arguments on the host before any launch: error code + message, no GPU needed."""
    from mappo_amd import _lib
    lib = _lib.load()
    ND = _lib.NetDesc
    actor, critic = ND(18, 64, 5, 1, 1, 1, 0), ND(54, 64, 1, 1, 1, 1, 0)

    def call(a, c, T=25, N=8, M=3, sm=18, centralized=1):
        rc = lib.mappo_rollout_episode(None, ctypes.byref(a), None, ctypes.byref(c), T, N, M, None, 25 * 55, 55, sm, None, 0, 0, 0,
                                       None, 0, 0, 0, 0, 1, 0, None, None, None, None, None, None, None, None, None, centralized, None)
        return rc, lib.mappo_last_error().decode()

    cases = [
        (dict(a=ND(18, 64, 5, 1, 1, 1, 1), c=critic), "recurrent"),
        (dict(a=ND(128, 64, 5, 1, 1, 1, 0), c=ND(128, 64, 1, 1, 1, 1, 0), centralized=0), "narrow"),
        (dict(a=actor, c=ND(54, 64, 1, 2, 1, 1, 0)), "layer_N"),
        (dict(a=actor, c=ND(54, 64, 1, 1, 0, 1, 0)), "activation"),
        (dict(a=actor, c=ND(54, 64, 5, 1, 1, 1, 0)), "out_dim"),
        (dict(a=actor, c=critic, T=0), "bad shape"),
        (dict(a=actor, c=critic, M=0), "bad shape"),
        (dict(a=actor, c=critic, sm=19), "centralized"),
        (dict(a=actor, c=ND(18, 64, 1, 1, 1, 1, 0)), "centralized"),
        (dict(a=actor, c=critic, centralized=0), "in_dim"),
        (dict(a=actor, c=critic), "null pointer"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc == -1, (kw, rc)
        assert "rollout_episode" in err and msg in err, (kw, err)
