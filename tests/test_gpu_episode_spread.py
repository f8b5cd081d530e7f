"""The one-launch rollout episode on the GPU-resident simple_spread env (mappo_rollout_episode_spread, csrc/rollout_spread.h): the
env steps run inside the rollout kernel.  Against the stepwise fused path (T x (mappo_rollout_step + mappo_mpe_spread_step) + the
bootstrap launch) on the same weights, buffer, env state and counter, every buffer array and the env's five state tensors must be
bit-identical — both paths run each row through the same tile16r_step and each environment through the same mpe_step_env.  An
independent check replays the recorded actions through the NumPy oracle.  Plus the argument checks, which need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

BUF_NAMES = ("obs", "share_obs", "rewards", "masks", "actions", "action_log_probs", "value_preds", "returns")
ENV_NAMES = ("agent_pos", "agent_vel", "landmark_pos", "tstep", "episode")


def _runner(episode, centralized=True, layer_N=1, relu=True, fnorm=True, N=16, M=3, L=3, T=25, env_T=25, graph=False, env_cls=None):
    from mappo_amd.config import get_config
    from mappo_amd.envs.mpe_spread import SimpleSpreadVecEnv
    from mappo_amd.runner.shared.mpe_runner import MPERunner
    dev = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.use_centralized_V, a.layer_N, a.use_ReLU, a.use_feature_normalization = centralized, layer_N, relu, fnorm
    a.use_hip_graph, a.fuse_rollout_episode = graph, episode
    torch.manual_seed(1)
    env = (env_cls or SimpleSpreadVecEnv)(N, M, L, env_T, seed=1, device=dev)
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


CASES = [  # (M, L, centralized, N, layer_N, relu, feature norm, env episode length)
    (3, 3, True, 1024, 1, True, True, 25),        # the bench shape; 1024 envs in tiles of 5: the last tile is partial
    (3, 3, False, 8, 0, False, True, 25),
    (2, 2, True, 1000, 2, True, False, 25),
    (4, 4, False, 37, 1, False, False, 25),
    (5, 5, False, 8, 2, False, True, 25),
    (3, 3, True, 37, 0, True, False, 25),
    (3, 3, True, 64, 1, True, True, 10),          # resets inside the launch, a non-zero tstep at the start of the second one
]


def _both_paths(M, L, centralized, N, layer_N, relu, fnorm, env_T, T=25):
    """Two eager episodes through each path: every buffer array, the bootstrap values, the counter word and the env's five state
    tensors agree bit for bit.  Returns the states [path][episode] (path 1: the one-launch episode) and the env state both paths
    started from."""
    runs = []
    for episode in (False, True):
        r, env = _runner(episode, centralized, layer_N, relu, fnorm, N, M, L, T=T, env_T=env_T)
        start = {n: getattr(env, n).cpu().numpy().copy() for n in ENV_NAMES}
        states = []
        for _ in range(2):
            r.rollout()
            states.append(_state(r, env))
        torch.cuda.synchronize()
        runs.append(states)
    for e in range(2):
        _assert_same(runs[0][e], runs[1][e], what=f"episode {e}: ")
    assert not torch.equal(runs[1][0]["actions"], runs[1][1]["actions"])          # fresh sampling stream
    assert not torch.equal(runs[1][0]["obs"], runs[1][1]["obs"])
    return runs, start


def _replay_through_oracle(buf, start, env_T, reset_states):
    """The actions `buf` recorded, replayed through the NumPy oracle from the env state `start` (saved before the launch), give its
    observations, rewards and masks (1e-6: the fp32 cast of the outputs, the tolerance of
    test_mpe_env.py::test_kernel_matches_oracle_step_by_step).  reset_states(n): the state environment n takes when its episode
    ends.  Returns the number of episodes that ended."""
    from oracle import mpe_oracle as R
    obs, rew, masks = (buf[k].cpu().numpy() for k in ("obs", "rewards", "masks"))
    T, N, M = rew.shape[:3]
    assert len(set(start["tstep"].tolist())) == 1
    ref = R.SimpleSpreadRef(start["agent_pos"], start["agent_vel"], start["landmark_pos"], env_T, tstep=int(start["tstep"][0]))
    np.testing.assert_allclose(obs[0], ref.obs(), rtol=1e-6, atol=1e-6)
    acts = buf["actions"].cpu().numpy().astype(np.int64).reshape(T, N, M)
    assert acts.min() >= 0 and acts.max() <= 4 and len(np.unique(acts)) > 1
    ended = 0
    for t in range(T):
        o_ref, r_ref, d_ref = ref.step(np.eye(5)[acts[t]], reset_states)
        ended += int(d_ref[:, 0].sum())
        np.testing.assert_allclose(obs[t + 1], o_ref, rtol=1e-6, atol=1e-6, err_msg=f"obs, step {t}")
        np.testing.assert_allclose(rew[t], r_ref, rtol=1e-6, atol=1e-6, err_msg=f"rewards, step {t}")
        np.testing.assert_array_equal(masks[t + 1, :, :, 0], 1.0 - d_ref, err_msg=f"masks, step {t}")
    return ended


@pytest.mark.gpu
@pytest.mark.parametrize("M,L,centralized,N,layer_N,relu,fnorm,env_T", CASES)
def test_episode_spread_launch_matches_stepwise(gpu_device, M, L, centralized, N, layer_N, relu, fnorm, env_T):
    runs, _ = _both_paths(M, L, centralized, N, layer_N, relu, fnorm, env_T)
    if env_T == 10:
        assert float(runs[1][0]["masks"][1:25].min()) == 0.0                       # a reset inside the launch
        assert int(runs[1][0]["env.tstep"].max()) == 5 and int(runs[1][1]["env.tstep"].max()) == 0      # 25 = 2 x 10 + 5; 50 = 5 x 10
    else:
        assert float(runs[1][0]["masks"][1:25].min()) == 1.0 and float(runs[1][0]["masks"][25].max()) == 0.0


SHAPE_CASES = [  # (M, L, centralized, N, layer_N, relu, feature norm, env episode length, T): shapes the 3 x 3 fixture does not reach
    (1, 1, True, 17, 1, True, True, 25, 6),       # S = 6; 16 environments per tile: one full tile and one single row
    (2, 5, True, 9, 0, False, False, 25, 6),      # S = 36, M < L
    (5, 2, False, 4, 1, False, True, 25, 6),      # G = 3: 4 environments leave a partial tile
    (7, 1, False, 3, 0, True, False, 25, 6),      # G = 2: 14 of 16 rows
    (8, 8, False, 3, 1, True, True, 25, 6),       # D = 48, G = 2: a full 16-row tile and a half one
    (6, 2, False, 5, 1, False, False, 3, 5),      # resets inside the launch; the second launch starts at tstep 2
]


@pytest.mark.gpu
@pytest.mark.parametrize("M,L,centralized,N,layer_N,relu,fnorm,env_T,T", SHAPE_CASES)
def test_episode_spread_other_shapes(gpu_device, M, L, centralized, N, layer_N, relu, fnorm, env_T, T):
    """What test_episode_spread_launch_matches_stepwise asserts (bit identity of the two paths) and what
    test_episode_spread_matches_oracle asserts (the recorded actions replayed through the oracle), at other M, L and tile fills.  The
    replay shares no code with mpe_step_env; an episode that ends takes the host Philox's reset draw, not the kernel's."""
    import mpe_spread_np as MS
    runs, start = _both_paths(M, L, centralized, N, layer_N, relu, fnorm, env_T, T=T)
    first, second = runs[1]
    D = 4 + 2 * L + 4 * (M - 1)
    assert tuple(first["obs"].shape) == (T + 1, N, M, D) and tuple(first["share_obs"].shape) == (T + 1, N, M, M * D if centralized else D)
    episode = start["episode"].copy()
    assert episode.tolist() == [1] * N and start["tstep"].tolist() == [0] * N                 # warmup's reset

    def reset_states(n):                                     # stream (seed 1, the environment's next episode number)
        episode[n] += 1
        pos, lpos = MS.reset_draws(1, int(episode[n]), n + 1, M, L)
        return pos[n], np.zeros((M, 2)), lpos[n]
    ended = _replay_through_oracle(first, start, env_T, reset_states)
    assert ended == N * (T // env_T)
    np.testing.assert_array_equal(first["env.episode"].cpu().numpy(), episode)
    assert first["env.tstep"].cpu().tolist() == [T % env_T] * N and second["env.tstep"].cpu().tolist() == [2 * T % env_T] * N
    if centralized:                                          # the environment's M observation rows side by side, once per agent
        side = first["obs"].reshape(T + 1, N, 1, M * D).expand(T + 1, N, M, M * D)
        assert torch.equal(first["share_obs"], side)
    else:
        assert torch.equal(first["share_obs"][1:], first["obs"][1:])


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
def test_episode_spread_path_is_taken_and_flag_turns_it_off(gpu_device):
    """The runner takes the one-launch episode when the env declares episode_state (and only then); --fuse_rollout_episode selects
    the stepwise loop on the same build; an env on the host-staging path keeps the stepwise loop."""
    from mappo_amd.envs.mpe_spread import SimpleSpreadVecEnv

    class HostSpread(SimpleSpreadVecEnv):
        """The same env behind the reference's NumPy vec-env contract: host arrays in and out."""
        graph_safe = accepts_device_actions = accepts_index_actions = False

        def reset(self):
            return super().reset().cpu().numpy()

        def step(self, actions_env):
            obs, rew, dones, infos = super().step(torch.as_tensor(np.asarray(actions_env, np.float32)))
            return obs.cpu().numpy(), rew.cpu().numpy(), dones.cpu().numpy(), infos

    names = ("rollout_episode_spread", "rollout_episode", "rollout_step", "mpe_spread_step")
    calls, restore = _counting(names)
    try:
        r, _ = _runner(True)
        r.rollout()
        assert calls == dict(rollout_episode_spread=1, rollout_episode=0, rollout_step=0, mpe_spread_step=0), calls
        r, _ = _runner(False)
        r.rollout()
        assert calls == dict(rollout_episode_spread=1, rollout_episode=0, rollout_step=26, mpe_spread_step=25), calls
        r, env = _runner(True, env_cls=HostSpread)
        assert r._staging is not None and hasattr(env, "episode_state")
        r.rollout()
        assert calls["rollout_episode_spread"] == 1 and calls["mpe_spread_step"] == 50 and calls["rollout_step"] >= 52, calls
    finally:
        restore()


@pytest.mark.gpu
@pytest.mark.parametrize("centralized", [True, False])
def test_episode_spread_graph_replay_matches_stepwise(gpu_device, centralized):
    """Runner level through the hipGraph path: eager episode, capture, then replays.  Both runners leave identical buffers and env
    states after every call, and each replayed episode sees new observations and a fresh sampling stream."""
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


@pytest.mark.gpu
@pytest.mark.parametrize("deterministic", [False, True])
def test_episode_spread_matches_oracle(gpu_device, deterministic):
    """Independent of the stepwise kernels: the actions the fused episode recorded, replayed through the NumPy oracle from the state
    saved before the launch, give the buffer's observations and rewards (1e-6: the fp32 cast of the outputs, the tolerance of
    test_mpe_env.py::test_kernel_matches_oracle_step_by_step).  deterministic=True covers the argmax path."""
    T, N, M = 25, 64, 3
    r, env = _runner(True, N=N)
    start = {n: getattr(env, n).cpu().numpy().copy() for n in ENV_NAMES}
    b = r.buffer
    if deterministic:
        nv = torch.empty(N * M, device=b.device)
        r.policy.collect_episode_env_fused(b, env.episode_state(), nv, True, deterministic=True)
    else:
        r.rollout()
    torch.cuda.synchronize()

    def reset_states(n):                                     # the oracle adopts the kernel's own reset draw (the last step's)
        return env.agent_pos[n].cpu().numpy(), env.agent_vel[n].cpu().numpy(), env.landmark_pos[n].cpu().numpy()
    assert _replay_through_oracle({k: getattr(b, k) for k in BUF_NAMES}, start, T, reset_states) == N
    assert int(env.tstep.max()) == 0 and int(env.episode.min()) == 2          # warmup's reset + the time-limit reset of step T - 1


def test_rollout_episode_spread_rejects_bad_arguments():
    """mappo_rollout_episode_spread validates its arguments on the host before any launch: error code + message, no GPU needed."""
    from mappo_amd import _lib
    lib = _lib.load()
    ND = _lib.NetDesc
    actor, critic = ND(18, 64, 5, 1, 1, 1, 0), ND(54, 64, 1, 1, 1, 1, 0)
    one = ctypes.c_void_p(16)                                # a non-null pointer that is never dereferenced: validation fails first

    def call(a, c, T=25, N=8, M=3, L=3, env_T=25, centralized=1, ptr=None):
        p = [ptr] * 15
        rc = lib.mappo_rollout_episode_spread(p[0], ctypes.byref(a) if a is not None else None, p[1],
                                              ctypes.byref(c) if c is not None else None, T, N, M, L, env_T, 1, p[2], p[3], p[4], p[5],
                                              p[6], 0, 1, 0, None, p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14], centralized, None)
        return rc, lib.mappo_last_error().decode()

    cases = [
        (dict(a=None, c=critic), "null desc"),
        (dict(a=ND(18, 64, 5, 1, 1, 1, 1), c=critic), "recurrent"),
        (dict(a=ND(128, 64, 5, 1, 1, 1, 0), c=ND(128, 64, 1, 1, 1, 1, 0), centralized=0), "narrow"),
        (dict(a=actor, c=ND(54, 64, 1, 2, 1, 1, 0)), "layer_N"),
        (dict(a=actor, c=ND(54, 64, 1, 1, 0, 1, 0)), "activation"),
        (dict(a=actor, c=ND(54, 64, 5, 1, 1, 1, 0)), "out_dim"),
        (dict(a=actor, c=critic, T=0), "bad shape"),
        (dict(a=actor, c=critic, N=0), "bad shape"),
        (dict(a=actor, c=critic, env_T=0), "bad shape"),
        (dict(a=actor, c=critic, M=0), "out of range"),
        (dict(a=actor, c=critic, M=9), "out of range"),
        (dict(a=actor, c=critic, L=9), "out of range"),
        (dict(a=ND(20, 64, 5, 1, 1, 1, 0), c=critic), "observation features"),
        (dict(a=ND(18, 64, 6, 1, 1, 1, 0), c=critic), "5 actions"),
        (dict(a=actor, c=ND(18, 64, 1, 1, 1, 1, 0)), "centralized"),
        (dict(a=actor, c=critic, centralized=0), "in_dim"),
        (dict(a=ND(24, 64, 5, 1, 1, 1, 0), c=ND(64, 64, 1, 1, 1, 1, 0), M=4, L=4), "centralized"),      # M * D = 96 does not fit
        (dict(a=actor, c=critic), "null pointer"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc == -1, (kw, rc)
        assert "rollout_episode_spread" in err and msg in err, (kw, err)
