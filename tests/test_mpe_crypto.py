"""MPE simple_crypto without a GPU: the NumPy mirror (tests/mpe_crypto_np.py) EQUALS the fixture stepped by the reference's own
environment (tests/golden/mpe_crypto.npz) — the reset-on-done boundary of the 7-step runs included —, the reward's zero-c branch
gives the values worked out by hand, the vec-env, the ops and the C ABI refuse by name what they are not built for, and the inputs of
the GPU sampling comparison (tests/test_gpu_mpe_crypto.py) keep clear of decision boundaries."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
import mpe_crypto_np as MC

OBS = ("eve", "bob", "alice")


def _fx(tag):
    g = golden("mpe_crypto")
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}


def test_fixture_covers_what_it_claims():
    lo, sh = _fx("long"), _fx("short")
    assert lo["actions"].shape == (24, 25, 3) and sh["actions"].shape == (2, 14, 3)
    assert lo["num_landmarks"].tolist() == [2] * 12 + [4] * 12 and sh["num_landmarks"].tolist() == [2, 4]
    for m in range(3):
        assert sorted(np.unique(lo["actions"][..., m])) == [0, 1, 2, 3]
    for k in ("goal", "key"):
        assert sorted(np.unique(lo[k][:12])) == [0, 1] and sorted(np.unique(lo[k][12:])) == [0, 1, 2, 3]
    assert (lo["goal"] == lo["key"]).any() and (lo["goal"] != lo["key"]).any()
    assert lo["dones"][:, :-1].sum() == 0 and lo["dones"][:, -1].all()
    assert sh["dones"][:, [6, 13]].all() and sh["dones"].sum() == 2 * 2 * 3
    assert lo["obs_eve"].shape == (24, 25, 4) and lo["obs_bob"].shape == (24, 25, 8) and lo["obs_alice"].shape == (24, 25, 8)
    assert lo["rewards"].shape == (24, 25, 3) and lo["rewards"].dtype == np.float64
    # per-agent rewards: Bob and Alice share one, Eve has her own; all of -2, 0, 2 occur for the good agents, -2 and 0 for Eve
    np.testing.assert_array_equal(lo["rewards"][..., 1], lo["rewards"][..., 2])
    assert sorted(np.unique(lo["rewards"][..., 1])) == [-2, 0, 2] and sorted(np.unique(lo["rewards"][..., 0])) == [-2, 0]
    assert (lo["rewards"][..., 0] != lo["rewards"][..., 1]).any()
    # after a reset nobody has spoken: Eve sees zeros, Bob e_key | 0, Alice e_goal | e_key
    np.testing.assert_array_equal(lo["obs0_eve"], 0.0)
    np.testing.assert_array_equal(lo["obs0_bob"], np.concatenate([np.eye(4)[lo["key"]], np.zeros((24, 4))], axis=1))
    np.testing.assert_array_equal(lo["obs0_alice"], np.concatenate([np.eye(4)[lo["goal"]], np.eye(4)[lo["key"]]], axis=1))


@pytest.mark.parametrize("onehot", [True, False], ids=["onehot", "index"])
def test_numpy_mirror_equals_reference_long_episodes(onehot):
    g = _fx("long")
    env = MC.SimpleCryptoNp(g["goal"], g["key"], episode_length=25)
    for m, o in enumerate(env.obs()):
        np.testing.assert_array_equal(o, g["obs0_" + OBS[m]])
    for t in range(25):
        a = g["actions"][:, t]
        obs, rew, dones = env.step(np.eye(4)[a] if onehot else a)
        for m in range(3):
            np.testing.assert_array_equal(obs[m], g["obs_" + OBS[m]][:, t], err_msg=f"obs of agent {m}, step {t}")
        np.testing.assert_array_equal(rew, g["rewards"][:, t], err_msg=f"rewards, step {t}")
        np.testing.assert_array_equal(dones, g["dones"][:, t])
    np.testing.assert_array_equal(env.comm, g["actions"][:, -1])


def test_numpy_mirror_equals_reference_across_reset_on_done():
    """episode_length 7, 14 steps: the steps that end an episode return the reset's observations (goal and key reloaded from the
    fixture, nothing said) and the ended step's rewards; the next episode continues from the reloaded state."""
    g = _fx("short")
    env = MC.SimpleCryptoNp(g["goal"], g["key"], episode_length=7)
    resets = 0
    for t in range(14):
        obs, rew, dones = env.step(g["actions"][:, t])
        np.testing.assert_array_equal(dones, g["dones"][:, t])
        np.testing.assert_array_equal(rew, g["rewards"][:, t], err_msg=f"rewards, step {t}")
        if dones.all():
            env.reload(np.arange(2), g["reset_goal"][:, resets], g["reset_key"][:, resets])
            obs = env.obs()
            resets += 1
        else:
            assert not dones.any()
        for m in range(3):
            np.testing.assert_array_equal(obs[m], g["obs_" + OBS[m]][:, t], err_msg=f"obs of agent {m}, step {t}")
    assert resets == 2


def test_reward_skips_an_agent_that_has_said_nothing():
    """scenarios/simple_crypto.py:104,109,119: an agent whose c is the zero vector (-1 here) adds nothing.  goal = 1 throughout;
    rows: (Eve, Bob) = (silent, silent), (silent, right), (silent, wrong), (right, silent), (wrong, silent), (wrong, right),
    (right, wrong), (wrong, wrong).  Alice's own symbol never enters a reward."""
    comm = np.array([[-1, -1, 0], [-1, 1, -1], [-1, 3, 1], [1, -1, 2], [0, -1, 3], [2, 1, -1], [1, 0, 0], [3, 2, 1]])
    want = np.array([[0, 0, 0], [0, 0, 0], [0, -2, -2], [0, 0, 0], [-2, 2, 2], [-2, 2, 2], [0, -2, -2], [-2, 0, 0]], np.float64)
    got = MC.rewards(np.full(8, 1), comm)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, want)
    # and the observations of a silent speaker are zeros where her symbol would stand
    o = MC.observation(np.array([1]), np.array([0]), np.array([[-1, -1, -1]]))
    np.testing.assert_array_equal(o[0], [[0, 0, 0, 0]])
    np.testing.assert_array_equal(o[1], [[1, 0, 0, 0, 0, 0, 0, 0]])
    np.testing.assert_array_equal(o[2], [[0, 1, 0, 0, 1, 0, 0, 0]])


def test_vec_env_refuses_other_shapes_by_name_without_a_device():
    import torch
    from mappo_amd.envs import SimpleCryptoVecEnv
    for n in (2, 4):
        with pytest.raises(ValueError, match=rf"num_agents = 3.*got num_agents {n}, num_landmarks 2"):
            SimpleCryptoVecEnv(4, num_agents=n, device="cuda:7")
    for L in (1, 5):
        with pytest.raises(ValueError, match=rf"num_landmarks = 2, 3 or 4.*got num_agents 3, num_landmarks {L}"):
            SimpleCryptoVecEnv(4, num_landmarks=L, device="cuda:7")
    env = SimpleCryptoVecEnv(4, device="cpu")
    assert env.observation_space == [[4], [8], [8]] and env.share_observation_space == [[20], [20], [20]]
    assert [s.__class__.__name__ for s in env.action_space] == ["Discrete"] * 3 and [s.n for s in env.action_space] == [4, 4, 4]
    assert env.graph_safe and env.accepts_device_actions and env.accepts_index_actions and env.consumes_actions and env.ragged_obs
    assert env.episode_flag == "MAPPO_CRYPTO_EPISODE" and (env.M, env.L) == (3, 2) and SimpleCryptoVecEnv(4, num_landmarks=4, device="cpu").L == 4
    st = env.state_tensors()
    assert set(st) == {"goal", "key", "comm", "tstep", "episode"} and tuple(st["comm"].shape) == (4, 3) and st["comm"].dtype == torch.int32
    assert tuple(st["goal"].shape) == (4,) and tuple(st["key"].shape) == (4,) and st["episode"].dtype == torch.int64
    assert st["comm"].tolist() == [[-1] * 3] * 4                   # nothing said before the first reset either
    for bad in (torch.zeros(4, 4), [torch.zeros(4, 4)] * 2, [torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4, 5)], torch.zeros(3, 3),
                torch.zeros(4, 3, 5)):
        with pytest.raises(ValueError, match=r"SimpleCryptoVecEnv.step: .*\[N, 4\].*\[N, 3, 4\].*\[N, 3\]"):
            env.step(bad)


def test_set_state_checks_its_ranges():
    from mappo_amd.envs import SimpleCryptoVecEnv
    env = SimpleCryptoVecEnv(4, num_landmarks=3, device="cpu")
    env.set_state([0, 1, 2, 2], [2, 2, 0, 1], [[-1, 0, 3]] * 4, tstep=5)
    assert env.goal.tolist() == [0, 1, 2, 2] and env.key.tolist() == [2, 2, 0, 1] and env.comm.tolist() == [[-1, 0, 3]] * 4
    assert env.tstep.tolist() == [5] * 4
    env.set_state(np.zeros(4), np.zeros(4))                        # comm defaults to nothing said
    assert env.comm.tolist() == [[-1] * 3] * 4 and env.tstep.tolist() == [0] * 4
    ok = np.zeros(4)
    with pytest.raises(ValueError, match=r"goal must be landmark indices 0 \.\. 2"):
        env.set_state(np.full(4, 3), ok)
    with pytest.raises(ValueError, match=r"goal must be landmark indices 0 \.\. 2"):
        env.set_state(np.array([0, -1, 0, 0]), ok)
    with pytest.raises(ValueError, match=r"key must be landmark indices 0 \.\. 2"):
        env.set_state(ok, np.full(4, 3))
    with pytest.raises(ValueError, match=r"comm must be symbols 0 \.\. 3, or -1"):
        env.set_state(ok, ok, np.full((4, 3), 4))
    with pytest.raises(ValueError, match=r"comm must be symbols 0 \.\. 3, or -1"):
        env.set_state(ok, ok, np.full((4, 3), -2))
    assert env.comm.tolist() == [[-1] * 3] * 4                     # a refused state is not loaded


# ---- the C ABI refuses what the kernels are not built for, before any launch -------------------------------------------------------
P = C.c_void_p(4096)                          # never dereferenced: the checks come before any launch


def test_mpe_crypto_reset_and_step_reject():
    from mappo_amd import _lib
    lib = _lib.load()
    assert lib.mappo_abi_version() >= 11

    def reset(N=4, M=3, L=2, ptr=P):
        return lib.mappo_mpe_crypto_reset(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, M, L, 1, None), lib.mappo_last_error().decode()

    def step(N=4, M=3, L=2, mode=1, env_T=6, ptr=P):
        return (lib.mappo_mpe_crypto_step(ptr, ptr, ptr, ptr, ptr, ptr, mode, ptr, ptr, ptr, ptr, ptr, N, M, L, env_T, 1, None),
                lib.mappo_last_error().decode())

    common = [(dict(N=0), ["N=0", "N >= 1"]), (dict(M=2), ["num_agents=2", "num_agents = 3"]), (dict(M=4), ["num_agents=4", "num_agents = 3"]),
              (dict(L=1), ["num_landmarks=1", "num_landmarks = 2, 3 or 4"]), (dict(L=5), ["num_landmarks=5", "num_landmarks = 2, 3 or 4"]),
              (dict(ptr=None), ["null pointer"])]
    for call, who, cases in ((reset, "mpe_crypto_reset", common),
                             (step, "mpe_crypto_step", common + [(dict(mode=2), ["action_mode 2"]), (dict(mode=-1), ["action_mode -1"]),
                                                                 (dict(env_T=0), ["episode length 0"])])):
        for kw, words in cases:
            rc, err = call(**kw)
            assert rc == -1, (who, kw, rc)
            assert who in err, err
            for w in words:
                assert w in err, (who, kw, err)


def test_ops_refuse_other_shapes_before_touching_a_tensor():
    from mappo_amd import ops
    for n in (2, 4):
        with pytest.raises(ValueError, match=rf"mpe_crypto_reset: .*num_agents = 3.*got {n}"):
            ops.mpe_crypto_reset(*[None] * 8, 4, 1, num_agents=n)
        with pytest.raises(ValueError, match=rf"mpe_crypto_step: .*num_agents = 3.*got {n}"):
            ops.mpe_crypto_step(*[None] * 6, 1, *[None] * 5, 4, 25, 1, num_agents=n)
    for L in (1, 5):
        with pytest.raises(ValueError, match=rf"mpe_crypto_reset: .*num_landmarks = 2, 3 or 4.*got {L}"):
            ops.mpe_crypto_reset(*[None] * 8, 4, 1, num_landmarks=L)
        with pytest.raises(ValueError, match=rf"mpe_crypto_step: .*num_landmarks = 2, 3 or 4.*got {L}"):
            ops.mpe_crypto_step(*[None] * 6, 1, *[None] * 5, 4, 25, 1, num_landmarks=L)
        with pytest.raises(ValueError, match=rf"rollout_episode_crypto: .*num_landmarks = 2, 3 or 4.*got {L}"):
            ops.rollout_episode_crypto([_agent(_desc(4, 4), _desc(20, 1))] * 3, 4, 4, 4, 1, *[None] * 5, False, 0, True, num_landmarks=L)


def test_ops_refuses_another_number_of_agents():
    from mappo_amd import ops
    for n in (2, 4):
        with pytest.raises(ValueError, match=rf"rollout_episode_crypto: simple_crypto is built for num_agents = 3 \(got {n} agents\)"):
            ops.rollout_episode_crypto([None] * n, 4, 4, 4, 1, *[None] * 5, False, 0, True)


def _desc(in_dim, out_dim, layer_N=1, recurrent=0, relu=1):
    from mappo_amd import _lib
    return _lib.NetDesc(in_dim, 64, out_dim, layer_N, relu, 1, recurrent)


def _agent(actor, critic, ptr=P):
    from mappo_amd import _lib
    ag = _lib.CommAgent()
    ag.actor_desc, ag.critic_desc, ag.seed = actor, critic, 1
    v = ptr.value if ptr is not None else None
    for f in ("actor_params", "critic_params", "obs_buf", "share_buf", "rew_buf", "mask_buf", "actions", "logp", "values", "next_values"):
        setattr(ag, f, v)
    return ag


def _episode(actors=None, critics=None, T=6, N=8, L=2, env_T=6, centralized=1, ptr=P, state=P, null_agents=False):
    """actors / critics: {agent: descriptor} replacing the valid ones."""
    from mappo_amd import _lib
    lib = _lib.load()
    ags = []
    for m, D in enumerate(MC.OBS_DIMS):
        a = (actors or {}).get(m) or _desc(D, 4)
        c = (critics or {}).get(m) or _desc(20 if centralized else D, 1)
        ags.append(_agent(a, c, ptr))
    arr = (_lib.CommAgent * 3)(*ags)
    rc = lib.mappo_rollout_episode_crypto(None if null_agents else arr, state, state, state, state, state, T, N, L, env_T, 1, 0, 0,
                                          centralized, None)
    return rc, lib.mappo_last_error().decode()


def _all(layer_N):
    return dict(actors={m: _desc(D, 4, layer_N=layer_N) for m, D in enumerate(MC.OBS_DIMS)}, critics={m: _desc(20, 1, layer_N=layer_N) for m in range(3)})


EPISODE_BAD = [
    ("N=0", dict(N=0), ["N=0", ">= 1"]),
    ("T=0", dict(T=0), ["T=0", ">= 1"]),
    ("env_T=0", dict(env_T=0), ["episode length 0"]),
    ("L=1", dict(L=1), ["num_landmarks=1", "num_landmarks = 2, 3 or 4"]),
    ("L=5", dict(L=5), ["num_landmarks=5", "num_landmarks = 2, 3 or 4"]),
    ("null agents", dict(null_agents=True), ["null agent descriptors", "num_agents = 3"]),
    ("null buffer pointer", dict(ptr=None), ["null pointer", "Eve"]),
    ("null state pointer", dict(state=None), ["null state pointer"]),
    ("recurrent Eve actor", dict(actors={0: _desc(4, 4, recurrent=1)}), ["Eve", "recurrent"]),
    ("recurrent Alice critic", dict(critics={2: _desc(20, 1, recurrent=1)}), ["Alice", "recurrent"]),
    ("layer_N 2", _all(2), ["layer_N 2", "layer_N <= 1"]),
    ("Eve in_dim 8", dict(actors={0: _desc(8, 4)}), ["Eve actor in_dim 8", "in_dim 4"]),
    ("Bob in_dim 4", dict(actors={1: _desc(4, 4)}), ["Bob actor in_dim 4", "in_dim 8"]),
    ("Alice out_dim 5", dict(actors={2: _desc(8, 5)}), ["Alice actor in_dim 8 / out_dim 5", "4 actions"]),
    ("critic 28 centralized", dict(critics={0: _desc(28, 1)}), ["centralized", "4 + 8 + 8 = 20", "got 28"]),
    ("critic 20 decentralized", dict(centralized=0, critics={1: _desc(20, 1)}), ["Bob critic in_dim 20", "8"]),
    ("critic out_dim", dict(critics={1: _desc(20, 2)}), ["critic out_dim"]),
    ("layer_N differs", dict(critics={2: _desc(20, 1, layer_N=0)}), ["share layer_N"]),
    ("activation differs", dict(actors={1: _desc(8, 4, relu=0)}), ["activation"]),
]


@pytest.mark.parametrize("name,kw,words", EPISODE_BAD, ids=[b[0] for b in EPISODE_BAD])
def test_rollout_episode_crypto_rejects(name, kw, words):
    rc, err = _episode(**kw)
    assert rc == -1, (name, rc)
    assert "rollout_episode_crypto" in err, err
    for w in words:
        assert w in err, (name, err)


def test_host_reset_draws_follow_the_index_rule():
    """The host restatement of the reset draws (what the GPU reset is held against): in range for every L, every index, goal and
    key independent (equal somewhere, different somewhere), another stream per episode."""
    for L in (2, 3, 4):
        goal, key = MC.reset_draws(7, 1, 4096, L)
        assert goal.shape == (4096,) and sorted(np.unique(goal)) == list(range(L)) and sorted(np.unique(key)) == list(range(L))
        assert 0 < int((goal == key).sum()) < 4096
        g2, k2 = MC.reset_draws(7, 2, 4096, L)
        assert not np.array_equal(goal, g2) and not np.array_equal(key, k2)


# ---- the inputs of the float64 sampling comparison (tests/test_gpu_mpe_crypto.py) keep clear of decision boundaries ----------------
def test_crypto_rollout_inputs_stay_under_the_exclusion_cap():
    """On the reference side alone (oracle networks in float64 / float32, host Philox, the NumPy mirror): over the T steps of N
    environments, at most 2 % of the (row, agent) pairs sit within the exclusion margin of tests/rollout_ref.py."""
    import crypto_rollout_ref as CR
    ref = CR.reference_rollout()
    near = np.concatenate([e.near for m in range(3) for e in ref["expected"][m]])
    assert near.mean() <= CR.NEAR_CAP, f"{near.sum()} of {near.size} (row, agent) pairs near a boundary"
    for m in range(3):
        assert len(np.unique(np.concatenate(ref["actions"][m]))) > 1, "an agent that only ever takes one action tests nothing"
