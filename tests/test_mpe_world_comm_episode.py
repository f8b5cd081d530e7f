"""CPU side of the one-launch rollout episode on MPE simple_world_comm (mappo_rollout_episode_world_comm): the entry point is exported
and declared, the host refuses what the kernel is not built for by name and before any launch, ops refuses another number of agents
without a device, and the env declares the opt-in path."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(64)                        # a non-null pointer nobody dereferences: every call below is refused on the host
OBS_DIMS, ACT_DIMS = (34, 34, 34, 34, 28, 28), (9, 5, 5, 5, 5, 5)


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


def _episode(actors=None, critics=None, T=6, N=8, env_T=6, centralized=1, ptr=P, state=P, null_agents=False):
    """actors / critics: {agent: descriptor} replacing the valid ones."""
    from mappo_amd import _lib
    lib = _lib.load()
    ags = []
    for m, (D, A) in enumerate(zip(OBS_DIMS, ACT_DIMS)):
        a = (actors or {}).get(m) or _desc(D, A)
        c = (critics or {}).get(m) or _desc(192 if centralized else D, 1)
        ags.append(_agent(a, c, ptr))
    arr = (_lib.CommAgent * 6)(*ags)
    rc = lib.mappo_rollout_episode_world_comm(None if null_agents else arr, state, state, state, state, state, T, N, env_T, 1, 0, 0, centralized,
                                              None)
    return rc, lib.mappo_last_error().decode()


def _all(layer_N):
    return dict(actors={m: _desc(D, A, layer_N=layer_N) for m, (D, A) in enumerate(zip(OBS_DIMS, ACT_DIMS))},
                critics={m: _desc(192, 1, layer_N=layer_N) for m in range(6)})


EPISODE_BAD = [
    ("N=0", dict(N=0), ["N=0", ">= 1"]),
    ("T=0", dict(T=0), ["T=0", ">= 1"]),
    ("env_T=0", dict(env_T=0), ["episode length 0"]),
    ("null agents", dict(null_agents=True), ["null agent descriptors", "num_agents = 6"]),
    ("null buffer pointer", dict(ptr=None), ["null pointer", "leader"]),
    ("null state pointer", dict(state=None), ["null state pointer"]),
    ("recurrent leader actor", dict(actors={0: _desc(34, 9, recurrent=1)}), ["leader", "recurrent"]),
    ("recurrent good critic", dict(critics={5: _desc(192, 1, recurrent=1)}), ["good agent 5", "recurrent"]),
    ("layer_N 2", _all(2), ["layer_N 2", "layer_N <= 1"]),
    ("leader out_dim 5", dict(actors={0: _desc(34, 5)}), ["leader actor in_dim 34 / out_dim 5", "9 actions"]),
    ("adversary in_dim 28", dict(actors={3: _desc(28, 5)}), ["adversary 3 actor in_dim 28", "in_dim 34"]),
    ("good agent in_dim 34", dict(actors={4: _desc(34, 5)}), ["good agent 4 actor in_dim 34", "in_dim 28"]),
    ("adversary out_dim 9", dict(actors={1: _desc(34, 9)}), ["adversary 1 actor in_dim 34 / out_dim 9", "5 actions"]),
    ("critic 191 centralized", dict(critics={0: _desc(191, 1)}), ["centralized", "192", "got 191"]),
    ("critic 192 decentralized", dict(centralized=0, critics={4: _desc(192, 1)}), ["good agent 4 critic in_dim 192", "28"]),
    ("critic out_dim", dict(critics={1: _desc(192, 2)}), ["critic out_dim"]),
    ("layer_N differs", dict(critics={2: _desc(192, 1, layer_N=0)}), ["share layer_N", "12 networks"]),
    ("activation differs", dict(actors={1: _desc(34, 5, relu=0)}), ["activation"]),
]


@pytest.mark.parametrize("name,kw,words", EPISODE_BAD, ids=[b[0] for b in EPISODE_BAD])
def test_rollout_episode_world_comm_rejects(name, kw, words):
    rc, err = _episode(**kw)
    assert rc == -1, (name, rc)
    assert "rollout_episode_world_comm" in err, err
    for w in words:
        assert w in err, (name, err)


def test_ops_refuses_another_number_of_episode_agents():
    from mappo_amd import ops
    for k in (5, 7):
        with pytest.raises(ValueError, match="rollout_episode_world_comm: simple_world_comm is built for num_agents = 6"):
            ops.rollout_episode_world_comm([None] * k, 4, 4, 4, 1, *[None] * 5, False, 0, True)


def test_entry_point_is_exported_and_declared():
    from mappo_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "mappo_rollout_episode_world_comm")
    with open(os.path.join(ROOT, "include", "mappo_hip.h")) as f:
        assert "int mappo_rollout_episode_world_comm(const mappo_comm_agent *agents" in f.read()


def test_env_declares_the_opt_in_episode(monkeypatch):
    from mappo_amd.envs import SimpleWorldCommVecEnv as E
    assert hasattr(E, "episode_launch") and E.episode_flag == "MAPPO_WORLD_COMM_EPISODE" and E.episode_default == "0"
    assert E.episode_critics_after is True
    env = E(4, device="cpu")
    for flag, has in ((None, False), ("0", False), ("1", True)):    # opt-in: an env of a run that did not ask has no such attribute
        monkeypatch.delenv(E.episode_flag, raising=False) if flag is None else monkeypatch.setenv(E.episode_flag, flag)
        assert hasattr(env, "episode_launch") == has, flag
    assert callable(env.episode_launch)


def test_reference_rollout_stays_under_the_exclusion_cap():
    """On the reference side alone (oracle networks in float64 / float32, host Philox, the NumPy mirror) from the start states and
    seeds the GPU test uses: at most 2 % of the (row, agent) pairs sit within the exclusion margin of tests/rollout_ref.py."""
    import numpy as np
    import world_comm_rollout_ref as WR
    ref = WR.reference_rollout()
    near = np.concatenate([x for m in range(6) for x in ref["near"][m]])
    assert near.size == WR.REF_N * WR.REF_T * 6
    assert near.mean() <= WR.NEAR_CAP, f"{near.sum()} of {near.size} (row, agent) pairs near a boundary"
    for m in range(6):
        a = np.concatenate(ref["actions"][m])
        for k in range(a.shape[1]):
            assert len(np.unique(a[:, k])) > 1, "a head that only ever takes one action tests nothing"
