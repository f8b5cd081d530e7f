"""MPE simple_speaker_listener without a GPU: the NumPy mirror (tests/mpe_comm_np.py) EQUALS the fixture stepped by the reference's
own environment (tests/golden/mpe_comm.npz), the fixture covers what it claims, the vec-env and the C ABI refuse by name what they
are not built for, and the inputs of the GPU rollout comparison (tests/test_gpu_comm_runner.py) keep clear of decision boundaries."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
import mpe_comm_np as MC


def _fx():
    g = golden("mpe_comm")
    return {k: g[k] for k in g.files}


def test_fixture_covers_what_it_claims():
    g = _fx()
    E, T = g["actions"].shape[:2]
    assert (E, T) == (12, 6)
    assert sorted(np.unique(g["goal"])) == [0, 1, 2]
    assert sorted(np.unique(g["actions"][..., 0])) == [0, 1, 2] and sorted(np.unique(g["actions"][..., 1])) == [0, 1, 2, 3, 4]
    assert g["dones"][:, :-1].sum() == 0 and g["dones"][:, -1].all()
    # the listener hears the symbol said in the same step; after a reset it hears nothing
    np.testing.assert_array_equal(g["obs_listener"][..., 8:], np.eye(3)[g["actions"][..., 0]])
    np.testing.assert_array_equal(g["obs0_listener"][:, 8:], 0.0)
    np.testing.assert_array_equal(g["obs0_listener"][:, :2], 0.0)
    assert g["obs0_speaker"].shape == (E, 3) and g["obs_listener"].shape == (E, T, 11)
    # the speaker never moves
    np.testing.assert_array_equal(g["pos0"][:, 0], g["pos1"][:, 0])
    np.testing.assert_array_equal(g["vel1"][:, 0], 0.0)


def test_numpy_mirror_equals_reference():
    g = _fx()
    env = MC.SimpleSpeakerListenerNp(g["pos0"][:, 1], g["vel0"][:, 1], g["lpos"], g["goal"], episode_length=6)
    os0, ol0 = env.obs()
    np.testing.assert_array_equal(os0, g["obs0_speaker"])
    np.testing.assert_array_equal(ol0, g["obs0_listener"])
    for t in range(6):
        a = g["actions"][:, t]
        os_, ol, rew, dones = env.step(np.eye(3)[a[:, 0]], np.eye(5)[a[:, 1]])
        np.testing.assert_array_equal(os_, g["obs_speaker"][:, t], err_msg=f"speaker obs, step {t}")
        np.testing.assert_array_equal(ol, g["obs_listener"][:, t], err_msg=f"listener obs, step {t}")
        np.testing.assert_array_equal(rew, g["rewards"][:, t], err_msg=f"rewards, step {t}")
        np.testing.assert_array_equal(dones, g["dones"][:, t])
    np.testing.assert_array_equal(env.pos, g["pos1"][:, 1])
    np.testing.assert_array_equal(env.vel, g["vel1"][:, 1])
    # collaborative: each agent gets twice the listener's own term
    d = g["pos1"][:, 1] - g["lpos"][np.arange(12), g["goal"]]
    np.testing.assert_array_equal(g["rewards"][:, -1, 0], 2 * -(np.square(d)[:, 0] + np.square(d)[:, 1]))


def test_vec_env_refuses_other_shapes_by_name_without_a_device():
    from mappo_amd.envs import SimpleSpeakerListenerVecEnv
    with pytest.raises(ValueError, match="num_agents = 2"):
        SimpleSpeakerListenerVecEnv(4, num_agents=3, device="cuda:7")
    with pytest.raises(ValueError, match="num_landmarks = 3"):
        SimpleSpeakerListenerVecEnv(4, num_landmarks=2, device="cuda:7")
    env = SimpleSpeakerListenerVecEnv(4, device="cpu")
    assert env.observation_space == [[3], [11]] and env.share_observation_space == [[14], [14]]
    assert [s.__class__.__name__ for s in env.action_space] == ["Discrete", "Discrete"] and [s.n for s in env.action_space] == [3, 5]
    assert env.graph_safe and env.accepts_device_actions and env.accepts_index_actions and env.consumes_actions and env.ragged_obs
    assert len(env._out) == 2
    st = env.episode_state_comm()
    assert st["scenario"] == "simple_speaker_listener" and tuple(st["listener_pos"].shape) == (4, 2) and tuple(st["goal"].shape) == (4,)
    assert int(st["symbol"].min()) == -1
    import torch
    for bad in (torch.zeros(4, 3), [torch.zeros(4, 3)], [torch.zeros(4, 5), torch.zeros(4, 3)], [torch.zeros(3), torch.zeros(3)]):
        with pytest.raises(ValueError, match=r"SimpleSpeakerListenerVecEnv.step: .*\[N, 3\].*\[N, 5\].*\[N, 2\]"):
            env.step(bad)
    with pytest.raises(ValueError, match="landmark indices"):
        env.set_state(np.zeros((4, 2)), np.zeros((4, 2)), np.zeros((4, 3, 2)), np.full(4, 3))


# ---- the C ABI refuses what the kernels are not built for, before any launch -------------------------------------------------------
P = C.c_void_p(4096)                          # never dereferenced: the checks come before any launch


def test_mpe_comm_reset_and_step_reject():
    from mappo_amd import _lib
    lib = _lib.load()
    assert lib.mappo_abi_version() >= 6

    def reset(N=4, ptr=P):
        return lib.mappo_mpe_comm_reset(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, 1, None), lib.mappo_last_error().decode()

    def step(N=4, mode=1, env_T=6, ptr=P):
        return (lib.mappo_mpe_comm_step(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, mode, ptr, ptr, ptr, ptr, N, env_T, 1, None),
                lib.mappo_last_error().decode())

    for call, who, cases in ((reset, "mpe_comm_reset", [(dict(N=0), ["N=0", "N >= 1"]), (dict(ptr=None), ["null pointer"])]),
                             (step, "mpe_comm_step", [(dict(N=0), ["N=0", "N >= 1"]), (dict(mode=2), ["action_mode 2"]),
                                                      (dict(mode=-1), ["action_mode -1"]), (dict(env_T=0), ["episode length 0"]),
                                                      (dict(ptr=None), ["null pointer"]), (dict(ptr=None, mode=0), ["null pointer"])])):
        for kw, words in cases:
            rc, err = call(**kw)
            assert rc == -1, (who, kw, rc)
            assert who in err, err
            for w in words:
                assert w in err, (who, kw, err)


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


def _episode(sa=None, sc=None, la=None, lc=None, T=6, N=8, env_T=6, centralized=1, ptr=P, state=P, null_agent=False):
    from mappo_amd import _lib
    lib = _lib.load()
    sp = _agent(sa or _desc(3, 3), sc or _desc(14 if centralized else 3, 1), ptr)
    li = _agent(la or _desc(11, 5), lc or _desc(14 if centralized else 11, 1), ptr)
    rc = lib.mappo_rollout_episode_comm(None if null_agent else C.byref(sp), C.byref(li), T, N, env_T, 1, state, state, state, state, state,
                                        state, state, 0, 0, centralized, None)
    return rc, lib.mappo_last_error().decode()


EPISODE_BAD = [
    ("N=0", dict(N=0), ["N=0", ">= 1"]),
    ("T=0", dict(T=0), ["T=0", ">= 1"]),
    ("env_T=0", dict(env_T=0), ["episode length 0"]),
    ("null agent", dict(null_agent=True), ["null agent descriptor"]),
    ("null buffer pointer", dict(ptr=None), ["null pointer", "speaker"]),
    ("null state pointer", dict(state=None), ["null state pointer"]),
    ("recurrent", dict(sa=_desc(3, 3, recurrent=1)), ["speaker", "recurrent"]),
    ("recurrent listener critic", dict(lc=_desc(14, 1, recurrent=1)), ["listener", "recurrent"]),
    ("layer_N 2", dict(sa=_desc(3, 3, layer_N=2), sc=_desc(14, 1, layer_N=2), la=_desc(11, 5, layer_N=2), lc=_desc(14, 1, layer_N=2)),
     ["layer_N 2", "layer_N <= 1"]),
    ("speaker in_dim 4", dict(sa=_desc(4, 3)), ["speaker actor in_dim 4", "in_dim 3"]),
    ("listener out_dim 3", dict(la=_desc(11, 3)), ["listener actor in_dim 11 / out_dim 3", "5 actions"]),
    ("critic 13 centralized", dict(sc=_desc(13, 1)), ["centralized", "14", "got 13"]),
    ("critic 14 decentralized", dict(centralized=0, lc=_desc(14, 1)), ["listener critic in_dim 14", "11"]),
    ("critic out_dim", dict(lc=_desc(14, 2)), ["critic out_dim"]),
    ("layer_N differs", dict(lc=_desc(14, 1, layer_N=0)), ["share layer_N"]),
    ("activation differs", dict(la=_desc(11, 5, relu=0)), ["activation"]),
]


@pytest.mark.parametrize("name,kw,words", EPISODE_BAD, ids=[b[0] for b in EPISODE_BAD])
def test_rollout_episode_comm_rejects(name, kw, words):
    rc, err = _episode(**kw)
    assert rc == -1, (name, rc)
    assert "rollout_episode_comm" in err, err
    for w in words:
        assert w in err, (name, err)


# ---- the inputs of the float64 rollout comparison (tests/test_gpu_comm_runner.py) keep clear of decision boundaries ----------------
def test_comm_rollout_inputs_stay_under_the_exclusion_cap():
    """On the reference side alone (oracle networks in float64 / float32, host Philox, the NumPy mirror): over the T = 4 steps of
    N = 5 environments, per agent, at most 2 % of the rows sit within the exclusion margin of tests/rollout_ref.py."""
    import comm_rollout_ref as CR
    ref = CR.reference_rollout()
    for m in range(2):
        near = np.concatenate([e.near for e in ref["expected"][m]])
        assert near.mean() <= CR.NEAR_CAP, f"agent {m}: {near.sum()} of {near.size} rows near a boundary"
        assert sorted(np.unique(np.concatenate(ref["actions"][m]))) != [0], "an agent that only ever takes action 0 tests nothing"
