"""MPE parity, pinned: tests/golden/mpe_envs.npz holds episodes stepped by the reference's own `simple_reference` and
`simple_spread` environments (tests/golden/generate_golden_mpe.py).  Here, without a GPU: the NumPy restatements that the GPU tests
are held against reproduce those episodes (simple_reference exactly — adds and multiplies only, in the reference's order;
simple_spread to 1e-12, measured 1.8e-15: the contact force goes through logaddexp, whose libm may differ), and the new entry points
refuse bad arguments before any launch with a message that names the limit."""
import ctypes as C

import numpy as np
import pytest

import mpe_ref_np
from conftest import golden, sub


@pytest.fixture(scope="module")
def fx():
    g = golden("mpe_envs")
    return sub(g, "ref"), sub(g, "spread")


def test_fixture_shapes(fx):
    ref, spread = fx
    E, T = 12, 6
    assert ref["obs"].shape == (E, T, 2, 21) and ref["obs"].dtype == np.float64 and ref["actions"].shape == (E, T, 2, 2)
    assert ref["goals"].shape == (E, 2) and set(np.unique(ref["goals"])) == {0, 1, 2}
    assert spread["obs"].shape == (E, T, 3, 18) and spread["actions"].shape == (E, T, 3)
    assert not ref["dones"][:, :-1].any() and ref["dones"][:, -1].all() and spread["dones"][:, -1].all()
    d01 = np.linalg.norm(spread["pos0"][:, 0] - spread["pos0"][:, 1], axis=-1)
    assert (d01 < 0.3).sum() == E // 2                                  # half of the spread episodes start in contact


def test_numpy_restatement_equals_the_reference_simple_reference(fx):
    """Float64 equality on obs, rewards, dones and the final state, every step of every episode."""
    ref, _ = fx
    E, T = ref["obs"].shape[:2]
    env = mpe_ref_np.SimpleReferenceNp(ref["pos0"], ref["vel0"], ref["lpos"], ref["goals"], T)
    np.testing.assert_array_equal(env.obs(), ref["obs0"])
    for t in range(T):
        obs, rew, dones = env.step(mpe_ref_np.onehot_actions(ref["actions"][:, t]))
        np.testing.assert_array_equal(obs, ref["obs"][:, t], err_msg=f"obs, step {t}")
        np.testing.assert_array_equal(rew, ref["rewards"][:, t], err_msg=f"rewards, step {t}")
        np.testing.assert_array_equal(dones, ref["dones"][:, t], err_msg=f"dones, step {t}")
    np.testing.assert_array_equal(env.pos, ref["pos1"])
    np.testing.assert_array_equal(env.vel, ref["vel1"])
    # the fixture has what the tests need it for: every move, most symbols, comm columns that are one-hot
    assert set(np.unique(ref["actions"][..., 0])) == {0, 1, 2, 3, 4} and len(np.unique(ref["actions"][..., 1])) >= 8
    assert (ref["obs"][..., 11:].sum(-1) == 1.0).all() and (ref["obs0"][..., 11:] == 0.0).all()


def test_oracle_equals_the_reference_simple_spread(fx):
    """oracle/mpe_oracle.py, which tests/test_mpe_env.py holds the spread kernel against, on the reference's own episodes: 1e-12
    absolute (the margin is for another libm's logaddexp)."""
    from oracle import mpe_oracle as R
    _, sp = fx
    E, T = sp["obs"].shape[:2]
    env = R.SimpleSpreadRef(sp["pos0"], sp["vel0"], sp["lpos"], T)
    np.testing.assert_allclose(env.obs(), sp["obs0"], rtol=0, atol=1e-12)
    worst = 0.0
    for t in range(T):
        def reset_states(n):                   # the reference env does not reset itself: keep the stepped state for the final check
            return env.pos[n], env.vel[n], env.lpos[n]
        obs, rew, dones = env.step(np.eye(5)[sp["actions"][:, t]], reset_states)
        worst = max(worst, np.abs(obs - sp["obs"][:, t]).max(), np.abs(rew[..., 0] - sp["rewards"][:, t]).max())
        np.testing.assert_allclose(obs, sp["obs"][:, t], rtol=0, atol=1e-12, err_msg=f"obs, step {t}")
        np.testing.assert_allclose(rew[..., 0], sp["rewards"][:, t], rtol=0, atol=1e-12, err_msg=f"rewards, step {t}")
        np.testing.assert_array_equal(dones, sp["dones"][:, t])
    print(f"simple_spread oracle vs reference: max |diff| {worst:.2e}")
    np.testing.assert_allclose(env.pos, sp["pos1"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(env.vel, sp["vel1"], rtol=0, atol=1e-12)
    # the contact force acted: a crowded episode's agents were pushed apart faster than any action can (5 * 0.1 per step)
    assert np.abs(sp["obs"][1::2, 0, :, :2]).max() > 0.5


# ---- the C ABI refuses what the kernels are not built for, before any launch -------------------------------------------------------
def _desc(in_dim=21, out_dim=15, layer_N=1, recurrent=0, relu=1):
    from mappo_amd import _lib
    return _lib.NetDesc(in_dim, 64, out_dim, layer_N, relu, 1, recurrent)


P = C.c_void_p(4096)                          # never dereferenced: the checks come before any launch


def _episode(actor=None, critic=None, heads=(5, 10), T=6, N=8, env_T=6, centralized=1, ptr=P):
    from mappo_amd import _lib
    lib = _lib.load()
    actor = actor if actor is not None else _desc()
    critic = critic if critic is not None else _desc(in_dim=42, out_dim=1)
    hd = (C.c_int32 * len(heads))(*heads)
    rc = lib.mappo_rollout_episode_reference(ptr, C.byref(actor), ptr, C.byref(critic), hd, len(heads), T, N, env_T, 1, ptr, ptr, ptr, ptr,
                                             ptr, ptr, 0, 1, 0, None, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, centralized, None)
    return rc, lib.mappo_last_error().decode()


EPISODE_BAD = [
    ("N=0", dict(N=0), ["N=0", ">= 1"]),
    ("T=0", dict(T=0), ["T=0", ">= 1"]),
    ("env_T=0", dict(env_T=0), ["episode length 0"]),
    ("heads(5,9)", dict(heads=(5, 9)), ["(5, 9", "exactly the heads (5, 10)"]),
    ("heads(5,5,5)", dict(heads=(5, 5, 5)), ["3 heads", "(5, 10)"]),
    ("actor in_dim 18", dict(actor=_desc(in_dim=18)), ["actor in_dim 18", "21 observation features"]),
    ("actor in_dim 65", dict(actor=_desc(in_dim=65)), ["in_dim 65", "64"]),
    ("critic in_dim 40 centralized", dict(critic=_desc(in_dim=40, out_dim=1)), ["centralized", "42", "got 40"]),
    ("critic in_dim 42 decentralized", dict(centralized=0), ["critic in_dim 42", "21"]),
    ("critic in_dim 128", dict(critic=_desc(in_dim=128, out_dim=1)), ["narrow", "64"]),
    ("recurrent", dict(actor=_desc(recurrent=1)), ["recurrent"]),
    ("recurrent critic", dict(critic=_desc(in_dim=42, out_dim=1, recurrent=1)), ["recurrent"]),
    ("layer_N 2", dict(actor=_desc(layer_N=2), critic=_desc(in_dim=42, out_dim=1, layer_N=2)), ["layer_N 2"]),
    ("layer_N differs", dict(critic=_desc(in_dim=42, out_dim=1, layer_N=0)), ["share layer_N"]),
    ("activation differs", dict(critic=_desc(in_dim=42, out_dim=1, relu=0)), ["activation"]),
    ("critic out_dim", dict(critic=_desc(in_dim=42, out_dim=2)), ["critic out_dim"]),
    ("null pointer", dict(ptr=None), ["null pointer"]),
]


@pytest.mark.parametrize("name,kw,words", EPISODE_BAD, ids=[b[0] for b in EPISODE_BAD])
def test_rollout_episode_reference_rejects(name, kw, words):
    from mappo_amd import _lib
    assert _lib.load().mappo_abi_version() >= 5
    rc, err = _episode(**kw)
    assert rc == -1, (name, rc)
    assert "rollout_episode_reference" in err, err
    for w in words:
        assert w in err, (name, err)


def test_mpe_reference_reset_and_step_reject():
    from mappo_amd import _lib
    lib = _lib.load()

    def reset(N=4, ptr=P):
        return lib.mappo_mpe_reference_reset(ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, 1, None), lib.mappo_last_error().decode()

    def step(N=4, mode=1, env_T=6, ptr=P):
        return (lib.mappo_mpe_reference_step(ptr, ptr, ptr, ptr, ptr, ptr, ptr, mode, ptr, ptr, ptr, N, env_T, 1, None),
                lib.mappo_last_error().decode())

    for call, who, cases in ((reset, "mpe_reference_reset", [(dict(N=0), ["N=0", "N >= 1"]), (dict(ptr=None), ["null pointer"])]),
                             (step, "mpe_reference_step", [(dict(N=0), ["N=0", "N >= 1"]), (dict(mode=2), ["action_mode 2"]),
                                                           (dict(mode=-1), ["action_mode -1"]), (dict(env_T=0), ["episode length 0"]),
                                                           (dict(ptr=None), ["null pointer"])])):
        for kw, words in cases:
            rc, err = call(**kw)
            assert rc == -1, (who, kw, rc)
            assert who in err, err
            for w in words:
                assert w in err, (who, kw, err)


def test_vec_env_rejects_other_action_shapes_by_name(monkeypatch):
    """step() names the shapes it takes; the check comes before anything touches the device (the env is built without one)."""
    import torch
    from mappo_amd.envs.mpe_reference import SimpleReferenceVecEnv
    env = SimpleReferenceVecEnv(4, device="cpu")
    assert env.action_space[0].__class__.__name__ == "MultiDiscrete" and list(env.action_space[0].high) == [4, 9] and len(env.action_space) == 2
    assert env.observation_space == [[21], [21]] and env.share_observation_space == [[42], [42]]
    assert env.graph_safe and env.accepts_device_actions and env.accepts_index_actions and env.consumes_actions
    st = env.episode_state_reference()
    assert st["scenario"] == "simple_reference" and st["goal"].dtype == torch.int32 and tuple(st["goal"].shape) == (4, 2)
    for shape in [(4, 2, 5), (4, 2, 1), (4, 2), (3, 2, 2), (4, 3, 15)]:
        with pytest.raises(ValueError, match=r"SimpleReferenceVecEnv.step: actions of shape .*\[N, 2, 15\].*\[N, 2, 2\]"):
            env.step(torch.zeros(shape))
    with pytest.raises(ValueError, match="2 agents and 3 landmarks"):
        SimpleReferenceVecEnv(4, num_agents=3, device="cpu")
    with pytest.raises(ValueError, match="landmark indices"):
        env.set_state(np.zeros((4, 2, 2)), np.zeros((4, 2, 2)), np.zeros((4, 3, 2)), np.full((4, 2), 3))
