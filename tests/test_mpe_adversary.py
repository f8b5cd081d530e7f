"""MPE simple_adversary without a GPU: the NumPy mirror (tests/mpe_adversary_np.py) EQUALS the fixture stepped by the reference's
own environment (tests/golden/mpe_adversary.npz) — the reset-on-done boundary of the 7-step runs included —, rewards are per agent,
the vec-env and the C ABI refuse by name what they are not built for, and the inputs of the GPU sampling comparison
(tests/test_gpu_mpe_adversary.py) keep clear of decision boundaries."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
import mpe_adversary_np as MA

OBS = ("adversary", "good1", "good2")


def _fx(tag):
    g = golden("mpe_adversary")
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}


def test_fixture_covers_what_it_claims():
    lo, sh = _fx("long"), _fx("short")
    assert lo["actions"].shape == (12, 25, 3) and sh["actions"].shape == (2, 14, 3)
    assert sorted(np.unique(lo["goal"])) == [0, 1] and sorted(np.unique(lo["actions"])) == [0, 1, 2, 3, 4]
    assert lo["dones"][:, :-1].sum() == 0 and lo["dones"][:, -1].all()
    assert sh["dones"][:, [6, 13]].all() and sh["dones"].sum() == 2 * 2 * 3
    assert lo["obs_adversary"].shape == (12, 25, 8) and lo["obs_good1"].shape == (12, 25, 10) and lo["obs_good2"].shape == (12, 25, 10)
    assert lo["rewards"].shape == (12, 25, 3) and lo["rewards"].dtype == np.float64
    np.testing.assert_array_equal(lo["vel0"], 0.0)
    # the good agents share one reward, the adversary has its own
    np.testing.assert_array_equal(lo["rewards"][..., 1], lo["rewards"][..., 2])


@pytest.mark.parametrize("onehot", [True, False], ids=["onehot", "index"])
def test_numpy_mirror_equals_reference_long_episodes(onehot):
    g = _fx("long")
    env = MA.SimpleAdversaryNp(g["pos0"], g["vel0"], g["lpos"], g["goal"], episode_length=25)
    for m, o in enumerate(env.obs()):
        np.testing.assert_array_equal(o, g["obs0_" + OBS[m]])
    for t in range(25):
        a = g["actions"][:, t]
        obs, rew, dones = env.step(np.eye(5)[a] if onehot else a)
        for m in range(3):
            np.testing.assert_array_equal(obs[m], g["obs_" + OBS[m]][:, t], err_msg=f"obs of agent {m}, step {t}")
        np.testing.assert_array_equal(rew, g["rewards"][:, t], err_msg=f"rewards, step {t}")
        np.testing.assert_array_equal(dones, g["dones"][:, t])
    np.testing.assert_array_equal(env.pos, g["pos1"])
    np.testing.assert_array_equal(env.vel, g["vel1"])


def test_numpy_mirror_equals_reference_across_reset_on_done():
    """episode_length 7, 14 steps: the steps that end an episode return the reset's observations (state reloaded from the fixture)
    and the ended step's rewards; the next episode continues from the reloaded state at rest."""
    g = _fx("short")
    env = MA.SimpleAdversaryNp(g["pos0"], g["vel0"], g["lpos"], g["goal"], episode_length=7)
    resets = 0
    for t in range(14):
        obs, rew, dones = env.step(g["actions"][:, t])
        np.testing.assert_array_equal(dones, g["dones"][:, t])
        np.testing.assert_array_equal(rew, g["rewards"][:, t], err_msg=f"rewards, step {t}")
        if dones.all():
            env.reload(np.arange(2), g["reset_pos"][:, resets], g["reset_lpos"][:, resets], g["reset_goal"][:, resets])
            obs = env.obs()
            resets += 1
        else:
            assert not dones.any()
        for m in range(3):
            np.testing.assert_array_equal(obs[m], g["obs_" + OBS[m]][:, t], err_msg=f"obs of agent {m}, step {t}")
    assert resets == 2


def test_rewards_are_per_agent():
    """A summed or shared reward would make agents 0 and 1 equal: they differ wherever the adversary is not on the goal."""
    for tag in ("long", "short"):
        g = _fx(tag)
        r = g["rewards"]
        off_goal = r[..., 0] != 0.0                               # the adversary's reward is -|p_adv - goal|^2
        assert off_goal.all()                                     # (nowhere in the fixture does it sit exactly on the goal)
        assert (r[..., 0][off_goal] != r[..., 1][off_goal]).all()
        assert (r[..., 0] <= 0).all()
        # the good agents' reward is not the negative of the adversary's either: it has the square roots
        assert (r[..., 1] != -r[..., 0]).any()


def test_vec_env_refuses_other_shapes_by_name_without_a_device():
    import torch
    from mappo_amd.envs import SimpleAdversaryVecEnv
    for n in (2, 4):
        with pytest.raises(ValueError, match="num_agents = 3"):
            SimpleAdversaryVecEnv(4, num_agents=n, device="cuda:7")
    env = SimpleAdversaryVecEnv(4, device="cpu")
    assert env.observation_space == [[8], [10], [10]] and env.share_observation_space == [[28], [28], [28]]
    assert [s.__class__.__name__ for s in env.action_space] == ["Discrete"] * 3 and [s.n for s in env.action_space] == [5, 5, 5]
    assert env.graph_safe and env.accepts_device_actions and env.accepts_index_actions and env.consumes_actions and env.ragged_obs
    st = env.episode_state_adversary()
    assert st["scenario"] == "simple_adversary" and tuple(st["agent_pos"].shape) == (4, 3, 2) and tuple(st["landmark_pos"].shape) == (4, 2, 2)
    assert tuple(st["goal"].shape) == (4,) and st["episode"].dtype == torch.int64 and set(env.state_tensors()) == {
        "agent_pos", "agent_vel", "landmark_pos", "goal", "tstep", "episode"}
    for bad in (torch.zeros(4, 5), [torch.zeros(4, 5)] * 2, [torch.zeros(4, 5), torch.zeros(4, 5), torch.zeros(4, 3)], torch.zeros(3, 3)):
        with pytest.raises(ValueError, match=r"SimpleAdversaryVecEnv.step: .*\[N, 5\].*\[N, 3, 5\].*\[N, 3\]"):
            env.step(bad)
    with pytest.raises(ValueError, match="landmark indices"):
        env.set_state(np.zeros((4, 3, 2)), np.zeros((4, 3, 2)), np.zeros((4, 2, 2)), np.full(4, 2))


# ---- the C ABI refuses what the kernels are not built for, before any launch -------------------------------------------------------
P = C.c_void_p(4096)                          # never dereferenced: the checks come before any launch


def test_mpe_adversary_reset_and_step_reject():
    from mappo_amd import _lib
    lib = _lib.load()
    assert lib.mappo_abi_version() >= 7

    def reset(N=4, M=3, ptr=P):
        return lib.mappo_mpe_adversary_reset(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, M, 1, None), lib.mappo_last_error().decode()

    def step(N=4, M=3, mode=1, env_T=6, ptr=P):
        return (lib.mappo_mpe_adversary_step(ptr, ptr, ptr, ptr, ptr, ptr, ptr, mode, ptr, ptr, ptr, ptr, ptr, N, M, env_T, 1, None),
                lib.mappo_last_error().decode())

    common = [(dict(N=0), ["N=0", "N >= 1"]), (dict(M=2), ["num_agents=2", "num_agents = 3"]), (dict(M=4), ["num_agents=4", "num_agents = 3"]),
              (dict(ptr=None), ["null pointer"])]
    for call, who, cases in ((reset, "mpe_adversary_reset", common),
                             (step, "mpe_adversary_step", common + [(dict(mode=2), ["action_mode 2"]), (dict(mode=-1), ["action_mode -1"]),
                                                                    (dict(env_T=0), ["episode length 0"])])):
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


def _episode(actors=None, critics=None, T=6, N=8, env_T=6, centralized=1, ptr=P, state=P, null_agents=False):
    """actors / critics: {agent: descriptor} replacing the valid ones."""
    from mappo_amd import _lib
    lib = _lib.load()
    ags = []
    for m, D in enumerate(MA.OBS_DIMS):
        a = (actors or {}).get(m) or _desc(D, 5)
        c = (critics or {}).get(m) or _desc(28 if centralized else D, 1)
        ags.append(_agent(a, c, ptr))
    arr = (_lib.CommAgent * 3)(*ags)
    rc = lib.mappo_rollout_episode_adversary(None if null_agents else arr, state, state, state, state, state, state, T, N, env_T, 1, 0, 0,
                                             centralized, None)
    return rc, lib.mappo_last_error().decode()


def _all(layer_N):
    return dict(actors={m: _desc(D, 5, layer_N=layer_N) for m, D in enumerate(MA.OBS_DIMS)}, critics={m: _desc(28, 1, layer_N=layer_N) for m in range(3)})


EPISODE_BAD = [
    ("N=0", dict(N=0), ["N=0", ">= 1"]),
    ("T=0", dict(T=0), ["T=0", ">= 1"]),
    ("env_T=0", dict(env_T=0), ["episode length 0"]),
    ("null agents", dict(null_agents=True), ["null agent descriptors", "num_agents = 3"]),
    ("null buffer pointer", dict(ptr=None), ["null pointer", "adversary"]),
    ("null state pointer", dict(state=None), ["null state pointer"]),
    ("recurrent adversary actor", dict(actors={0: _desc(8, 5, recurrent=1)}), ["adversary", "recurrent"]),
    ("recurrent good critic", dict(critics={2: _desc(28, 1, recurrent=1)}), ["good agent 2", "recurrent"]),
    ("layer_N 2", _all(2), ["layer_N 2", "layer_N <= 1"]),
    ("adversary in_dim 10", dict(actors={0: _desc(10, 5)}), ["adversary actor in_dim 10", "in_dim 8"]),
    ("good agent in_dim 8", dict(actors={1: _desc(8, 5)}), ["good agent 1 actor in_dim 8", "in_dim 10"]),
    ("good agent out_dim 3", dict(actors={2: _desc(10, 3)}), ["good agent 2 actor in_dim 10 / out_dim 3", "5 actions"]),
    ("critic 27 centralized", dict(critics={0: _desc(27, 1)}), ["centralized", "28", "got 27"]),
    ("critic 28 decentralized", dict(centralized=0, critics={1: _desc(28, 1)}), ["good agent 1 critic in_dim 28", "10"]),
    ("critic out_dim", dict(critics={1: _desc(28, 2)}), ["critic out_dim"]),
    ("layer_N differs", dict(critics={2: _desc(28, 1, layer_N=0)}), ["share layer_N"]),
    ("activation differs", dict(actors={1: _desc(10, 5, relu=0)}), ["activation"]),
]


@pytest.mark.parametrize("name,kw,words", EPISODE_BAD, ids=[b[0] for b in EPISODE_BAD])
def test_rollout_episode_adversary_rejects(name, kw, words):
    rc, err = _episode(**kw)
    assert rc == -1, (name, rc)
    assert "rollout_episode_adversary" in err, err
    for w in words:
        assert w in err, (name, err)


def test_ops_refuses_another_number_of_agents():
    from mappo_amd import ops
    with pytest.raises(ValueError, match="num_agents = 3"):
        ops.rollout_episode_adversary([None, None], 4, 4, 4, 1, *[None] * 6, False, 0, True)


def test_host_reset_draws_follow_the_index_rule():
    """The host restatement of the reset draws (what the GPU reset is held against): in range, both goals, no index shared."""
    pos, lpos, goal = MA.reset_draws(7, 1, 37)
    assert pos.shape == (37, 3, 2) and lpos.shape == (37, 2, 2) and sorted(np.unique(goal)) == [0, 1]
    allv = np.concatenate([pos.reshape(-1), lpos.reshape(-1)])
    assert (allv >= -1).all() and (allv < 1).all() and len(np.unique(allv)) == allv.size
    p2, _, _ = MA.reset_draws(7, 2, 37)
    assert not np.array_equal(pos, p2)


# ---- the inputs of the float64 sampling comparison (tests/test_gpu_mpe_adversary.py) keep clear of decision boundaries -------------
def test_adversary_rollout_inputs_stay_under_the_exclusion_cap():
    """On the reference side alone (oracle networks in float64 / float32, host Philox, the NumPy mirror): over the T steps of N
    environments, at most 2 % of the (row, agent) pairs sit within the exclusion margin of tests/rollout_ref.py."""
    import adversary_rollout_ref as AR
    ref = AR.reference_rollout()
    near = np.concatenate([e.near for m in range(3) for e in ref["expected"][m]])
    assert near.mean() <= AR.NEAR_CAP, f"{near.sum()} of {near.size} (row, agent) pairs near a boundary"
    for m in range(3):
        assert len(np.unique(np.concatenate(ref["actions"][m]))) > 1, "an agent that only ever takes one action tests nothing"
