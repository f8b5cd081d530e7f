"""MPE simple_push without a GPU: the fixture stepped by the reference's own environment (tests/golden/mpe_push.npz) covers what it
claims — real contacts between the two agents among it —, the NumPy mirror (tests/mpe_push_np.py) EQUALS it — the reset-on-done
boundary of the 7-step runs and the scripted contact episodes included —, rewards are per agent, and the vec-env, `ops` and the C ABI
refuse by name what they are not built for."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
import mpe_push_np as MP

OBS = MP.OBS


def _fx(tag):
    g = golden("mpe_push")
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}


def test_fixture_covers_what_it_claims():
    lo, sh, co = _fx("long"), _fx("short"), _fx("contact")
    assert lo["actions"].shape == (12, 25, 2) and sh["actions"].shape == (2, 14, 2) and co["actions"].shape == (6, 25, 2)
    for g in (lo, co):
        assert g["dones"][:, :-1].sum() == 0 and g["dones"][:, -1].all()
        assert sorted(np.unique(g["goal"])) == [0, 1] and sorted(np.unique(g["actions"])) == [0, 1, 2, 3, 4]
        E = g["actions"].shape[0]
        for n, d in zip(OBS, MP.OBS_DIMS):
            assert g["obs_" + n].shape == (E, 25, d) and g["obs0_" + n].shape == (E, d)
        assert g["rewards"].shape == (E, 25, 2) and g["rewards"].dtype == np.float64
    assert sh["dones"][:, [6, 13]].all() and sh["dones"].sum() == 2 * 2 * 2 and sh["reset_pos"].shape == (2, 2, 2, 2)
    assert sh["reset_goal"].shape == (2, 2) and sorted(np.unique(np.concatenate([sh["goal"], sh["reset_goal"].reshape(-1)]))) == [0, 1]
    # the good agent's colour names the goal, the landmarks' colours are fixed (float64 sums of the reference)
    for g in (lo, co):
        np.testing.assert_array_equal(g["obs0_good"][:, 4:7], MP.good_color(g["goal"]))
        np.testing.assert_array_equal(g["obs_good"][:, 3, 11:17], np.broadcast_to(MP.landmark_colors().reshape(1, 6), (len(g["goal"]), 6)))


def test_contact_steps_really_are_contacts():
    """contact/: three episodes start with the agents inside each other's contact distance, the others are driven into each other;
    where they touch, the velocity change is not what the action alone gives — the contact force acted."""
    g = _fx("contact")
    start = MP.in_contact(g["pos0"])
    assert start.tolist() == [True] * 3 + [False] * 3
    pos = MP.positions_after(g)                                      # [E, T, 2, 2]
    np.testing.assert_allclose(pos[:, -1], g["pos1"], rtol=0, atol=1e-15)
    touch = MP.in_contact(pos)                                       # [E, T] after each step
    print("steps in contact per episode:", touch.sum(1), "closest approach:", MP._norm(pos[..., 0, :] - pos[..., 1, :]).min())
    assert (touch[3:].sum(1) >= 1).all() and touch.sum() >= 20
    before = np.concatenate([start[:, None], touch[:, :-1]], axis=1)  # in contact when step t began
    vel = np.stack([g["obs_adversary"][..., 0:2], g["obs_good"][..., 0:2]], axis=2)
    prev = np.concatenate([g["vel0"][:, None], vel[:, :-1]], axis=1)
    a1h = np.eye(5)[g["actions"]]
    u = np.stack([a1h[..., 1] - a1h[..., 2], a1h[..., 3] - a1h[..., 4]], axis=-1) * 5.0
    free = prev * 0.75 + u * 0.1                                     # the velocity without a contact force
    extra = np.abs(vel - free).max(axis=(2, 3))                      # [E, T]
    assert (extra[before] > 1e-3).all(), "a step that began in contact shows no contact force"
    far = MP._norm(np.concatenate([g["pos0"][:, None], pos[:, :-1]], axis=1)[..., 0, :]
                   - np.concatenate([g["pos0"][:, None], pos[:, :-1]], axis=1)[..., 1, :]) > 0.2
    assert far.any() and (extra[far] < 1e-12).all()                  # and none a contact distance apart
    # equal and opposite: both masses are 1
    np.testing.assert_allclose((vel - free)[:, :, 0], -(vel - free)[:, :, 1], rtol=0, atol=1e-15)


@pytest.mark.parametrize("tag", ["long", "contact"])
@pytest.mark.parametrize("onehot", [True, False], ids=["onehot", "index"])
def test_numpy_mirror_equals_reference_whole_episodes(tag, onehot):
    g = _fx(tag)
    env = MP.SimplePushNp(g["pos0"], g["vel0"], g["lpos"], g["goal"], episode_length=25)
    for m, o in enumerate(env.obs()):
        np.testing.assert_array_equal(o, g["obs0_" + OBS[m]])
    for t in range(25):
        a = g["actions"][:, t]
        obs, rew, dones = env.step(np.eye(5)[a] if onehot else a)
        for m in range(2):
            np.testing.assert_array_equal(obs[m], g["obs_" + OBS[m]][:, t], err_msg=f"obs of agent {m}, step {t}")
        np.testing.assert_array_equal(rew, g["rewards"][:, t], err_msg=f"rewards, step {t}")
        np.testing.assert_array_equal(dones, g["dones"][:, t])
    np.testing.assert_array_equal(env.pos, g["pos1"])
    np.testing.assert_array_equal(env.vel, g["vel1"])


@pytest.mark.parametrize("onehot", [True, False], ids=["onehot", "index"])
def test_numpy_mirror_equals_reference_across_reset_on_done(onehot):
    """episode_length 7, 14 steps: the steps that end an episode return the reset's observations (state reloaded from the fixture)
    and the ended step's rewards; the next episode continues from the reloaded state at rest."""
    g = _fx("short")
    env = MP.SimplePushNp(g["pos0"], g["vel0"], g["lpos"], g["goal"], episode_length=7)
    resets = 0
    for t in range(14):
        a = g["actions"][:, t]
        obs, rew, dones = env.step(np.eye(5)[a] if onehot else a)
        np.testing.assert_array_equal(dones, g["dones"][:, t])
        np.testing.assert_array_equal(rew, g["rewards"][:, t], err_msg=f"rewards, step {t}")
        if dones.all():
            env.reload(np.arange(2), g["reset_pos"][:, resets], g["reset_lpos"][:, resets], g["reset_goal"][:, resets])
            obs = env.obs()
            resets += 1
        else:
            assert not dones.any()
        for m in range(2):
            np.testing.assert_array_equal(obs[m], g["obs_" + OBS[m]][:, t], err_msg=f"obs of agent {m}, step {t}")
    assert resets == 2


def test_rewards_are_per_agent():
    """The good agent is paid -|good - goal|, the adversary |good - goal| - |adversary - goal|: a summed or shared reward would make
    the two equal."""
    for tag in ("long", "short", "contact"):
        r = _fx(tag)["rewards"]
        assert (r[..., 1] <= 0).all() and (r[..., 0] != r[..., 1]).all()
        assert (r[..., 0] > 0).any() and (r[..., 0] < 0).any()
        assert (r[..., 0] + r[..., 1] <= 0).all()                     # their sum is -|adversary - goal|


def test_vec_env_and_ops_refuse_other_shapes_by_name_without_a_device():
    import torch
    from mappo_amd import ops
    from mappo_amd.envs import SimplePushVecEnv
    for n in (1, 3, 4):
        with pytest.raises(ValueError, match=f"num_agents = 2.*got num_agents {n}, num_landmarks 2"):
            SimplePushVecEnv(4, num_agents=n, device="cuda:7")
        with pytest.raises(ValueError, match="mpe_push_reset: simple_push is built for num_agents = 2"):
            ops.mpe_push_reset(*[None] * 8, 4, 1, num_agents=n)
        with pytest.raises(ValueError, match="mpe_push_step: simple_push is built for num_agents = 2"):
            ops.mpe_push_step(*[None] * 6, None, 1, *[None] * 4, 4, 25, 1, num_agents=n)
    for l in (1, 3):
        with pytest.raises(ValueError, match=f"1 adversary, 1 good agent, 2 landmarks .got num_agents 2, num_landmarks {l}"):
            SimplePushVecEnv(4, device="cuda:7", num_landmarks=l)
    env = SimplePushVecEnv(4, device="cpu")
    assert env.observation_space == [[8], [19]] and env.share_observation_space == [[27]] * 2
    assert [s.__class__.__name__ for s in env.action_space] == ["Discrete"] * 2 and [s.n for s in env.action_space] == [5] * 2
    assert env.graph_safe and env.accepts_device_actions and env.accepts_index_actions and env.consumes_actions and env.ragged_obs
    assert env.episode_flag == "MAPPO_PUSH_EPISODE" and (env.M, env.L) == (2, 2) and hasattr(env, "episode_launch")
    st = env.state_tensors()
    assert set(st) == {"agent_pos", "agent_vel", "landmark_pos", "goal", "tstep", "episode"}
    assert tuple(st["agent_pos"].shape) == (4, 2, 2) and tuple(st["landmark_pos"].shape) == (4, 2, 2) and st["goal"].dtype == torch.int32
    assert st["episode"].dtype == torch.int64
    with pytest.raises(ValueError, match="goal must be landmark indices"):
        env.set_state(np.zeros((4, 2, 2)), np.zeros((4, 2, 2)), np.zeros((4, 2, 2)), [0, 1, 2, 0])
    for bad in (torch.zeros(4, 5), [torch.zeros(4, 5)] * 3, [torch.zeros(4, 5), torch.zeros(4, 3)], torch.zeros(4, 3), torch.zeros(3, 2)):
        with pytest.raises(ValueError, match=r"SimplePushVecEnv.step: .*\[N, 5\].*\[N, 2, 5\].*\[N, 2\]"):
            env.step(bad)


# ---- the C ABI refuses what the kernels are not built for, before any launch -------------------------------------------------------
P = C.c_void_p(4096)                          # never dereferenced: the checks come before any launch


def test_mpe_push_reset_and_step_reject():
    from mappo_amd import _lib
    lib = _lib.load()
    assert lib.mappo_abi_version() >= 10

    def reset(N=4, M=2, ptr=P):
        return lib.mappo_mpe_push_reset(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, M, 1, None), lib.mappo_last_error().decode()

    def step(N=4, M=2, mode=1, env_T=6, ptr=P):
        return (lib.mappo_mpe_push_step(ptr, ptr, ptr, ptr, ptr, ptr, ptr, mode, ptr, ptr, ptr, ptr, N, M, env_T, 1, None),
                lib.mappo_last_error().decode())

    common = [(dict(N=0), ["N=0", "N >= 1"]), (dict(M=3), ["num_agents=3", "num_agents = 2"]), (dict(M=1), ["num_agents=1", "num_agents = 2"]),
              (dict(ptr=None), ["null pointer"])]
    for call, who, cases in ((reset, "mpe_push_reset", common),
                             (step, "mpe_push_step", common + [(dict(mode=2), ["action_mode 2"]), (dict(mode=-1), ["action_mode -1"]),
                                                               (dict(env_T=0), ["episode length 0"])])):
        for kw, words in cases:
            rc, err = call(**kw)
            assert rc == -1, (who, kw, rc)
            assert who in err, err
            for w in words:
                assert w in err, (who, kw, err)


def test_host_reset_draws_follow_the_index_rule():
    """The host restatement of the reset draws (what the GPU reset is held against): agents in [-1, 1), landmarks in 0.8 [-1, 1), both
    goals, no index shared, another stream per episode."""
    pos, lpos, goal = MP.reset_draws(7, 1, 37)
    assert pos.shape == (37, 2, 2) and lpos.shape == (37, 2, 2) and goal.shape == (37,)
    assert (pos >= -1).all() and (pos < 1).all() and (np.abs(lpos) <= 0.8).all() and np.abs(lpos).max() > 0.7
    assert sorted(np.unique(goal)) == [0, 1]
    allv = np.concatenate([pos.reshape(-1), lpos.reshape(-1) / 0.8])
    assert len(np.unique(allv)) == allv.size
    p2, _, _ = MP.reset_draws(7, 2, 37)
    assert not np.array_equal(pos, p2)
    # environment n draws at 16 n + k: the first environment of a 37-wide reset is the only environment of a 1-wide one
    p1, l1, g1 = MP.reset_draws(7, 1, 1)
    np.testing.assert_array_equal(p1[0], pos[0]); np.testing.assert_array_equal(l1[0], lpos[0]); assert g1[0] == goal[0]


# ---- the one-launch episode's entry point refuses what it is not built for, before any launch -----------------------------------
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
    for m, D in enumerate(MP.OBS_DIMS):
        a = (actors or {}).get(m) or _desc(D, 5)
        c = (critics or {}).get(m) or _desc(27 if centralized else D, 1)
        ags.append(_agent(a, c, ptr))
    arr = (_lib.CommAgent * 2)(*ags)
    rc = lib.mappo_rollout_episode_push(None if null_agents else arr, state, state, state, state, state, state, T, N, env_T, 1, 0, 0, centralized,
                                        None)
    return rc, lib.mappo_last_error().decode()


def _all(layer_N):
    return dict(actors={m: _desc(D, 5, layer_N=layer_N) for m, D in enumerate(MP.OBS_DIMS)}, critics={m: _desc(27, 1, layer_N=layer_N) for m in range(2)})


EPISODE_BAD = [
    ("N=0", dict(N=0), ["N=0", ">= 1"]),
    ("T=0", dict(T=0), ["T=0", ">= 1"]),
    ("env_T=0", dict(env_T=0), ["episode length 0"]),
    ("null agents", dict(null_agents=True), ["null agent descriptors", "num_agents = 2"]),
    ("null buffer pointer", dict(ptr=None), ["null pointer", "adversary"]),
    ("null state pointer", dict(state=None), ["null state pointer"]),
    ("recurrent adversary actor", dict(actors={0: _desc(8, 5, recurrent=1)}), ["adversary", "recurrent"]),
    ("recurrent good critic", dict(critics={1: _desc(27, 1, recurrent=1)}), ["good agent", "recurrent"]),
    ("layer_N 2", _all(2), ["layer_N 2", "layer_N <= 1"]),
    ("adversary in_dim 19", dict(actors={0: _desc(19, 5)}), ["adversary actor in_dim 19", "in_dim 8"]),
    ("good agent in_dim 8", dict(actors={1: _desc(8, 5)}), ["good agent actor in_dim 8", "in_dim 19"]),
    ("good agent out_dim 3", dict(actors={1: _desc(19, 3)}), ["good agent actor in_dim 19 / out_dim 3", "5 actions"]),
    ("critic 28 centralized", dict(critics={0: _desc(28, 1)}), ["centralized", "8 + 19 = 27", "got 28"]),
    ("critic 27 decentralized", dict(centralized=0, critics={1: _desc(27, 1)}), ["good agent critic in_dim 27", "19"]),
    ("critic out_dim", dict(critics={1: _desc(27, 2)}), ["critic out_dim"]),
    ("layer_N differs", dict(critics={1: _desc(27, 1, layer_N=0)}), ["share layer_N"]),
    ("activation differs", dict(actors={1: _desc(19, 5, relu=0)}), ["activation"]),
]


@pytest.mark.parametrize("name,kw,words", EPISODE_BAD, ids=[b[0] for b in EPISODE_BAD])
def test_rollout_episode_push_rejects(name, kw, words):
    rc, err = _episode(**kw)
    assert rc == -1, (name, rc)
    assert "rollout_episode_push" in err, err
    for w in words:
        assert w in err, (name, err)


def test_ops_refuses_another_number_of_episode_agents():
    from mappo_amd import ops
    for k in (1, 3):
        with pytest.raises(ValueError, match="rollout_episode_push: simple_push is built for num_agents = 2"):
            ops.rollout_episode_push([None] * k, 4, 4, 4, 1, *[None] * 6, False, 0, True)


def test_push_rollout_inputs_stay_under_the_exclusion_cap():
    """On the reference side alone (oracle networks in float64 / float32, host Philox, the NumPy mirror): over the T steps of N
    environments, at most 2 % of the (row, agent) pairs sit within the exclusion margin of tests/rollout_ref.py."""
    import push_rollout_ref as PR
    ref = PR.reference_rollout()
    near = np.concatenate([e.near for m in range(2) for e in ref["expected"][m]])
    assert near.mean() <= PR.NEAR_CAP, f"{near.sum()} of {near.size} (row, agent) pairs near a boundary"
    for m in range(2):
        assert len(np.unique(np.concatenate(ref["actions"][m]))) > 1, "an agent that only ever takes one action tests nothing"
