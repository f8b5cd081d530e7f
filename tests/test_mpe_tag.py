"""MPE simple_tag without a GPU: the fixture stepped by the reference's own environment (tests/golden/mpe_tag.npz) reaches every
branch it claims, the NumPy mirror (tests/mpe_tag_np.py) EQUALS it — the reset-on-done boundary of the 7-step runs included —,
rewards are per agent, and the vec-env, `ops` and the C ABI refuse by name what they are not built for."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
import mpe_tag_np as MT

OBS = MT.OBS


def _fx(tag):
    g = golden("mpe_tag")
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}


def test_fixture_covers_what_it_claims():
    lo, sh = _fx("long"), _fx("short")
    assert lo["actions"].shape == (12, 25, 4) and sh["actions"].shape == (2, 14, 4)
    assert lo["dones"][:, :-1].sum() == 0 and lo["dones"][:, -1].all()
    assert sh["dones"][:, [6, 13]].all() and sh["dones"].sum() == 2 * 2 * 4 and sh["reset_pos"].shape == (2, 2, 4, 2)
    for n, d in zip(OBS, MT.OBS_DIMS):
        assert lo["obs_" + n].shape == (12, 25, d) and lo["obs0_" + n].shape == (12, d)
    assert lo["rewards"].shape == (12, 25, 4) and lo["rewards"].dtype == np.float64
    c = MT.coverage(lo)
    print(c)
    # an adversary on the good agent (+10 / -10), two at once (+20 / -20), agents on landmarks, two adversaries on each other
    for k in ("one_contact", "two_contacts", "adversary_landmark", "good_landmark", "adversary_adversary"):
        assert c[k] >= 1, (k, c)
    # the speed clamp engaged (free-flight speed above max_speed, stepped speed on it) and did not, for both kinds of agent
    for k in ("adversary_clamped", "good_clamped", "adversary_unclamped", "good_unclamped"):
        assert c[k] >= 1, (k, c)
    # every branch of the boundary penalty: |x| < 0.9, [0.9, 1), [1, 1 + ln(10) / 2], beyond the cap
    for k in ("bound_inside", "bound_linear", "bound_exp", "bound_capped"):
        assert c[k] >= 1, (k, c)
    assert c["actions"] == [0, 1, 2, 3, 4]
    r = lo["rewards"]
    assert (r[..., 3] <= -20.0).any()
    # the capped branch pays exactly 10 per coordinate
    x = np.abs(lo["obs_good"][..., 2:4])
    far = (x[..., 0] > 1 + np.log(10) / 2) & (x[..., 1] < 0.9) & (r[..., 0] == 0)
    assert far.any() and (r[..., 3][far] == -10.0).all()


@pytest.mark.parametrize("onehot", [True, False], ids=["onehot", "index"])
def test_numpy_mirror_equals_reference_long_episodes(onehot):
    g = _fx("long")
    env = MT.SimpleTagNp(g["pos0"], g["vel0"], g["lpos"], episode_length=25)
    for m, o in enumerate(env.obs()):
        np.testing.assert_array_equal(o, g["obs0_" + OBS[m]])
    clamped = np.zeros(4, np.int64)
    for t in range(25):
        a = g["actions"][:, t]
        obs, rew, dones = env.step(np.eye(5)[a] if onehot else a)
        for m in range(4):
            np.testing.assert_array_equal(obs[m], g["obs_" + OBS[m]][:, t], err_msg=f"obs of agent {m}, step {t}")
        np.testing.assert_array_equal(rew, g["rewards"][:, t], err_msg=f"rewards, step {t}")
        np.testing.assert_array_equal(dones, g["dones"][:, t])
        clamped += (env.pre_speed > MT.MAX_SPEED).sum(0)
    np.testing.assert_array_equal(env.pos, g["pos1"])
    np.testing.assert_array_equal(env.vel, g["vel1"])
    assert (clamped > 0).all(), clamped                              # pre-clamp speed above 1.0 / 1.3, for every agent


@pytest.mark.parametrize("onehot", [True, False], ids=["onehot", "index"])
def test_numpy_mirror_equals_reference_across_reset_on_done(onehot):
    """episode_length 7, 14 steps: the steps that end an episode return the reset's observations (state reloaded from the fixture)
    and the ended step's rewards; the next episode continues from the reloaded state at rest."""
    g = _fx("short")
    env = MT.SimpleTagNp(g["pos0"], g["vel0"], g["lpos"], episode_length=7)
    resets = 0
    for t in range(14):
        a = g["actions"][:, t]
        obs, rew, dones = env.step(np.eye(5)[a] if onehot else a)
        np.testing.assert_array_equal(dones, g["dones"][:, t])
        np.testing.assert_array_equal(rew, g["rewards"][:, t], err_msg=f"rewards, step {t}")
        if dones.all():
            env.reload(np.arange(2), g["reset_pos"][:, resets], g["reset_lpos"][:, resets])
            obs = env.obs()
            resets += 1
        else:
            assert not dones.any()
        for m in range(4):
            np.testing.assert_array_equal(obs[m], g["obs_" + OBS[m]][:, t], err_msg=f"obs of agent {m}, step {t}")
    assert resets == 2


def test_rewards_are_per_agent():
    """The adversaries share one number and the good agent has its own: a summed or shared reward would make all four equal."""
    for tag in ("long", "short"):
        r = _fx(tag)["rewards"]
        np.testing.assert_array_equal(r[..., 0], r[..., 1])
        np.testing.assert_array_equal(r[..., 0], r[..., 2])
        assert (r[..., 0] >= 0).all() and (r[..., 3] <= 0).all()
    r = _fx("long")["rewards"]
    hit = r[..., 0] > 0
    assert hit.any() and (r[..., 3][hit] <= -r[..., 0][hit]).all() and (r[..., 3] != -r[..., 0]).any()
    assert set(np.unique(r[..., 0])) == {0.0, 10.0, 20.0}


def test_vec_env_and_ops_refuse_other_shapes_by_name_without_a_device():
    import torch
    from mappo_amd import ops
    from mappo_amd.envs import SimpleTagVecEnv
    for n in (2, 3, 5):
        with pytest.raises(ValueError, match="num_agents = 4"):
            SimpleTagVecEnv(4, num_agents=n, device="cuda:7")
        with pytest.raises(ValueError, match="mpe_tag_reset: simple_tag is built for num_agents = 4"):
            ops.mpe_tag_reset(*[None] * 9, 4, 1, num_agents=n)
        with pytest.raises(ValueError, match="mpe_tag_step: simple_tag is built for num_agents = 4"):
            ops.mpe_tag_step(*[None] * 6, 1, *[None] * 6, 4, 25, 1, num_agents=n)
    for kw in (dict(num_adversaries=2), dict(num_good_agents=2), dict(num_landmarks=3)):
        with pytest.raises(ValueError, match="3 adversaries, 1 good agent, 2 landmarks"):
            SimpleTagVecEnv(4, device="cuda:7", **kw)
    env = SimpleTagVecEnv(4, device="cpu")
    assert env.observation_space == [[16], [16], [16], [14]] and env.share_observation_space == [[62]] * 4
    assert [s.__class__.__name__ for s in env.action_space] == ["Discrete"] * 4 and [s.n for s in env.action_space] == [5] * 4
    assert env.graph_safe and env.accepts_device_actions and env.accepts_index_actions and env.consumes_actions and env.ragged_obs
    st = env.episode_state_tag()
    assert st["scenario"] == "simple_tag" and tuple(st["agent_pos"].shape) == (4, 4, 2) and tuple(st["landmark_pos"].shape) == (4, 2, 2)
    assert st["episode"].dtype == torch.int64 and set(env.state_tensors()) == {"agent_pos", "agent_vel", "landmark_pos", "tstep", "episode"}
    for bad in (torch.zeros(4, 5), [torch.zeros(4, 5)] * 3, [torch.zeros(4, 5)] * 3 + [torch.zeros(4, 3)], torch.zeros(4, 3), torch.zeros(3, 4)):
        with pytest.raises(ValueError, match=r"SimpleTagVecEnv.step: .*\[N, 5\].*\[N, 4, 5\].*\[N, 4\]"):
            env.step(bad)


# ---- the C ABI refuses what the kernels are not built for, before any launch -------------------------------------------------------
P = C.c_void_p(4096)                          # never dereferenced: the checks come before any launch


def test_mpe_tag_reset_and_step_reject():
    from mappo_amd import _lib
    lib = _lib.load()
    assert lib.mappo_abi_version() >= 9

    def reset(N=4, M=4, ptr=P):
        return lib.mappo_mpe_tag_reset(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, M, 1, None), lib.mappo_last_error().decode()

    def step(N=4, M=4, mode=1, env_T=6, ptr=P):
        return (lib.mappo_mpe_tag_step(ptr, ptr, ptr, ptr, ptr, ptr, mode, ptr, ptr, ptr, ptr, ptr, ptr, N, M, env_T, 1, None),
                lib.mappo_last_error().decode())

    common = [(dict(N=0), ["N=0", "N >= 1"]), (dict(M=3), ["num_agents=3", "num_agents = 4"]), (dict(M=5), ["num_agents=5", "num_agents = 4"]),
              (dict(ptr=None), ["null pointer"])]
    for call, who, cases in ((reset, "mpe_tag_reset", common),
                             (step, "mpe_tag_step", common + [(dict(mode=2), ["action_mode 2"]), (dict(mode=-1), ["action_mode -1"]),
                                                              (dict(env_T=0), ["episode length 0"])])):
        for kw, words in cases:
            rc, err = call(**kw)
            assert rc == -1, (who, kw, rc)
            assert who in err, err
            for w in words:
                assert w in err, (who, kw, err)


def test_host_reset_draws_follow_the_index_rule():
    """The host restatement of the reset draws (what the GPU reset is held against): agents in [-1, 1), landmarks in 0.8 [-1, 1), no
    index shared, another stream per episode."""
    pos, lpos = MT.reset_draws(7, 1, 37)
    assert pos.shape == (37, 4, 2) and lpos.shape == (37, 2, 2)
    assert (pos >= -1).all() and (pos < 1).all() and (np.abs(lpos) <= 0.8).all() and np.abs(lpos).max() > 0.7
    allv = np.concatenate([pos.reshape(-1), lpos.reshape(-1) / 0.8])
    assert len(np.unique(allv)) == allv.size
    p2, _ = MT.reset_draws(7, 2, 37)
    assert not np.array_equal(pos, p2)
    # environment n draws at 16 n + k: the first environment of a 37-wide reset is the only environment of a 1-wide one
    p1, l1 = MT.reset_draws(7, 1, 1)
    np.testing.assert_array_equal(p1[0], pos[0]); np.testing.assert_array_equal(l1[0], lpos[0])


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
    for m, D in enumerate(MT.OBS_DIMS):
        a = (actors or {}).get(m) or _desc(D, 5)
        c = (critics or {}).get(m) or _desc(62 if centralized else D, 1)
        ags.append(_agent(a, c, ptr))
    arr = (_lib.CommAgent * 4)(*ags)
    rc = lib.mappo_rollout_episode_tag(None if null_agents else arr, state, state, state, state, state, T, N, env_T, 1, 0, 0, centralized, None)
    return rc, lib.mappo_last_error().decode()


def _all(layer_N):
    return dict(actors={m: _desc(D, 5, layer_N=layer_N) for m, D in enumerate(MT.OBS_DIMS)}, critics={m: _desc(62, 1, layer_N=layer_N) for m in range(4)})


EPISODE_BAD = [
    ("N=0", dict(N=0), ["N=0", ">= 1"]),
    ("T=0", dict(T=0), ["T=0", ">= 1"]),
    ("env_T=0", dict(env_T=0), ["episode length 0"]),
    ("null agents", dict(null_agents=True), ["null agent descriptors", "num_agents = 4"]),
    ("null buffer pointer", dict(ptr=None), ["null pointer", "adversary 0"]),
    ("null state pointer", dict(state=None), ["null state pointer"]),
    ("recurrent adversary actor", dict(actors={0: _desc(16, 5, recurrent=1)}), ["adversary 0", "recurrent"]),
    ("recurrent good critic", dict(critics={3: _desc(62, 1, recurrent=1)}), ["good agent", "recurrent"]),
    ("layer_N 2", _all(2), ["layer_N 2", "layer_N <= 1"]),
    ("adversary in_dim 14", dict(actors={1: _desc(14, 5)}), ["adversary 1 actor in_dim 14", "in_dim 16"]),
    ("good agent in_dim 16", dict(actors={3: _desc(16, 5)}), ["good agent actor in_dim 16", "in_dim 14"]),
    ("adversary out_dim 3", dict(actors={2: _desc(16, 3)}), ["adversary 2 actor in_dim 16 / out_dim 3", "5 actions"]),
    ("critic 61 centralized", dict(critics={0: _desc(61, 1)}), ["centralized", "62", "got 61"]),
    ("critic 62 decentralized", dict(centralized=0, critics={3: _desc(62, 1)}), ["good agent critic in_dim 62", "14"]),
    ("critic out_dim", dict(critics={1: _desc(62, 2)}), ["critic out_dim"]),
    ("layer_N differs", dict(critics={2: _desc(62, 1, layer_N=0)}), ["share layer_N"]),
    ("activation differs", dict(actors={1: _desc(16, 5, relu=0)}), ["activation"]),
]


@pytest.mark.parametrize("name,kw,words", EPISODE_BAD, ids=[b[0] for b in EPISODE_BAD])
def test_rollout_episode_tag_rejects(name, kw, words):
    rc, err = _episode(**kw)
    assert rc == -1, (name, rc)
    assert "rollout_episode_tag" in err, err
    for w in words:
        assert w in err, (name, err)


def test_ops_refuses_another_number_of_episode_agents():
    from mappo_amd import ops
    for k in (3, 5):
        with pytest.raises(ValueError, match="rollout_episode_tag: simple_tag is built for num_agents = 4"):
            ops.rollout_episode_tag([None] * k, 4, 4, 4, 1, *[None] * 5, False, 0, True)


def test_tag_rollout_inputs_stay_under_the_exclusion_cap():
    """On the reference side alone (oracle networks in float64 / float32, host Philox, the NumPy mirror): over the T steps of N
    environments, at most 2 % of the (row, agent) pairs sit within the exclusion margin of tests/rollout_ref.py."""
    import tag_rollout_ref as TR
    ref = TR.reference_rollout()
    near = np.concatenate([e.near for m in range(4) for e in ref["expected"][m]])
    assert near.mean() <= TR.NEAR_CAP, f"{near.sum()} of {near.size} (row, agent) pairs near a boundary"
    for m in range(4):
        assert len(np.unique(np.concatenate(ref["actions"][m]))) > 1, "an agent that only ever takes one action tests nothing"
