"""MPE simple_world_comm without a GPU: the fixture stepped by the reference's own environment (tests/golden/mpe_world_comm.npz)
reaches every branch it claims and keeps every contact and forest flag away from its threshold, the NumPy mirror
(tests/mpe_world_comm_np.py) EQUALS it — the reset-on-done boundary of the 5-step runs included —, the vec-env, `ops` and the C ABI
refuse by name what they are not built for, and the separated runner's action packing equals the reference's formula."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
import mpe_world_comm_np as MW

OBS = MW.OBS
E_LONG, T_LONG, E_SHORT, T_SHORT, LEN_SHORT = 8, 10, 2, 10, 5


def _fx(tag):
    g = golden("mpe_world_comm")
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "/")}


def test_fixture_covers_what_it_claims():
    lo, sh = _fx("long"), _fx("short")
    assert lo["actions"].shape == (E_LONG, T_LONG, 7) and sh["actions"].shape == (E_SHORT, T_SHORT, 7)
    assert lo["dones"][:, :-1].sum() == 0 and lo["dones"][:, -1].all()
    assert sh["dones"][:, [4, 9]].all() and sh["dones"].sum() == 2 * 2 * 6
    assert sh["reset_pos"].shape == sh["done_pos"].shape == (2, 2, 6, 2) and sh["reset_lpos"].shape == (2, 2, 5, 2)
    for n, d in zip(OBS, MW.OBS_DIMS):
        assert lo["obs_" + n].shape == (E_LONG, T_LONG, d) and lo["obs0_" + n].shape == (E_LONG, d)
    assert lo["rewards"].shape == (E_LONG, T_LONG, 6) and lo["rewards"].dtype == np.float64
    assert (lo["actions"][..., 0] <= 4).all() and (lo["actions"][..., 1] <= 3).all() and lo["actions"].min() == 0
    c = MW.coverage(lo)
    print(c)
    # what random play reaches anyway: hidden agents, forests, an adversary on a good agent, a good agent on food
    for k in ("hidden_observations", "forest_steps", "adversary_good_contact", "food_contact"):
        assert c[k] >= 1, (k, c)
    # what is scripted: an agent pressed on landmark 0; every branch of bound(): |x| < 0.9, [0.9, 1), [1, 1 + ln(10) / 2], beyond the cap
    for k in ("pressed_on_landmark", "bound_inside", "bound_linear", "bound_exp", "bound_capped"):
        assert c[k] >= 1, (k, c)
    # two agents in one forest see each other while a third outside sees neither; an agent inside both forests; the leader sees an
    # agent the forest rule alone would hide from it
    for k in ("pair_in_forest_third_outside", "in_both_forests", "leader_sees_hidden"):
        assert c[k] >= 1, (k, c)
    assert c["leader_actions"] == [(a, b) for a in range(5) for b in range(4)]          # every one of the 5 x 4 leader actions
    assert c["words_heard"] == 4 * E_LONG * T_LONG                                      # a one-hot word in every adversary's observation
    # the capped branch costs 2 x 10 for its coordinate; the food term gives back 0.05 x a distance of a few units at the most
    r, x = lo["rewards"], np.abs(np.stack([lo["obs_good0"][..., 2:4], lo["obs_good1"][..., 2:4]], axis=2))
    capped = x.max(-1) > 1 + np.log(10) / 2
    assert capped.any() and (r[..., 4:][capped] <= -19.5).all()
    # at reset nothing has been said
    for tag in (lo, sh):
        for n in OBS[:4]:
            assert (tag["obs0_" + n][:, MW.COMM] == 0).all()
    for e in range(E_SHORT):
        for t in (4, 9):
            for n in OBS[:4]:
                assert (sh["obs_" + n][e, t, MW.COMM] == 0).all()


def test_no_flag_of_the_fixture_sits_on_its_threshold():
    """For every is_collision the reference evaluated (good agent x adversary, good agent x food, agent x forest), |dist - dist_min| >
    1e-9, from the recorded states: a float64 kernel whose exp / log1p differ from NumPy's in the last place cannot flip any of them,
    so no test needs to leave a case out."""
    for tag in ("long", "short"):
        m = MW.margins(_fx(tag))
        print(tag, "smallest margin", m.min(), "of", m.size)
        assert m.size >= 500 and m.min() > 1e-9, (tag, m.min())


@pytest.mark.parametrize("onehot", [True, False], ids=["onehot", "index"])
def test_numpy_mirror_equals_reference_long_episodes(onehot):
    g = _fx("long")
    env = MW.SimpleWorldCommNp(g["pos0"], g["vel0"], g["lpos"], episode_length=T_LONG)
    for m, o in enumerate(env.obs()):
        np.testing.assert_array_equal(o, g["obs0_" + OBS[m]])
    for t in range(T_LONG):
        a = g["actions"][:, t]
        obs, rew, dones = env.step(MW.onehots(a) if onehot else a)
        for m in range(6):
            np.testing.assert_array_equal(obs[m], g["obs_" + OBS[m]][:, t], err_msg=f"obs of agent {m}, step {t}")
        np.testing.assert_array_equal(rew, g["rewards"][:, t], err_msg=f"rewards, step {t}")
        np.testing.assert_array_equal(dones, g["dones"][:, t])
    np.testing.assert_array_equal(env.pos, g["pos1"])
    np.testing.assert_array_equal(env.vel, g["vel1"])


@pytest.mark.parametrize("onehot", [True, False], ids=["onehot", "index"])
def test_numpy_mirror_equals_reference_across_reset_on_done(onehot):
    """episode_length 5, 10 steps: the steps that end an episode return the reset's observations (state reloaded from the fixture,
    nothing said) and the ended step's rewards; the next episode continues from the reloaded state at rest."""
    g = _fx("short")
    env = MW.SimpleWorldCommNp(g["pos0"], g["vel0"], g["lpos"], episode_length=LEN_SHORT)
    resets = 0
    for t in range(T_SHORT):
        a = g["actions"][:, t]
        obs, rew, dones = env.step(MW.onehots(a) if onehot else a)
        np.testing.assert_array_equal(dones, g["dones"][:, t])
        np.testing.assert_array_equal(rew, g["rewards"][:, t], err_msg=f"rewards, step {t}")
        if dones.all():
            np.testing.assert_array_equal(env.pos, g["done_pos"][:, resets])
            env.reload(np.arange(E_SHORT), g["reset_pos"][:, resets], g["reset_lpos"][:, resets])
            obs = env.obs()
            resets += 1
        else:
            assert not dones.any()
        for m in range(6):
            np.testing.assert_array_equal(obs[m], g["obs_" + OBS[m]][:, t], err_msg=f"obs of agent {m}, step {t}")
    assert resets == 2


def test_rewards_are_per_agent():
    """The adversaries share the contact term but not the distance term, and each good agent has its own: a summed or shared reward
    would make all six equal."""
    r = _fx("long")["rewards"]
    assert (r[..., 0] != r[..., 1]).any() and (r[..., 4] != r[..., 5]).any() and (r[..., 0] != r[..., 4]).any()
    hit = r[..., :4].max(-1) > 4                                     # some (good, adversary) pair in contact: +5 for EVERY adversary
    assert hit.any() and (r[..., :4][hit] > 3).all()


def test_vec_env_and_ops_refuse_other_shapes_by_name_without_a_device():
    import torch
    from mappo_amd import ops
    from mappo_amd.envs import SimpleWorldCommVecEnv
    for n in (4, 5, 7):
        with pytest.raises(ValueError, match="simple_world_comm is built for num_agents = 6"):
            SimpleWorldCommVecEnv(4, num_agents=n, device="cuda:7")
        with pytest.raises(ValueError, match="mpe_world_comm_reset: simple_world_comm is built for num_agents = 6"):
            ops.mpe_world_comm_reset(*[None] * 6, 4, 1, num_agents=n)
        with pytest.raises(ValueError, match="mpe_world_comm_step: simple_world_comm is built for num_agents = 6"):
            ops.mpe_world_comm_step(*[None] * 6, 1, *[None] * 3, 4, 25, 1, num_agents=n)
    for kw in (dict(num_adversaries=3), dict(num_good_agents=1), dict(num_landmarks=2), dict(num_landmarks=0)):
        with pytest.raises(ValueError, match=r"4 adversaries \(the first their leader\), 2 good agents, 1 landmark"):
            SimpleWorldCommVecEnv(4, device="cuda:7", **kw)
        with pytest.raises(ValueError, match="mpe_world_comm_reset: .*4 adversaries .*2 good agents, 1 landmark"):
            ops.mpe_world_comm_reset(*[None] * 6, 4, 1, **kw)
        with pytest.raises(ValueError, match="mpe_world_comm_step: .*4 adversaries .*2 good agents, 1 landmark"):
            ops.mpe_world_comm_step(*[None] * 6, 1, *[None] * 3, 4, 25, 1, **kw)
    env = SimpleWorldCommVecEnv(4, device="cpu")
    assert env.observation_space == [[34]] * 4 + [[28]] * 2 and env.share_observation_space == [[192]] * 6
    sp = env.action_space
    assert sp[0].__class__.__name__ == "MultiDiscrete" and list(sp[0].low) == [0, 0] and list(sp[0].high) == [4, 3] and sp[0].shape == 2
    assert [s.__class__.__name__ for s in sp[1:]] == ["Discrete"] * 5 and [s.n for s in sp[1:]] == [5] * 5
    assert env.graph_safe and env.accepts_device_actions and env.accepts_index_actions and env.consumes_actions and env.ragged_obs
    assert env.accepts_multidiscrete_agents and not hasattr(env, "episode_launch")
    assert set(env.state_tensors()) == {"agent_pos", "agent_vel", "landmark_pos", "tstep", "episode"}
    st = env.state_tensors()
    assert tuple(st["agent_pos"].shape) == (4, 6, 2) and tuple(st["landmark_pos"].shape) == (4, 5, 2) and st["episode"].dtype == torch.int64
    # the forms of `actions`
    hot = [torch.zeros(4, 9)] + [torch.zeros(4, 5)] * 5
    mode, act = env._parse_actions(hot)
    assert mode == 0 and [tuple(x.shape) for x in act] == [(4, 9)] + [(4, 5)] * 5
    idx = torch.arange(28, dtype=torch.float32).reshape(4, 7)
    mode, act = env._parse_actions(idx)
    assert mode == 1 and torch.equal(act, idx)
    mode, act = env._parse_actions([idx[:, :2]] + [idx[:, 2 + m] for m in range(5)])
    assert mode == 1 and torch.equal(act, idx)
    mode, act = env._parse_actions([idx[:, :2]] + [idx[:, 2 + m:3 + m] for m in range(5)])
    assert mode == 1 and torch.equal(act, idx)
    for bad in (torch.zeros(4, 6), torch.zeros(4, 6, 5), [torch.zeros(4, 5)] * 6, hot[:5], [torch.zeros(4)] * 6, torch.zeros(3, 7)):
        with pytest.raises(ValueError, match=r"SimpleWorldCommVecEnv.step: .*\[N, 9\].*\[N, 5\] x 5.*\[N, 7\]"):
            env.step(bad)


def test_the_envs_without_a_multidiscrete_agent_parse_actions_as_before():
    """SimpleWorldCommVecEnv brings its own _parse_actions; the shared one is untouched."""
    import torch
    from mappo_amd.envs import SimpleTagVecEnv
    env = SimpleTagVecEnv(4, device="cpu")
    assert not getattr(env, "accepts_multidiscrete_agents", False)
    mode, act = env._parse_actions(torch.zeros(4, 4))
    assert mode == 1 and tuple(act.shape) == (4, 4)
    mode, act = env._parse_actions([torch.zeros(4, 5)] * 4)
    assert mode == 0 and tuple(act.shape) == (4, 4, 5)


# ---- the separated runner's action packing ---------------------------------------------------------------------------------------------
def test_pack_actions_equals_the_reference_formula_on_cpu_tensors():
    """separated/mpe_runner.py:118-124 of the reference: np.eye(high_i + 1)[action[:, i]] of a MultiDiscrete agent's heads side by
    side, np.eye(n)[a] for a Discrete one; and the index form [N, 7] in the order leader move, leader word, agents 1..5."""
    import torch
    from mappo_amd.envs import SimpleWorldCommVecEnv
    from mappo_amd.runner.separated.mpe_runner import pack_actions
    N = 23
    rs = np.random.RandomState(5)
    lead = np.stack([rs.randint(0, 5, N), rs.randint(0, 4, N)], axis=1)
    lead[:4] = [[0, 0], [4, 3], [4, 0], [0, 3]]                      # the corners of the leader's space
    rest = [rs.randint(0, 5, N) for _ in range(5)]
    spaces = SimpleWorldCommVecEnv(N, device="cpu").action_space
    high = spaces[0].high
    want = [np.concatenate([np.eye(high[i] + 1)[lead[:, i]] for i in range(2)], axis=1)] + [np.eye(5)[a] for a in rest]
    for shape in ((N,), (N, 1)):
        acts = [torch.from_numpy(lead)] + [torch.from_numpy(a).reshape(shape) for a in rest]
        got = pack_actions(acts, spaces, False)
        assert len(got) == 6 and [tuple(x.shape) for x in got] == [(N, 9)] + [(N, 5)] * 5
        for m in range(6):
            assert got[m].dtype == torch.float32
            np.testing.assert_array_equal(got[m].numpy(), want[m].astype(np.float32), err_msg=f"agent {m}")
        idx = pack_actions(acts, spaces, True)
        assert idx.dtype == torch.float32 and tuple(idx.shape) == (N, 7)
        np.testing.assert_array_equal(idx.numpy(), np.concatenate([lead, np.stack(rest, axis=1)], axis=1).astype(np.float32))
    # fp32 index tensors, as the buffers hold them, pack the same
    got = pack_actions([torch.from_numpy(lead).float()] + [torch.from_numpy(a).float() for a in rest], spaces, False)
    for m in range(6):
        np.testing.assert_array_equal(got[m].numpy(), want[m].astype(np.float32))
    # the mirror's own restatement agrees
    for m, x in enumerate(MW.onehots(idx.numpy())):
        np.testing.assert_array_equal(x, want[m])
    with pytest.raises(ValueError, match="pack_actions: 1 action columns for MultiDiscrete"):
        pack_actions([torch.from_numpy(lead[:, 0])] + [torch.from_numpy(a) for a in rest], spaces, False)


# ---- the C ABI refuses what the kernels are not built for, before any launch -------------------------------------------------------
P = C.c_void_p(4096)                          # never dereferenced: the checks come before any launch


def _arr(ptr, n=6, hole=None):
    return (C.c_void_p * n)(*[None if (ptr is None or m == hole) else ptr.value for m in range(n)])


def test_mpe_world_comm_reset_and_step_reject():
    from mappo_amd import _lib
    lib = _lib.load()
    assert lib.mappo_abi_version() >= 12

    def reset(N=4, M=6, L=1, ptr=P, obs="full"):
        o = None if obs is None else _arr(P, hole=obs if isinstance(obs, int) else None)
        return lib.mappo_mpe_world_comm_reset(ptr, ptr, ptr, ptr, ptr, o, N, M, L, 1, None), lib.mappo_last_error().decode()

    def step(N=4, M=6, L=1, mode=1, env_T=6, ptr=P, obs="full", act="full"):
        o = None if obs is None else _arr(P, hole=obs if isinstance(obs, int) else None)
        a = None if act is None else _arr(P, hole=act if isinstance(act, int) else None)
        return (lib.mappo_mpe_world_comm_step(ptr, ptr, ptr, ptr, ptr, a, mode, o, ptr, ptr, N, M, L, env_T, 1, None),
                lib.mappo_last_error().decode())

    common = [(dict(N=0), ["N=0", "N >= 1"]), (dict(M=5), ["num_agents=5", "num_agents = 6"]), (dict(M=7), ["num_agents=7", "num_agents = 6"]),
              (dict(M=4), ["num_agents=4", "num_agents = 6"]), (dict(L=2), ["num_landmarks=2", "num_landmarks = 1"]),
              (dict(L=0), ["num_landmarks=0", "num_landmarks = 1"]), (dict(ptr=None), ["null pointer"]), (dict(obs=None), ["null pointer"]),
              (dict(obs=5), ["null pointer"])]
    for call, who, cases in ((reset, "mpe_world_comm_reset", common),
                             (step, "mpe_world_comm_step", common + [(dict(mode=2), ["action_mode 2"]), (dict(mode=-1), ["action_mode -1"]),
                                                                     (dict(env_T=0), ["episode length 0"]), (dict(act=None), ["null pointer"]),
                                                                     (dict(act=0), ["null pointer"]),
                                                                     (dict(act=3, mode=0), ["null pointer", "actions[3]"])])):
        for kw, words in cases:
            rc, err = call(**kw)
            assert rc == -1, (who, kw, rc)
            assert who in err, err
            for w in words:
                assert w in err, (who, kw, err)


def test_host_reset_draws_follow_the_index_rule():
    """The host restatement of the reset draws (what the GPU reset is held against): agents in [-1, 1), landmarks in 0.8 [-1, 1), no
    index shared, another stream per episode."""
    pos, lpos = MW.reset_draws(7, 1, 37)
    assert pos.shape == (37, 6, 2) and lpos.shape == (37, 5, 2)
    assert (pos >= -1).all() and (pos < 1).all() and (np.abs(lpos) <= 0.8).all() and np.abs(lpos).max() > 0.7
    allv = np.concatenate([pos.reshape(-1), lpos.reshape(-1) / 0.8])
    assert len(np.unique(allv)) == allv.size
    p2, _ = MW.reset_draws(7, 2, 37)
    assert not np.array_equal(pos, p2)
    # environment n draws at 32 n + k: the first environment of a 37-wide reset is the only environment of a 1-wide one
    p1, l1 = MW.reset_draws(7, 1, 1)
    np.testing.assert_array_equal(p1[0], pos[0]); np.testing.assert_array_equal(l1[0], lpos[0])
