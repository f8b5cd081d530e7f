#!/usr/bin/env python3
"""Generate tests/golden/mpe_world_comm.npz by STEPPING the reference's own MPE `simple_world_comm` (build container only): the parity
pin of the GPU-vectorised scenario (csrc/mpe_world_comm_core.h) and of its NumPy restatement (tests/mpe_world_comm_np.py).

Run:  python tests/golden/generate_golden_mpe_world_comm.py       (needs the reference checkout; writes the .npz here)

The stub modules and the reproducible .npz writer are those of generate_golden_mpe.py; the env is built here, because this scenario
reads num_good_agents and num_adversaries.  Only data is written.  The env's time limit is set on the env object (10, then 5).

num_adversaries = 4 (agents 0..3, 0 the leader), num_good_agents = 2 (agents 4, 5), num_landmarks = 1 (+ 2 food, 2 forests).  Actions
are indices [7] — leader move, leader word, agents 1..5 — fed as the reference's one-hots: the leader's two heads side by side [9],
np.eye(5)[a] for the rest.
  long/*    E = 8 episodes of episode_length 10, stepped 10 times: done on the last step only.
            0..2: from np.random.seed(20 + e), indices from RandomState(1000 + e).
            3..7: SCRIPTED (see SCRIPTS): after reset() the positions, velocities and landmarks are set on the reference's own
            objects, and each agent holds one index or chases a target (the index that shortens the larger of |dx|, |dy|); the
            leader's (move, word) walks through all 5 x 4 pairs, step t of script k taking pair number 10 k + t (mod 20) — unless the
            script gives the leader a move, then only the word walks.  They make the reference itself step what random play does
            not reach: see the comment on each script
  short/*   E = 2 runs of episode_length 5 from np.random.seed(40 + e), stepped 10 times the way the vec-env wrapper does it: a
            step that returns done is followed by env.reset(), and the observation kept for that step is the reset's.  The state
            each reset left is recorded (reset_pos [E, 2, 6, 2], reset_lpos [E, 2, 5, 2]: after steps 4 and 9), and the stepped
            state each ended episode's last rewards came from (done_pos [E, 2, 6, 2])
  both:     pos0, vel0 [E, 6, 2], lpos [E, 5, 2], obs0_adv0 .. obs0_adv3 [E, 34], obs0_good0 / obs0_good1 [E, 28] (of the start state),
            actions [E, T, 7], obs_adv0 .. obs_adv3 [E, T, 34], obs_good0 / obs_good1 [E, T, 28], rewards [E, T, 6] (one per agent), dones
            [E, T, 6]; long/ also pos1, vel1 [E, 6, 2], the state after the last step
float64, int32 (actions) and bool (dones).

So that every flag in the file is well defined, the generator asserts that no is_collision the reference evaluated (good agent x
adversary, good agent x food, agent x forest) came within 1e-9 of its threshold (mpe_world_comm_np.margins)."""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True            # tests/golden/ is not covered by the __pycache__ ignore rule
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from generate_golden_mpe import OUT, install_stubs, write_npz  # noqa: E402
import mpe_world_comm_np as MW  # noqa: E402

OBS = MW.OBS
AWAY = [[-0.7, -0.7], [-0.7, 0.7], [-0.5, 0.7], [0.7, -0.7], [0.7, 0.7]]          # landmark, food x 2, forest x 2: out of everybody's way
# per agent: an index held for the episode | ("agent", j) / ("landmark", l): chase it.  Entry 0, the leader's MOVE, may be None: it
# then walks through the (move, word) pairs
SCRIPTS = [
    # adversary 1 pressed on landmark 0 from the left, adversary 2 and good agent 5 run into each other; good agent 4 leaves along +x
    # through the inside, linear and exp branches of bound()
    dict(pos=[[-0.6, -0.6], [-0.3, 0.0], [0.2, 0.6], [0.0, -0.5], [0.85, 0.2], [0.5, 0.61]], lpos=[[0.0, 0.0]] + AWAY[1:],
         act=[None, ("landmark", 0), ("agent", 5), 0, 1, ("agent", 2)]),
    # good agent 5 far outside along -y: the exp branch, then the capped one; good agent 4 walks over a food item
    dict(pos=[[0.0, 0.0], [-0.5, 0.5], [0.5, 0.5], [-0.5, -0.5], [0.1, 0.3], [0.3, -1.95]], lpos=[AWAY[0], [0.3, 0.3], [-0.8, 0.8]] + AWAY[3:],
         act=[None, 0, 0, 0, ("landmark", 1), 4]),
    # adversary 1 and good agent 4 rest in forest 0 and see each other; adversary 2, good agent 5 and the leader stand outside:
    # 2 and 5 see neither, the leader sees both; adversary 3 walks into the forest and starts seeing them
    dict(pos=[[-0.2, -0.2], [0.45, 0.5], [-0.5, 0.1], [0.0, 0.52], [0.6, 0.45], [-0.4, -0.6]],
         lpos=[AWAY[0], AWAY[1], AWAY[2], [0.5, 0.5], [-0.7, 0.75]], act=[None, 0, 0, 1, 0, 0]),
    # the forests overlap: adversary 1 rests inside both, good agent 4 inside forest 0 only, adversary 2 inside forest 1 only (1 sees
    # both, 4 and 2 do not see each other), good agent 5 crosses from outside through forest 1 into the overlap
    dict(pos=[[-0.5, -0.5], [0.5, 0.5], [0.95, 0.5], [-0.6, 0.3], [0.1, 0.5], [1.3, 0.45]],
         lpos=[AWAY[0], AWAY[1], AWAY[2], [0.35, 0.5], [0.7, 0.5]], act=[None, 0, 0, 0, 0, 2]),
    # the leader itself inside a forest with a start velocity, holding its move (only the word walks); everybody else outside
    dict(pos=[[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5], [0.0, 0.0], [-0.1, 0.9]], vel=[[0.3, 0.0]] + [[0.0, 0.0]] * 5,
         lpos=[AWAY[0], AWAY[1], AWAY[2], [0.55, 0.5], [-0.7, -0.75]], act=[3, 0, ("agent", 4), 0, 3, 3]),
]


def make_env():
    """What MPE_env.MPEEnv does, with the scenario module imported by name."""
    import importlib
    from onpolicy.envs.mpe.environment import MultiAgentEnv
    scenario = importlib.import_module("onpolicy.envs.mpe.scenarios.simple_world_comm").Scenario()
    args = types.SimpleNamespace(episode_length=25, num_agents=6, num_good_agents=2, num_adversaries=4, num_landmarks=1,
                                 scenario_name="simple_world_comm")
    world = scenario.make_world(args)
    return MultiAgentEnv(world, scenario.reset_world, scenario.reward, scenario.observation, scenario.info)


def chase(me, target):
    d = target - me
    if abs(d[0]) >= abs(d[1]):
        return 1 if d[0] > 0 else 2
    return 3 if d[1] > 0 else 4


def scripted_indices(env, act, pair):
    """-> [7]: leader move, leader word, agents 1..5.  pair: the number of the leader's (move, word) pair."""
    agents, landmarks = env.world.agents, env.world.landmarks
    idx = []
    for m, a in enumerate(act):
        if isinstance(a, tuple):
            t = (agents if a[0] == "agent" else landmarks)[a[1]]
            a = chase(agents[m].state.p_pos, t.state.p_pos)
        if m == 0:
            idx += [pair % 5 if a is None else a, (pair // 5) % 4]
        else:
            idx.append(a)
    return np.array(idx)


def feed(idx):
    return [np.concatenate([np.eye(5)[idx[0]], np.eye(4)[idx[1]]])] + [np.eye(5)[i] for i in idx[2:]]


def run(env, E, seed, steps, world_length, wrapper_reset, scripts=()):
    env.world_length = world_length
    rec = {}
    add = lambda k, v: rec.setdefault(k, []).append(v)
    for e in range(E + len(scripts)):
        np.random.seed(seed + e)
        obs0 = env.reset()
        agents, landmarks = env.world.agents, env.world.landmarks
        script = scripts[e - E] if e >= E else None
        if script:
            for m, a in enumerate(agents):
                a.state.p_pos = np.array(script["pos"][m], np.float64)
                a.state.p_vel = np.array(script.get("vel", np.zeros((6, 2)))[m], np.float64)
            for l, lm in enumerate(landmarks):
                lm.state.p_pos = np.array(script["lpos"][l], np.float64)
            obs0 = [env._get_obs(a) for a in agents]
        add("pos0", [a.state.p_pos.copy() for a in agents]); add("vel0", [a.state.p_vel.copy() for a in agents])
        add("lpos", [l.state.p_pos.copy() for l in landmarks])
        for m, name in enumerate(OBS):
            add("obs0_" + name, np.array(obs0[m], np.float64))
        rs = np.random.RandomState(1000 + e)
        ep = {k: [] for k in ("actions", "rewards", "dones", "reset_pos", "reset_lpos", "done_pos") + tuple("obs_" + n for n in OBS)}
        for t in range(steps):
            if script:
                idx = scripted_indices(env, script["act"], (e - E) * steps + t)
            else:
                idx = np.concatenate([[rs.randint(0, 5), rs.randint(0, 4)], rs.randint(0, 5, 5)])
            o, r, d, _ = env.step(feed(idx))
            if wrapper_reset and all(d):
                ep["done_pos"].append([a.state.p_pos.copy() for a in agents])
                o = env.reset()
                ep["reset_pos"].append([a.state.p_pos.copy() for a in agents])
                ep["reset_lpos"].append([l.state.p_pos.copy() for l in landmarks])
            ep["actions"].append(idx); ep["rewards"].append(np.asarray(r, np.float64)[:, 0]); ep["dones"].append(d)
            for m, name in enumerate(OBS):
                ep["obs_" + name].append(np.array(o[m], np.float64))
        for k, v in ep.items():
            if v:
                add(k, v)
        if not wrapper_reset:
            add("pos1", [a.state.p_pos.copy() for a in agents]); add("vel1", [a.state.p_vel.copy() for a in agents])
    return {k: np.asarray(v, dtype=np.int32 if k == "actions" else (np.bool_ if k == "dones" else np.float64)) for k, v in rec.items()}


def check_coverage(c):
    """Every branch the fixture claims (tests/test_mpe_world_comm.py asserts the same from the file)."""
    for k in ("hidden_observations", "forest_steps", "adversary_good_contact", "food_contact", "pressed_on_landmark", "bound_inside",
              "bound_linear", "bound_exp", "bound_capped", "pair_in_forest_third_outside", "in_both_forests", "leader_sees_hidden",
              "words_heard"):
        assert c[k] >= 1, (k, c)
    assert c["leader_actions"] == [(a, b) for a in range(5) for b in range(4)], c


def main():
    install_stubs()
    env = make_env()
    sp = env.action_space
    assert sp[0].__class__.__name__ == "MultiDiscrete" and list(sp[0].high) == [4, 3] and list(sp[0].low) == [0, 0]
    assert [s.n for s in sp[1:]] == [5] * 5 and not env.shared_reward
    assert [len(env._get_obs(a)) for a in env.world.agents] == list(MW.OBS_DIMS)
    assert env.share_observation_space[0].shape == (192,)
    out = {}
    for tag, res in (("long", run(env, 3, 20, 10, 10, False, SCRIPTS)), ("short", run(env, 2, 40, 10, 5, True))):
        out.update({f"{tag}/{k}": v for k, v in res.items()})
    assert out["long/dones"][:, :-1].sum() == 0 and out["long/dones"][:, -1].all()       # dones on the last step only
    d = out["short/dones"]
    assert d[:, [4, 9]].all() and d.sum() == 2 * 2 * 6 and out["short/reset_pos"].shape == (2, 2, 6, 2)
    for tag in ("long", "short"):
        m = MW.margins({k[len(tag) + 1:]: v for k, v in out.items() if k.startswith(tag + "/")})
        print(tag, "smallest |dist - dist_min|", m.min(), "of", m.size)
        assert m.min() > 1e-9, (tag, m.min())
    c = MW.coverage({k[5:]: v for k, v in out.items() if k.startswith("long/")})
    print(c)
    check_coverage(c)
    path = os.path.join(OUT, "mpe_world_comm.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        print(f"  {k:22s} {out[k].dtype} {out[k].shape}")


if __name__ == "__main__":
    main()
