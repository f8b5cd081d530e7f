#!/usr/bin/env python3
"""Generate tests/golden/mpe_push.npz by STEPPING the reference's own MPE `simple_push` (build container only): the parity pin of
the GPU-vectorised scenario (csrc/mpe_push_core.h) and of its NumPy restatement (tests/mpe_push_np.py).

Run:  python tests/golden/generate_golden_mpe_push.py       (needs the reference checkout; writes the .npz here)

The stub modules, the env construction and the reproducible .npz writer are those of generate_golden_mpe.py.  Only data is written.
The scenario never sets world.world_length, so the env's time limit is set here on the env object (25, then 7).

num_agents = 2 (agent 0 the adversary, agent 1 the good agent), 2 landmarks, every action the one-hot [5] of an index.
  long/*     E = 12 episodes of episode_length 25 from np.random.seed(20 + e), indices from RandomState(1000 + e), stepped 25 times:
             done on the last step only
  short/*    E = 2 runs of episode_length 7 from np.random.seed(40 + e), stepped 14 times the way the vec-env wrapper does it: a
             step that returns done is followed by env.reset(), and the observation kept for that step is the reset's.  The state
             each reset left is recorded (reset_pos [E, 2, 2, 2], reset_lpos [E, 2, 2, 2], reset_goal [E, 2]: after steps 6 and 13)
  contact/*  E = 6 SCRIPTED episodes of episode_length 25 (see SCRIPTS): after reset() from np.random.seed(60 + e) the positions,
             velocities and landmarks are set on the reference's own objects (the goal stays the one reset drew), and each agent
             holds one index or chases a target (the index that shortens the larger of |dx|, |dy|).  The first three START with the
             two agents inside each other's contact distance, at rest, pressed together and flying apart; in the others the actions
             drive them into each other.  The contact force is what random play from U(-1,1)^2 almost never reaches
  all:       pos0, vel0 [E, 2, 2], lpos [E, 2, 2], goal [E] (index k with `agents[0].goal_a is landmarks[k]`), obs0_adversary [E, 8],
             obs0_good [E, 19] (of the start state), actions [E, T, 2], obs_adversary [E, T, 8], obs_good [E, T, 19], rewards
             [E, T, 2] (one per agent), dones [E, T, 2]; long/ and contact/ also pos1, vel1 [E, 2, 2], the state after the last step
float64, int32 (goal, actions) and bool (dones)."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True            # tests/golden/ is not covered by the __pycache__ ignore rule
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from generate_golden_mpe import OUT, install_stubs, make_env, write_npz  # noqa: E402
import mpe_push_np as MP  # noqa: E402

OBS = MP.OBS
# per agent: an index held for the episode | ("agent", j) / ("landmark", l) / ("goal",): chase it
SCRIPTS = [
    # inside each other at rest, nobody pushes: the contact force alone drives them apart
    dict(pos=[[0.0, 0.0], [0.06, 0.02]], lpos=[[0.5, 0.5], [-0.5, 0.4]], act=[0, 0]),
    # inside each other and pushing against each other for the whole episode
    dict(pos=[[-0.04, 0.0], [0.04, 0.01]], lpos=[[0.6, -0.5], [-0.5, 0.4]], act=[("agent", 1), ("agent", 0)]),
    # deep inside each other with velocities, the good agent makes for the goal with the adversary after it
    dict(pos=[[0.1, 0.1], [0.11, 0.13]], vel=[[0.3, 0.0], [-0.2, 0.1]], lpos=[[0.4, 0.1], [-0.3, 0.2]], act=[("agent", 1), ("goal",)]),
    # apart, head on along x
    dict(pos=[[-0.5, 0.0], [0.5, 0.03]], lpos=[[0.0, 0.6], [0.0, -0.6]], act=[("agent", 1), ("agent", 0)]),
    # both make for the goal from opposite sides and meet on it
    dict(pos=[[-0.45, 0.02], [0.4, -0.03]], lpos=[[0.0, 0.0], [0.01, -0.01]], act=[("goal",), ("goal",)]),
    # the adversary runs down a good agent that drifts along +y
    dict(pos=[[0.0, -0.6], [0.02, 0.0]], vel=[[0.0, 0.0], [0.0, 0.1]], lpos=[[0.7, 0.7], [-0.7, 0.7]], act=[("agent", 1), 0]),
]


def goal_index(env):
    return [k for k, l in enumerate(env.world.landmarks) if env.world.agents[0].goal_a is l][0]


def chase(me, target):
    d = target - me
    if abs(d[0]) >= abs(d[1]):
        return 1 if d[0] > 0 else 2
    return 3 if d[1] > 0 else 4


def scripted_indices(env, act):
    agents, landmarks = env.world.agents, env.world.landmarks
    idx = []
    for m, a in enumerate(act):
        if isinstance(a, tuple):
            t = agents[m].goal_a if a[0] == "goal" else (agents if a[0] == "agent" else landmarks)[a[1]]
            idx.append(chase(agents[m].state.p_pos, t.state.p_pos))
        else:
            idx.append(a)
    return np.array(idx)


def run(env, E, seed, steps, world_length, wrapper_reset, scripts=None):
    env.world_length = world_length
    rec = {}
    add = lambda k, v: rec.setdefault(k, []).append(v)
    for e in range(E):
        np.random.seed(seed + e)
        obs0 = env.reset()
        agents, landmarks = env.world.agents, env.world.landmarks
        script = scripts[e] if scripts else None
        if script:
            for m, a in enumerate(agents):
                a.state.p_pos = np.array(script["pos"][m], np.float64)
                a.state.p_vel = np.array(script.get("vel", np.zeros((2, 2)))[m], np.float64)
            for l, lm in enumerate(landmarks):
                lm.state.p_pos = np.array(script["lpos"][l], np.float64)
            obs0 = [env._get_obs(a) for a in agents]
        add("pos0", [a.state.p_pos.copy() for a in agents]); add("vel0", [a.state.p_vel.copy() for a in agents])
        add("lpos", [l.state.p_pos.copy() for l in landmarks]); add("goal", goal_index(env))
        for m, name in enumerate(OBS):
            add("obs0_" + name, np.array(obs0[m], np.float64))
        rs = np.random.RandomState(1000 + e)
        ep = {k: [] for k in ("actions", "rewards", "dones", "reset_pos", "reset_lpos", "reset_goal") + tuple("obs_" + n for n in OBS)}
        for t in range(steps):
            idx = scripted_indices(env, script["act"]) if script else rs.randint(0, 5, 2)
            o, r, d, _ = env.step([np.eye(5)[i] for i in idx])
            if wrapper_reset and all(d):
                o = env.reset()
                ep["reset_pos"].append([a.state.p_pos.copy() for a in agents])
                ep["reset_lpos"].append([l.state.p_pos.copy() for l in landmarks])
                ep["reset_goal"].append(goal_index(env))
            ep["actions"].append(idx); ep["rewards"].append(np.asarray(r, np.float64)[:, 0]); ep["dones"].append(d)
            for m, name in enumerate(OBS):
                ep["obs_" + name].append(np.array(o[m], np.float64))
        for k, v in ep.items():
            if v:
                add(k, v)
        if not wrapper_reset:
            add("pos1", [a.state.p_pos.copy() for a in agents]); add("vel1", [a.state.p_vel.copy() for a in agents])
    ints = ("actions", "goal", "reset_goal")
    return {k: np.asarray(v, dtype=np.int32 if k in ints else (np.bool_ if k == "dones" else np.float64)) for k, v in rec.items()}


def main():
    install_stubs()
    env = make_env("simple_push", 2, 2)
    assert [s.n for s in env.action_space] == [5, 5] and not env.shared_reward
    assert [len(env._get_obs(a)) for a in env.world.agents] == list(MP.OBS_DIMS)
    out = {}
    for tag, res in (("long", run(env, 12, 20, 25, 25, False)), ("short", run(env, 2, 40, 14, 7, True)),
                     ("contact", run(env, len(SCRIPTS), 60, 25, 25, False, SCRIPTS))):
        out.update({f"{tag}/{k}": v for k, v in res.items()})
    group = lambda tag: {k[len(tag) + 1:]: v for k, v in out.items() if k.startswith(tag + "/")}
    for tag in ("long", "contact"):
        assert sorted(np.unique(out[tag + "/goal"])) == [0, 1], tag                      # both goal indices occur
    assert sorted(np.unique(np.concatenate([out["short/goal"], out["short/reset_goal"].reshape(-1)]))) == [0, 1]
    assert sorted(np.unique(out["long/actions"])) == [0, 1, 2, 3, 4]                     # every move
    assert sorted(np.unique(out["contact/actions"])) == [0, 1, 2, 3, 4]
    for tag in ("long", "contact"):
        assert out[tag + "/dones"][:, :-1].sum() == 0 and out[tag + "/dones"][:, -1].all()   # dones on the last step only
    d = out["short/dones"]
    assert d[:, [6, 13]].all() and d.sum() == 2 * 2 * 2 and out["short/reset_pos"].shape == (2, 2, 2, 2)
    c = group("contact")
    start, after = MP.in_contact(c["pos0"]), MP.in_contact(MP.positions_after(c))
    print("contact/: start in contact", start.astype(int), "steps in contact per episode", after.sum(1))
    assert start[:3].all() and not start[3:].any()                                        # three start inside, three are driven in
    assert (start | (after.sum(1) >= 1)).all() and (after[3:].sum(1) >= 1).all()          # the driven ones record steps in contact
    path = os.path.join(OUT, "mpe_push.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        print(f"  {k:22s} {out[k].dtype} {out[k].shape}")


if __name__ == "__main__":
    main()
