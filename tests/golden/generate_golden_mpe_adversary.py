#!/usr/bin/env python3
"""Generate tests/golden/mpe_adversary.npz by STEPPING the reference's own MPE `simple_adversary` (build container only): the parity
pin of the GPU-vectorised scenario (csrc/mpe_adv_core.h) and of its NumPy restatement (tests/mpe_adversary_np.py).

Run:  python tests/golden/generate_golden_mpe_adversary.py       (needs the reference checkout; writes the .npz here)

The stub modules, the env construction and the reproducible .npz writer are those of generate_golden_mpe.py.  Only data is written.
The scenario never sets world.world_length, so the env's time limit is set here on the env object (25, then 7).

num_agents = 3 (agent 0 the adversary, 1 and 2 good), 2 landmarks, every action a one-hot [5] of an index from RandomState(1000 + e).
  long/*    E = 12 episodes of episode_length 25 from np.random.seed(20 + e), stepped 25 times: done on the last step only
  short/*   E = 2 runs of episode_length 7 from np.random.seed(40 + e), stepped 14 times the way the vec-env wrapper does it: a
            step that returns done is followed by env.reset(), and the observation kept for that step is the reset's.  The state
            each reset left is recorded (reset_pos [E, 2, 3, 2], reset_lpos [E, 2, 2, 2], reset_goal [E, 2]: after steps 6 and 13)
  both:     pos0, vel0 [E, 3, 2], lpos [E, 2, 2], goal [E] (index k with `agents[0].goal_a is landmarks[k]`), obs0_adversary [E, 8],
            obs0_good1 / obs0_good2 [E, 10] (what reset returned), actions [E, T, 3], obs_adversary [E, T, 8], obs_good1 /
            obs_good2 [E, T, 10], rewards [E, T, 3] (one per agent), dones [E, T, 3]; long/ also pos1, vel1 [E, 3, 2], the state
            after the last step
float64, int32 (goal, actions) and bool (dones)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from generate_golden_mpe import OUT, install_stubs, make_env, write_npz  # noqa: E402

OBS = ("adversary", "good1", "good2")


def goal_index(env):
    return [k for k, l in enumerate(env.world.landmarks) if env.world.agents[0].goal_a is l][0]


def run(env, E, seed, steps, world_length, wrapper_reset):
    env.world_length = world_length
    rec = {}
    add = lambda k, v: rec.setdefault(k, []).append(v)
    for e in range(E):
        np.random.seed(seed + e)
        obs0 = env.reset()
        agents, landmarks = env.world.agents, env.world.landmarks
        add("pos0", [a.state.p_pos.copy() for a in agents]); add("vel0", [a.state.p_vel.copy() for a in agents])
        add("lpos", [l.state.p_pos.copy() for l in landmarks]); add("goal", goal_index(env))
        for m, name in enumerate(OBS):
            add("obs0_" + name, np.array(obs0[m], np.float64))
        rs = np.random.RandomState(1000 + e)
        ep = {k: [] for k in ("actions", "rewards", "dones", "reset_pos", "reset_lpos", "reset_goal") + tuple("obs_" + n for n in OBS)}
        for t in range(steps):
            idx = rs.randint(0, 5, 3)
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
    env = make_env("simple_adversary", 3, 2)
    assert [s.n for s in env.action_space] == [5, 5, 5] and not env.shared_reward
    out = {}
    for tag, res in (("long", run(env, 12, 20, 25, 25, False)), ("short", run(env, 2, 40, 14, 7, True))):
        out.update({f"{tag}/{k}": v for k, v in res.items()})
    assert sorted(np.unique(out["long/goal"])) == [0, 1]                                 # both goal indices occur
    assert sorted(np.unique(out["long/actions"])) == [0, 1, 2, 3, 4]                     # every move
    assert out["long/dones"][:, :-1].sum() == 0 and out["long/dones"][:, -1].all()       # dones on the last step only
    d = out["short/dones"]
    assert d[:, [6, 13]].all() and d.sum() == 2 * 2 * 3 and out["short/reset_pos"].shape == (2, 2, 3, 2)
    path = os.path.join(OUT, "mpe_adversary.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        print(f"  {k:22s} {out[k].dtype} {out[k].shape}")


if __name__ == "__main__":
    main()
