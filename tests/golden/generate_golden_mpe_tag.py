#!/usr/bin/env python3
"""Generate tests/golden/mpe_tag.npz by STEPPING the reference's own MPE `simple_tag` (build container only): the parity pin of the
GPU-vectorised scenario (csrc/mpe_tag_core.h) and of its NumPy restatement (tests/mpe_tag_np.py).

Run:  python tests/golden/generate_golden_mpe_tag.py       (needs the reference checkout; writes the .npz here)

The stub modules and the reproducible .npz writer are those of generate_golden_mpe.py; the env is built here, because this scenario
reads num_good_agents and num_adversaries.  Only data is written.  The env's time limit is set on the env object (25, then 7).

num_adversaries = 3 (agents 0..2), num_good_agents = 1 (agent 3), 2 landmarks, every action the one-hot [5] of an index.
  long/*    E = 12 episodes of episode_length 25, stepped 25 times: done on the last step only.
            0..7: from np.random.seed(20 + e), indices from RandomState(1000 + e).
            8..11: SCRIPTED (see SCRIPTS): after reset() the positions, velocities and landmarks are set on the reference's own
            objects, and each agent holds one index or chases a target (the index that shortens the larger of |dx|, |dy|), so that
            the branches random play does not reach are stepped by the reference too: an adversary on the good agent, two at once,
            agents on landmarks, two adversaries on each other, the good agent far outside the arena
  short/*   E = 2 runs of episode_length 7 from np.random.seed(40 + e), stepped 14 times the way the vec-env wrapper does it: a
            step that returns done is followed by env.reset(), and the observation kept for that step is the reset's.  The state
            each reset left is recorded (reset_pos [E, 2, 4, 2], reset_lpos [E, 2, 2, 2]: after steps 6 and 13)
  both:     pos0, vel0 [E, 4, 2], lpos [E, 2, 2], obs0_adv0 / obs0_adv1 / obs0_adv2 [E, 16], obs0_good [E, 14] (of the start state),
            actions [E, T, 4], obs_adv0 / obs_adv1 / obs_adv2 [E, T, 16], obs_good [E, T, 14], rewards [E, T, 4] (one per agent), dones
            [E, T, 4]; long/ also pos1, vel1 [E, 4, 2], the state after the last step
float64, int32 (actions) and bool (dones)."""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True            # tests/golden/ is not covered by the __pycache__ ignore rule
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from generate_golden_mpe import OUT, install_stubs, write_npz  # noqa: E402
import mpe_tag_np as MT  # noqa: E402

OBS = MT.OBS
FAR = [[-0.7, -0.7], [0.7, -0.7]]
# per agent: an index held for the episode | ("agent", j) / ("landmark", l): chase it
SCRIPTS = [
    # two adversaries close in on a resting good agent from both sides: one contact, then two at once
    dict(pos=[[-0.4, 0.0], [0.33, 0.02], [0.8, 0.8], [0.0, 0.0]], lpos=FAR, act=[("agent", 3), ("agent", 3), 0, 0]),
    # two adversaries run into each other, the third into a landmark; the good agent leaves the arena along +x, far enough for the
    # capped branch of the boundary penalty
    dict(pos=[[-0.3, 0.0], [0.3, 0.01], [-0.2, 0.5], [0.85, 0.5]], lpos=[[-0.7, 0.5], [0.7, -0.7]],
         act=[("agent", 1), ("agent", 0), ("landmark", 0), 1]),
    # the good agent runs into a landmark with an adversary behind it; another leaves along -y with a start velocity
    dict(pos=[[-0.6, 0.1], [0.5, -0.8], [0.1, 0.9], [-0.3, 0.0]], vel=[[0, 0], [0.0, -0.5], [0, 0], [0.2, 0.0]], lpos=[[0.2, 0.0], [-0.7, -0.7]],
         act=[("agent", 3), 4, 3, ("landmark", 0)]),
    # the good agent outside along -y and back in, an adversary pressed against a landmark from above
    dict(pos=[[0.0, 0.6], [0.6, 0.6], [-0.6, 0.6], [0.1, -1.3]], lpos=[[0.0, 0.3], [0.7, -0.7]], act=[("landmark", 0), 2, 1, 3]),
]


def make_env():
    """What MPE_env.MPEEnv does, with the scenario module imported by name."""
    import importlib
    from onpolicy.envs.mpe.environment import MultiAgentEnv
    scenario = importlib.import_module("onpolicy.envs.mpe.scenarios.simple_tag").Scenario()
    args = types.SimpleNamespace(episode_length=25, num_agents=4, num_good_agents=1, num_adversaries=3, num_landmarks=2,
                                 scenario_name="simple_tag")
    world = scenario.make_world(args)
    return MultiAgentEnv(world, scenario.reset_world, scenario.reward, scenario.observation, scenario.info)


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
            t = (agents if a[0] == "agent" else landmarks)[a[1]]
            idx.append(chase(agents[m].state.p_pos, t.state.p_pos))
        else:
            idx.append(a)
    return np.array(idx)


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
                a.state.p_vel = np.array(script.get("vel", np.zeros((4, 2)))[m], np.float64)
            for l, lm in enumerate(landmarks):
                lm.state.p_pos = np.array(script["lpos"][l], np.float64)
            obs0 = [env._get_obs(a) for a in agents]
        add("pos0", [a.state.p_pos.copy() for a in agents]); add("vel0", [a.state.p_vel.copy() for a in agents])
        add("lpos", [l.state.p_pos.copy() for l in landmarks])
        for m, name in enumerate(OBS):
            add("obs0_" + name, np.array(obs0[m], np.float64))
        rs = np.random.RandomState(1000 + e)
        ep = {k: [] for k in ("actions", "rewards", "dones", "reset_pos", "reset_lpos") + tuple("obs_" + n for n in OBS)}
        for t in range(steps):
            idx = scripted_indices(env, script["act"]) if script else rs.randint(0, 5, 4)
            o, r, d, _ = env.step([np.eye(5)[i] for i in idx])
            if wrapper_reset and all(d):
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
    """Every branch the fixture claims (tests/test_mpe_tag.py asserts the same from the file)."""
    for k in ("one_contact", "two_contacts", "adversary_landmark", "good_landmark", "adversary_adversary", "adversary_clamped", "good_clamped",
              "adversary_unclamped", "good_unclamped", "bound_inside", "bound_linear", "bound_exp", "bound_capped"):
        assert c[k] >= 1, (k, c)
    assert c["actions"] == [0, 1, 2, 3, 4], c


def main():
    install_stubs()
    env = make_env()
    assert [s.n for s in env.action_space] == [5, 5, 5, 5] and not env.shared_reward
    assert [len(env._get_obs(a)) for a in env.world.agents] == list(MT.OBS_DIMS)
    out = {}
    for tag, res in (("long", run(env, 8, 20, 25, 25, False, SCRIPTS)), ("short", run(env, 2, 40, 14, 7, True))):
        out.update({f"{tag}/{k}": v for k, v in res.items()})
    assert out["long/dones"][:, :-1].sum() == 0 and out["long/dones"][:, -1].all()       # dones on the last step only
    d = out["short/dones"]
    assert d[:, [6, 13]].all() and d.sum() == 2 * 2 * 4 and out["short/reset_pos"].shape == (2, 2, 4, 2)
    c = MT.coverage({k[5:]: v for k, v in out.items() if k.startswith("long/")})
    print(c)
    check_coverage(c)
    path = os.path.join(OUT, "mpe_tag.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        print(f"  {k:22s} {out[k].dtype} {out[k].shape}")


if __name__ == "__main__":
    main()
