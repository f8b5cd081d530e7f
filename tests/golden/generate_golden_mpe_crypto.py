#!/usr/bin/env python3
"""Generate tests/golden/mpe_crypto.npz by STEPPING the reference's own MPE `simple_crypto` (build container only): the parity pin
of the GPU-vectorised scenario (csrc/mpe_crypto_core.h) and of its NumPy restatement (tests/mpe_crypto_np.py).

Run:  python tests/golden/generate_golden_mpe_crypto.py       (needs the reference checkout; writes the .npz here)

The stub modules, the env construction and the reproducible .npz writer are those of generate_golden_mpe.py.  Only data is written.
The scenario never sets world.world_length, so the env's time limit is set here on the env object (25, then 7).

num_agents = 3 (agent 0 Eve the adversary, 1 Bob the good listener, 2 Alice the speaker); num_landmarks 2 and 4, one env each; every
action a one-hot [4] of an index from RandomState(1000 + e).
  long/*    E = 24 episodes of episode_length 25 from np.random.seed(20 + e), stepped 25 times: done on the last step only.
            Episodes 0 .. 11 have 2 landmarks, 12 .. 23 have 4
  short/*   E = 2 runs of episode_length 7 from np.random.seed(40 + e), stepped 14 times the way the vec-env wrapper does it: a
            step that returns done is followed by env.reset(), and the observation kept for that step is the reset's.  The state
            each reset left is recorded (reset_goal, reset_key [E, 2]: after steps 6 and 13).  Run 0 has 2 landmarks, run 1 has 4
  both:     num_landmarks [E], goal [E] (index k with `agents[0].goal_a is landmarks[k]`), key [E] (index k with the speaker's key
            being landmark k's colour e_k), obs0_eve [E, 4], obs0_bob / obs0_alice [E, 8] (what reset returned), actions [E, T, 3],
            obs_eve [E, T, 4], obs_bob / obs_alice [E, T, 8], rewards [E, T, 3] (one per agent), dones [E, T, 3]
float64, int32 (num_landmarks, goal, key, actions) and bool (dones)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from generate_golden_mpe import OUT, install_stubs, make_env, write_npz  # noqa: E402

OBS = ("eve", "bob", "alice")
INTS = ("num_landmarks", "actions", "goal", "key", "reset_goal", "reset_key")


def goal_index(env):
    return [k for k, l in enumerate(env.world.landmarks) if env.world.agents[0].goal_a is l][0]


def key_index(env):
    key = env.world.agents[2].key
    assert key.shape == (4,) and key.sum() == 1 and key.max() == 1
    return int(np.argmax(key))


def run(env, episodes, seed, steps, world_length, wrapper_reset):
    env.world_length = world_length
    rec = {}
    add = lambda k, v: rec.setdefault(k, []).append(v)
    for e in episodes:
        np.random.seed(seed + e)
        obs0 = env.reset()
        add("num_landmarks", len(env.world.landmarks)); add("goal", goal_index(env)); add("key", key_index(env))
        for m, name in enumerate(OBS):
            add("obs0_" + name, np.array(obs0[m], np.float64))
        rs = np.random.RandomState(1000 + e)
        ep = {k: [] for k in ("actions", "rewards", "dones", "reset_goal", "reset_key") + tuple("obs_" + n for n in OBS)}
        for t in range(steps):
            idx = rs.randint(0, 4, 3)
            o, r, d, _ = env.step([np.eye(4)[i] for i in idx])
            if wrapper_reset and all(d):
                o = env.reset()
                ep["reset_goal"].append(goal_index(env)); ep["reset_key"].append(key_index(env))
            ep["actions"].append(idx); ep["rewards"].append(np.asarray(r, np.float64)[:, 0]); ep["dones"].append(d)
            for m, name in enumerate(OBS):
                ep["obs_" + name].append(np.array(o[m], np.float64))
        for k, v in ep.items():
            if v:
                add(k, v)
    return rec


def main():
    install_stubs()
    envs = {L: make_env("simple_crypto", 3, L) for L in (2, 4)}
    for env in envs.values():
        assert [s.n for s in env.action_space] == [4, 4, 4] and not env.shared_reward
    out = {}
    for tag, E, args in (("long", 24, (20, 25, 25, False)), ("short", 2, (40, 14, 7, True))):
        rec = {}
        for half, L in enumerate((2, 4)):
            for k, v in run(envs[L], range(half * E // 2, (half + 1) * E // 2), *args).items():
                rec.setdefault(k, []).extend(v)
        out.update({f"{tag}/{k}": np.asarray(v, dtype=np.int32 if k in INTS else (np.bool_ if k == "dones" else np.float64))
                    for k, v in rec.items()})
    lo, sh = {k[5:]: v for k, v in out.items() if k.startswith("long/")}, {k[6:]: v for k, v in out.items() if k.startswith("short/")}
    assert lo["num_landmarks"].tolist() == [2] * 12 + [4] * 12 and sh["num_landmarks"].tolist() == [2, 4]
    for m in range(3):
        assert sorted(np.unique(lo["actions"][..., m])) == [0, 1, 2, 3]                  # every agent says every symbol
    for k in ("goal", "key"):                                                            # every goal and key index occurs
        assert sorted(np.unique(lo[k][:12])) == [0, 1] and sorted(np.unique(lo[k][12:])) == [0, 1, 2, 3]
    assert (lo["goal"] == lo["key"]).any() and (lo["goal"] != lo["key"]).any()
    assert sorted(np.unique(lo["rewards"][..., 1])) == [-2, 0, 2] and sorted(np.unique(lo["rewards"][..., 0])) == [-2, 0]
    assert lo["dones"][:, :-1].sum() == 0 and lo["dones"][:, -1].all()                   # dones on the last step only
    d = sh["dones"]
    assert d[:, [6, 13]].all() and d.sum() == 2 * 2 * 3 and sh["reset_goal"].shape == (2, 2) and sh["reset_key"].shape == (2, 2)
    path = os.path.join(OUT, "mpe_crypto.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        print(f"  {k:22s} {out[k].dtype} {out[k].shape}")


if __name__ == "__main__":
    main()
