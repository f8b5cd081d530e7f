#!/usr/bin/env python3
"""Generate tests/golden/mpe_comm.npz by STEPPING the reference's own MPE `simple_speaker_listener` (build container only): the
parity pin of the GPU-vectorised scenario (csrc/mpe_comm_core.h) and of its NumPy restatement (tests/mpe_comm_np.py).

Run:  python tests/golden/generate_golden_mpe_comm.py       (needs the reference checkout; writes the .npz here)

The stub modules, the env construction and the reproducible .npz writer are those of generate_golden_mpe.py.  Only data is written.

E = 12 episodes of episode_length 6 from np.random.seed(20 + e), actions from RandomState(1000 + e), fed as one-hots: [3] for the
speaker (agent 0: the symbol it says), [5] for the listener (agent 1: its move).
  pos0, vel0 [E, 2, 2]    both agents at the start                 lpos [E, 3, 2]   landmark positions
  goal [E]                index k with `agents[0].goal_b is landmarks[k]`
  obs0_speaker [E, 3], obs0_listener [E, 11]                       what reset returned
  actions [E, T, 2]       the indices fed (symbol, move)
  obs_speaker [E, T, 3], obs_listener [E, T, 11], rewards [E, T, 2], dones [E, T, 2]     per step
  pos1, vel1 [E, 2, 2]    the state after the last step (the env itself does not reset on done)
float64, int32 (goal, actions) and bool (dones)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from generate_golden_mpe import E, OUT, SEED, T, install_stubs, make_env, write_npz  # noqa: E402

DIMS = (3, 5)                                        # speaker: Discrete(dim_c = 3); listener: Discrete(5)


def run():
    env = make_env("simple_speaker_listener", 2, 3)
    assert [s.n for s in env.action_space] == list(DIMS)
    keys = ("pos0", "vel0", "lpos", "goal", "obs0_speaker", "obs0_listener", "actions", "obs_speaker", "obs_listener", "rewards", "dones",
            "pos1", "vel1")
    rec = {k: [] for k in keys}
    for e in range(E):
        np.random.seed(SEED + e)
        obs0 = env.reset()
        agents, landmarks = env.world.agents, env.world.landmarks
        rec["pos0"].append([a.state.p_pos.copy() for a in agents])
        rec["vel0"].append([a.state.p_vel.copy() for a in agents])
        rec["lpos"].append([l.state.p_pos.copy() for l in landmarks])
        rec["goal"].append([k for k, l in enumerate(landmarks) if agents[0].goal_b is l][0])
        rec["obs0_speaker"].append(np.array(obs0[0], np.float64))
        rec["obs0_listener"].append(np.array(obs0[1], np.float64))
        rs = np.random.RandomState(1000 + e)
        acts, osp, oli, rew, dones = [], [], [], [], []
        for t in range(T):
            idx = np.array([rs.randint(0, d) for d in DIMS])
            o, r, d, _ = env.step([np.eye(n)[i] for n, i in zip(DIMS, idx)])
            acts.append(idx)
            osp.append(np.array(o[0], np.float64)); oli.append(np.array(o[1], np.float64))
            rew.append(np.asarray(r, np.float64)[:, 0])
            dones.append(d)
        rec["actions"].append(acts); rec["obs_speaker"].append(osp); rec["obs_listener"].append(oli)
        rec["rewards"].append(rew); rec["dones"].append(dones)
        rec["pos1"].append([a.state.p_pos.copy() for a in agents])
        rec["vel1"].append([a.state.p_vel.copy() for a in agents])
    out = {k: np.asarray(v, dtype=np.int32 if k in ("actions", "goal") else (np.bool_ if k == "dones" else np.float64))
           for k, v in rec.items()}
    assert sorted(np.unique(out["goal"])) == [0, 1, 2]                                   # all three goal indices occur
    assert out["dones"][:, :-1].sum() == 0 and out["dones"][:, -1].all()                 # dones on the last step only
    assert sorted(np.unique(out["actions"][..., 0])) == [0, 1, 2]                        # every symbol
    assert sorted(np.unique(out["actions"][..., 1])) == [0, 1, 2, 3, 4]                  # every move
    return out


def main():
    install_stubs()
    out = run()
    path = os.path.join(OUT, "mpe_comm.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        print(f"  {k:14s} {out[k].dtype} {out[k].shape}")


if __name__ == "__main__":
    main()
