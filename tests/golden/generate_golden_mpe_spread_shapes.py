#!/usr/bin/env python3
"""Generate tests/golden/mpe_spread_shapes.npz by STEPPING the reference's own `simple_spread` at other shapes than the 3 x 3 of
mpe_envs.npz (build container only): the parity pin of everything in the spread kernels that depends on the number of agents M
and of landmarks L — the observation width and layout, the pair loops, the reward loops.

Run:  python tests/golden/generate_golden_mpe_spread_shapes.py       (needs the reference checkout; writes the .npz here)

The stand-ins for gym / seaborn, the env construction and the reproducible .npz writer are generate_golden_mpe.py's.  Only data is
written: the states each episode starts from, the actions fed, and what the reference returned.

SHAPES: every (M, L) below, chosen so that M = 1, L = 1, M < L, M > L, both maxima (8) and every tile size floor(16 / M) of the
one-launch episode in {16, 8, 4, 3, 2} occur.  Per shape, under `{M}x{L}/`, E episodes of 6 steps; kind [E] says what each is:
  0 plain     the reference's own reset (np.random.seed(SEED + 100 M + 10 L + e)), random index actions
  1 crowded   agents 1.. within 0.12 (per coordinate) of agent 0, as in generate_golden_mpe.py: the contact force acts
  2 scripted  (M >= 2) the agents form a chain whose consecutive distances cycle through DISTS: 0.3 -+ 1e-4 (both inside the
              softplus transition of the contact force), 1e-6 (deep overlap) and 50 (far field: the penetration underflows to 0);
              ceil(4 / (M - 1)) such episodes, so that every shape sees all four.  No two agents share a point.
  3 soft      fed PROBABILITY rows, not one-hots: rows of a seeded Dirichlet(1, 1, 1, 1, 1), rounded to float32 so that the
              reference (float64) and the kernel (fp32 action input) are fed the same numbers
Arrays, float64 unless said: pos0, vel0 [E, M, 2], lpos [E, L, 2], obs0 [E, M, D], actions_env [E, T, M, 5] (what was fed),
actions [E, T, M] int32 (the index fed as a one-hot; -1 in the soft episode), obs [E, T, M, D], rewards [E, T, M], dones [E, T, M]
bool, pos, vel [E, T, M, 2] (the state after every step), pos1, vel1 [E, M, 2] (after the last), kind [E] int8."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True                             # no __pycache__ next to the fixtures
import generate_golden_mpe as G  # noqa: E402

SHAPES = [(1, 1), (1, 3), (2, 5), (5, 2), (4, 3), (7, 1), (8, 8)]
DISTS = (0.3 - 1e-4, 0.3 + 1e-4, 1e-6, 50.0)
PLAIN, CROWDED, SCRIPTED, SOFT = 0, 1, 2, 3
T, SEED = G.T, 40


def kinds(M):
    if M == 1:
        return [PLAIN, PLAIN, SOFT]
    return [PLAIN, CROWDED] + [SCRIPTED] * -(-len(DISTS) // (M - 1)) + [SOFT]


def run(M, L):
    env = G.make_env("simple_spread", M, L)
    names = ("pos0", "vel0", "lpos", "obs0", "actions_env", "actions", "obs", "rewards", "dones", "pos", "vel", "pos1", "vel1", "kind")
    rec = {k: [] for k in names}
    chain = 0                                              # gaps scripted so far in this shape: the cycle through DISTS goes on
    for e, kind in enumerate(kinds(M)):
        np.random.seed(SEED + 100 * M + 10 * L + e)
        obs0 = env.reset()
        agents, landmarks = env.world.agents, env.world.landmarks
        rs = np.random.RandomState(500 + 100 * M + 10 * L + e)
        if kind == CROWDED:
            for a in agents[1:]:
                a.state.p_pos = agents[0].state.p_pos + rs.uniform(-0.12, 0.12, 2)
        elif kind == SCRIPTED:
            for i in range(1, M):
                th = rs.uniform(0, 2 * np.pi)
                agents[i].state.p_pos = agents[i - 1].state.p_pos + DISTS[chain % len(DISTS)] * np.array([np.cos(th), np.sin(th)])
                chain += 1
        if kind in (CROWDED, SCRIPTED):
            obs0 = [env._get_obs(a) for a in agents]
        rec["kind"].append(kind)
        rec["pos0"].append([a.state.p_pos.copy() for a in agents])
        rec["vel0"].append([a.state.p_vel.copy() for a in agents])
        rec["lpos"].append([l.state.p_pos.copy() for l in landmarks])
        rec["obs0"].append(obs0)
        rs = np.random.RandomState(1000 + 100 * M + 10 * L + e)
        ep = {k: [] for k in ("actions_env", "actions", "obs", "rewards", "dones", "pos", "vel")}
        for t in range(T):
            if kind == SOFT:
                idx = np.full(M, -1)
                fed = rs.dirichlet(np.ones(5), M).astype(np.float32).astype(np.float64)
            else:
                idx = rs.randint(0, 5, M)
                fed = np.eye(5)[idx]
            o, r, d, _ = env.step([fed[i].copy() for i in range(M)])
            ep["actions_env"].append(fed); ep["actions"].append(idx); ep["obs"].append(o)
            ep["rewards"].append(np.asarray(r, np.float64)[:, 0]); ep["dones"].append(d)
            ep["pos"].append([a.state.p_pos.copy() for a in agents])
            ep["vel"].append([a.state.p_vel.copy() for a in agents])
        for k, v in ep.items():
            rec[k].append(v)
        rec["pos1"].append(ep["pos"][-1])
        rec["vel1"].append(ep["vel"][-1])
    dtypes = dict(actions=np.int32, dones=np.bool_, kind=np.int8)
    out = {k: np.asarray(v, dtype=dtypes.get(k, np.float64)) for k, v in rec.items()}
    assert out["dones"][:, :-1].sum() == 0 and out["dones"][:, -1].all()
    assert out["obs"].shape[-1] == 4 + 2 * L + 4 * (M - 1) and np.isfinite(out["obs"]).all() and np.isfinite(out["rewards"]).all()
    return out


def main():
    G.install_stubs()
    out = {}
    for M, L in SHAPES:
        out.update({f"{M}x{L}/{k}": v for k, v in run(M, L).items()})
    path = os.path.join(G.OUT, "mpe_spread_shapes.npz")
    G.write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        print(f"  {k:18s} {out[k].dtype} {out[k].shape}")


if __name__ == "__main__":
    main()
