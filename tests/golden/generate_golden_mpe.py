#!/usr/bin/env python3
"""Generate tests/golden/mpe_envs.npz by STEPPING the reference's own MPE environments (build container only): the parity pin of
the GPU-vectorised `simple_reference` and `simple_spread`.

Run:  python tests/golden/generate_golden_mpe.py            (needs the reference checkout; writes the .npz here)

The reference's env package does not import as it stands where this project is built: `core.py` imports seaborn (for a colour
palette it no longer uses), `environment.py` / `multi_discrete.py` import gym (for base classes and the space types), and the
package `__init__`s pull in every other environment.  So, before anything of the reference is imported:
  * `gym`, `gym.spaces`, `gym.envs.registration`, `seaborn` (and `imp`, where the interpreter no longer has it) are registered as
    stub modules of a few lines: empty base classes and the three space types with the attributes the env reads;
  * `onpolicy`, `onpolicy.envs`, `onpolicy.envs.mpe` and `onpolicy.envs.mpe.scenarios` are registered as bare packages (a module
    with a __path__), so their `__init__`s never run and the scenario modules are imported by name.
Only data is written: the states each episode starts from, the actions fed, and what the reference returned.

Per scenario, E = 12 episodes of episode_length 6 from np.random.seed(SEED + e), actions from RandomState(1000 + e):
  ref/*     simple_reference, M = 2, L = 3, dim_c = 10, MultiDiscrete([[0, 4], [0, 9]]) — actions [E, T, 2, 2] head indices, fed as the
            heads' one-hots side by side ([15] per agent: mpe_runner.py:111-117); goals [E, 2]: the landmark index k with
            `agent.goal_b is world.landmarks[k]`
  spread/*  simple_spread, M = 3, L = 3, Discrete(5) — actions [E, T, 3] indices, fed as one-hots [5]; the odd episodes start with
            the agents within 0.3 of each other (placed by hand after the reset), so the contact force acts
  both:     pos0, vel0 [E, M, 2], lpos [E, L, 2], obs0 [E, M, D] (what reset returned), obs [E, T, M, D], rewards [E, T, M],
            dones [E, T, M], pos1, vel1 [E, M, 2] (the state after the last step; the env itself does not reset on done) — float64"""
import io
import os
import sys
import types
import zipfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
# the reference checkout: $MAPPO_REFERENCE, or a `reference` directory next to this repository
REF = os.environ.get("MAPPO_REFERENCE") or os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(OUT))), "reference")
E, T, SEED = 12, 6, 20


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _package(name, path):
    return _module(name, __path__=[path])


def install_stubs():
    class Env:
        pass

    class Space:
        pass

    class Discrete(Space):
        def __init__(self, n):
            self.n = n

    class Box(Space):
        def __init__(self, low=None, high=None, shape=None, dtype=None):
            self.low, self.high, self.shape, self.dtype = low, high, shape, dtype

    class Tuple(Space):
        def __init__(self, spaces):
            self.spaces = spaces

    spaces = _module("gym.spaces", Space=Space, Discrete=Discrete, Box=Box, Tuple=Tuple)
    registration = _module("gym.envs.registration", EnvSpec=type("EnvSpec", (), {}))
    envs = _module("gym.envs", registration=registration)
    _module("gym", Env=Env, Space=Space, spaces=spaces, envs=envs)
    _module("seaborn")
    try:
        import imp  # noqa: F401
    except ImportError:
        _module("imp")
    sys.dont_write_bytecode = True
    root = os.path.join(REF, "onpolicy")
    _package("onpolicy", root)
    _package("onpolicy.envs", os.path.join(root, "envs"))
    _package("onpolicy.envs.mpe", os.path.join(root, "envs", "mpe"))
    _package("onpolicy.envs.mpe.scenarios", os.path.join(root, "envs", "mpe", "scenarios"))


def make_env(scenario_name, num_agents, num_landmarks):
    """What MPE_env.MPEEnv does, with the scenario module imported by name."""
    import importlib
    from onpolicy.envs.mpe.environment import MultiAgentEnv
    scenario = importlib.import_module("onpolicy.envs.mpe.scenarios." + scenario_name).Scenario()
    args = types.SimpleNamespace(episode_length=T, num_agents=num_agents, num_landmarks=num_landmarks, scenario_name=scenario_name)
    world = scenario.make_world(args)
    return MultiAgentEnv(world, scenario.reset_world, scenario.reward, scenario.observation, scenario.info)


def run(scenario_name, M, L, head_dims, crowd):
    env = make_env(scenario_name, M, L)
    K = len(head_dims)
    rec = {k: [] for k in ("pos0", "vel0", "lpos", "obs0", "actions", "obs", "rewards", "dones", "pos1", "vel1", "goals")}
    for e in range(E):
        np.random.seed(SEED + e)
        obs0 = env.reset()
        agents, landmarks = env.world.agents, env.world.landmarks
        if crowd and e % 2 == 1:                      # agents 1.. within 0.3 of agent 0: the contact force is exercised
            rs = np.random.RandomState(500 + e)
            for a in agents[1:]:
                a.state.p_pos = agents[0].state.p_pos + rs.uniform(-0.12, 0.12, 2)
            obs0 = [env._get_obs(a) for a in agents]
        rec["pos0"].append([a.state.p_pos.copy() for a in agents])
        rec["vel0"].append([a.state.p_vel.copy() for a in agents])
        rec["lpos"].append([l.state.p_pos.copy() for l in landmarks])
        rec["obs0"].append(obs0)
        if hasattr(agents[0], "goal_b"):
            rec["goals"].append([[k for k, l in enumerate(landmarks) if a.goal_b is l][0] for a in agents])
        rs = np.random.RandomState(1000 + e)
        acts, obs, rew, dones = [], [], [], []
        for t in range(T):
            idx = np.stack([rs.randint(0, d, M) for d in head_dims], axis=1)                  # [M, K]
            onehot = [np.concatenate([np.eye(d)[idx[i, j]] for j, d in enumerate(head_dims)]) for i in range(M)]
            o, r, d, _ = env.step(onehot)
            acts.append(idx if K > 1 else idx[:, 0])
            obs.append(o)
            rew.append(np.asarray(r, np.float64)[:, 0])
            dones.append(d)
        rec["actions"].append(acts); rec["obs"].append(obs); rec["rewards"].append(rew); rec["dones"].append(dones)
        rec["pos1"].append([a.state.p_pos.copy() for a in agents])
        rec["vel1"].append([a.state.p_vel.copy() for a in agents])
    out = {}
    for k, v in rec.items():
        if not v:
            continue
        out[k] = np.asarray(v, dtype=np.int32 if k in ("actions", "goals") else (np.bool_ if k == "dones" else np.float64))
    assert out["dones"][:, :-1].sum() == 0 and out["dones"][:, -1].all()
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that the file regenerates bit-identically."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    install_stubs()
    out = {}
    for tag, res in (("ref", run("simple_reference", 2, 3, (5, 10), False)), ("spread", run("simple_spread", 3, 3, (5,), True))):
        out.update({f"{tag}/{k}": v for k, v in res.items()})
    d = np.linalg.norm(out["spread/pos0"][:, 0] - out["spread/pos0"][:, 1], axis=-1)
    assert (d[1::2] < 0.3).all() and (d[0::2] > 0.3).all(), d
    assert len(np.unique(out["ref/goals"])) == 3
    path = os.path.join(OUT, "mpe_envs.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        print(f"  {k:18s} {out[k].dtype} {out[k].shape}")


if __name__ == "__main__":
    main()
