"""Time train() alone of the SEPARATED runner, sequential against grouped (MAPPO_SEPARATED_GROUP_TRAIN=1), with the rollout beside it:
`python scripts/time_separated_train.py OUT.json [--scenarios tag adversary] [--n 128 1024] [--trains 10]`.

    sequential  Runner.train as it is without the flag: per agent R_MAPPO.train (its own hipGraph: prologue 2 launches, ppo_epoch x
                (dual update + 2 optimiser launches), statistics) + the agent's after_update launch + the statistics' host read
    grouped     per-agent prologues, ppo_epoch x (ONE update launch + ONE optimiser call for all agents), per-agent epilogues with
                after_update inside, one hipGraph for everything; the agents' statistics read at the end

T = 25, ppo_epoch = 10, layer_N = 1, centralized critics, hipGraphs on (the training default).  Both variants run in one session on
runners built from the same seed: one rollout fills the buffers, three untimed train() calls (eager, capture, first replay), then
REPEATS repeats of TRAINS back-to-back train() calls between device synchronisations on the host clock (train() ends with a host
read per agent, so the host clock is what a training loop sees).  The rollout (one-launch episode + bootstrap + GAE per agent) is
timed the same way.  Reported: microseconds per call, median and [min, max] over the repeats."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 7
FLAG = "MAPPO_SEPARATED_GROUP_TRAIN"
SCENARIOS = dict(adversary="SimpleAdversaryVecEnv", tag="SimpleTagVecEnv", push="SimplePushVecEnv", crypto="SimpleCryptoVecEnv")


def runner(env_cls, N, T, ppo_epoch):
    from mappo_amd.config import get_config
    from mappo_amd.runner.separated.mpe_runner import MPERunner
    dev = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.use_centralized_V, a.layer_N, a.share_policy, a.use_hip_graph = True, 1, False, True
    a.ppo_epoch, a.num_mini_batch, a.algorithm_name = ppo_epoch, 1, "mappo"
    torch.manual_seed(1)
    env = env_cls(N, episode_length=T, seed=1, device=dev)
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=env.M, device=dev, run_dir=None))
    r.warmup()
    return r


def timed(fn, calls):
    us = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        us.append(1e6 * (time.perf_counter() - t0) / calls)
    return dict(median=round(statistics.median(us), 1), min=round(min(us), 1), max=round(max(us), 1), repeats=[round(u, 1) for u in us])


def main(out, scenarios, ns, trains):
    from mappo_amd import envs
    T, E = 25, 10
    res = []
    for sc in scenarios:
        env_cls = getattr(envs, SCENARIOS[sc])
        for N in ns:
            row = dict(scenario=sc, N=N, T=T, ppo_epoch=E, agents=env_cls.M, rows_per_agent=N * T)
            for name, flag in (("sequential", None), ("grouped", "1")):
                os.environ.pop(FLAG, None)
                if flag:
                    os.environ[FLAG] = flag
                r = runner(env_cls, N, T, E)
                assert r._group_train_ready() == bool(flag)
                r.rollout()
                for _ in range(3):
                    infos = r.train()
                row[f"train_{name}_us"] = timed(r.train, trains)
                assert all(bool(torch.isfinite(p.flat_params).all()) for p in r.policy), "training diverged on the repeated buffer"
                if not flag:
                    for _ in range(3):
                        r.rollout()
                    row["rollout_us"] = timed(r.rollout, trains)
                del r
            row["grouped_over_sequential"] = round(row["train_grouped_us"]["median"] / row["train_sequential_us"]["median"], 3)
            res.append(row)
            print(json.dumps(row), flush=True)
    os.environ.pop(FLAG, None)
    with open(out, "w") as f:
        json.dump(dict(trains_per_repeat=trains, repeats=REPEATS, results=res), f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--scenarios", nargs="+", default=["tag", "adversary"], choices=sorted(SCENARIOS))
    ap.add_argument("--n", nargs="+", type=int, default=[128, 1024])
    ap.add_argument("--trains", type=int, default=10)
    args = ap.parse_args()
    main(args.out, args.scenarios, args.n, args.trains)
