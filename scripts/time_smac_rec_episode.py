"""Time rollout() of a recurrent (rmappo) shared policy on the synthetic SMAC-shaped env, stepwise against the one-launch episode
(MAPPO_SMAC_REC_EPISODE=1): `python scripts/time_smac_rec_episode.py OUT.json [--n 256 512] [--T 25] [--runs 40]`.

    stepwise   pool launch, mappo_recurrent_step_dual, T - 1 x mappo_recurrent_rollout_step, mappo_insert_smac + compute(), in the
               runner's hipGraph
    episode    pool launch, mappo_rollout_episode_smac_recurrent (ONE launch for steps 0 .. T-1 and every insert) + compute(), in the
               runner's hipGraph

The 3m shape: M = 3 agents, obs 30, share 48, 9 actions, layer_N = 1, centralized critic, hipGraphs on.  Both variants run in one
process on runners built from the same seed, in both orders (stepwise first, then episode first), so that neither always benefits
from a warm device: three untimed rollouts (eager, capture, first replay), then RUNS single rollout() calls, each between device
synchronisations on the host clock.  Reported: microseconds per rollout(), median and [min, max], per order.  N = 256 is config 3 of
BASELINE.json; above 1024 rows (N = 512: 1536) the stepwise step is the two-launch form (features, then GRU step), whose arithmetic
differs from the fused step's, so there the episode's buffer is NOT bit-identical to the stepwise one — the comparison is of time
only.  Run it on the parent commit too (the flag is ignored there: both columns are the stepwise path, their difference is the
run-to-run spread)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLAG = "MAPPO_SMAC_REC_EPISODE"


def runner(N, T):
    from mappo_amd.config import get_config
    from mappo_amd.envs.synthetic import SyntheticSMACEnv
    from mappo_amd.runner.shared.smac_runner import SMACRunner
    dev = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy, a.use_naive_recurrent_policy, a.recurrent_N = True, False, 1
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "StarCraft2", 1
    a.use_centralized_V, a.layer_N, a.use_hip_graph, a.algorithm_name = True, 1, True, "rmappo"
    torch.manual_seed(1)
    env = SyntheticSMACEnv(N, 3, 30, 48, 9, seed=1, device=dev, pool_steps=T)
    r = SMACRunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=3, device=dev, run_dir=None))
    r.warmup()
    return r


def timed(r, runs):
    us = []
    for _ in range(runs):
        r.buffer.after_update()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.rollout()
        torch.cuda.synchronize()
        us.append(1e6 * (time.perf_counter() - t0))
    return dict(median=round(statistics.median(us), 1), min=round(min(us), 1), max=round(max(us), 1), runs=runs)


def main(out, ns, T, runs):
    res = []
    for N in ns:
        for order in (("stepwise", "episode"), ("episode", "stepwise")):
            row = dict(N=N, M=3, T=T, rows=3 * N, order=list(order))
            for name in order:
                os.environ[FLAG] = "1" if name == "episode" else "0"
                r = runner(N, T)
                for _ in range(3):
                    r.rollout()
                    r.buffer.after_update()
                assert isinstance(r._rollout_graph, torch.cuda.CUDAGraph)
                row[f"{name}_us"] = timed(r, runs)
                assert bool(torch.isfinite(r.buffer.returns).all())
                del r
            row["episode_over_stepwise"] = round(row["episode_us"]["median"] / row["stepwise_us"]["median"], 3)
            res.append(row)
            print(json.dumps(row), flush=True)
    os.environ.pop(FLAG, None)
    with open(out, "w") as f:
        json.dump(dict(runs=runs, results=res), f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--n", nargs="+", type=int, default=[256, 512])
    ap.add_argument("--T", type=int, default=25)
    ap.add_argument("--runs", type=int, default=40)
    args = ap.parse_args()
    main(args.out, args.n, args.T, args.runs)
