"""Time MPERunner.eval() on the GPU-resident simple_spread env, the stepwise loop against the one-launch evaluation episode
(MAPPO_SPREAD_EVAL_EPISODE=1): `python scripts/time_spread_eval_episode.py OUT.json [--n 128 1024] [--runs 40]`.

    stepwise   env reset, T x (policy.act, one-hot, env step, mask update), a stack of T reward tensors, rew.sum(0).mean() read back
    episode    env reset, mappo_eval_episode_spread (ONE launch for steps 0 .. T-1), returns.mean() read back

M = 3 agents, 3 landmarks, T = 25, layer_N = 1, feed-forward policy; eval() is eager in both variants.  Every (N, variant) pair runs
in a process of its own (this script starts them one after the other and does not touch the GPU itself): three untimed eval()
calls, then RUNS single calls, each between device synchronisations on the host clock — eval() ends in a host read, so the clock
covers the launches and that read.  Reported: microseconds per eval(), median and [min, max], and the value each variant logged."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLAG = "MAPPO_SPREAD_EVAL_EPISODE"
T = 25


def runner(N):
    import torch
    from mappo_amd.config import get_config
    from mappo_amd.envs.mpe_spread import SimpleSpreadVecEnv
    from mappo_amd.runner.shared.mpe_runner import MPERunner
    dev = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.use_centralized_V, a.layer_N = True, 1
    torch.manual_seed(1)
    env, eval_env = (SimpleSpreadVecEnv(N, 3, 3, T, seed=s, device=dev) for s in (1, 2))
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=eval_env, num_agents=3, device=dev, run_dir=None))
    r.warmup()
    return r


def child(N, runs):
    """One variant (the flag is in the environment) at one N: prints a JSON line."""
    import contextlib
    import io
    import torch
    r = runner(N)
    values = []
    r.log_env = lambda info, steps: values.append(info["eval_average_episode_rewards"][0])
    us = []
    with contextlib.redirect_stdout(io.StringIO()):          # eval() prints the value it logs
        for k in range(3 + runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.eval(0)
            torch.cuda.synchronize()
            if k >= 3:
                us.append(1e6 * (time.perf_counter() - t0))
    print(json.dumps(dict(median=round(statistics.median(us), 1), min=round(min(us), 1), max=round(max(us), 1), runs=runs, value=values[-1])))


def main(out, ns, runs):
    res = []
    for N in ns:
        row = dict(N=N, M=3, T=T, rows=3 * N)
        for name, flag in (("stepwise", "0"), ("episode", "1")):
            env = dict(os.environ, **{FLAG: flag})
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(N), "--runs", str(runs)], env=env,
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"{name} at N = {N} ended with status {p.returncode}:\n{p.stdout}\n{p.stderr}")
            row[f"{name}_us"] = json.loads(p.stdout.strip().splitlines()[-1])
        row["episode_over_stepwise"] = round(row["episode_us"]["median"] / row["stepwise_us"]["median"], 3)
        res.append(row)
        print(json.dumps(row), flush=True)
    with open(out, "w") as f:
        json.dump(dict(runs=runs, results=res), f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--n", nargs="+", type=int, default=[128, 1024])
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--child", type=int, default=None, help="internal: time one variant at this N in this process")
    args = ap.parse_args()
    if args.child is not None:
        child(args.child, args.runs)
    else:
        if not args.out:
            ap.error("OUT.json is required")
        main(args.out, args.n, args.runs)
