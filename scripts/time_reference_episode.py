"""Time the rollout of one episode on SimpleReferenceVecEnv (MPE simple_reference, MultiDiscrete (5, 10) policy) at N = 1024,
T = 25, four ways: `python scripts/time_reference_episode.py OUT.json [ROLLOUTS]`.

    stepwise eager   T x (mappo_rollout_step_md + mappo_mpe_reference_step) + the bootstrap launch, launched from Python
    stepwise graph   the same launches replayed from the captured hipGraph
    episode eager    mappo_rollout_episode_reference, one launch from Python
    episode graph    the same launch replayed from the captured hipGraph

Each is MPERunner.rollout() as training calls it, so the GAE launch that follows the episode is inside every number.  Three
untimed rollouts first (eager pass, capture, first replay), then REPEATS repeats of ROLLOUTS back-to-back rollouts, each repeat
between two device synchronisations on the host clock (the eager stepwise path is bound by the host's launch rate, which device
events would not show).  Reported: microseconds per rollout, median and [min, max] over the repeats."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 7


def runner(episode, graph, N, T):
    from mappo_amd.config import get_config
    from mappo_amd.envs.mpe_reference import SimpleReferenceVecEnv
    from mappo_amd.runner.shared.mpe_runner import MPERunner
    dev = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.use_centralized_V, a.layer_N = True, 1
    a.use_hip_graph, a.fuse_rollout_episode = graph, episode
    torch.manual_seed(1)
    env = SimpleReferenceVecEnv(N, episode_length=T, seed=1, device=dev)
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=2, device=dev, run_dir=None))
    r.warmup()
    return r


def main(out, rollouts):
    N, T = 1024, 25
    res = []
    for name, episode, graph in (("stepwise eager", False, False), ("stepwise graph", False, True), ("episode eager", True, False),
                                 ("episode graph", True, True)):
        r = runner(episode, graph, N, T)
        for _ in range(3):
            r.rollout()
        torch.cuda.synchronize()
        us = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(rollouts):
                r.rollout()
            torch.cuda.synchronize()
            us.append(1e6 * (time.perf_counter() - t0) / rollouts)
        assert bool(torch.isfinite(r.buffer.rewards).all()) and float(r.buffer.rewards.max()) < 0
        res.append(dict(path=name, us_per_rollout=dict(median=round(statistics.median(us), 1), min=round(min(us), 1), max=round(max(us), 1)),
                        repeats=[round(u, 1) for u in us]))
        print(json.dumps(res[-1]), flush=True)
    with open(out, "w") as f:
        json.dump(dict(shape=dict(N=N, M=2, D=21, heads=[5, 10], T=T, layer_N=1), rollouts_per_repeat=rollouts, repeats=REPEATS, results=res), f,
                  indent=1)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 50)
