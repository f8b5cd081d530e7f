"""Time the one-launch rollout episode (mappo_rollout_episode) alone at the bench shape under a list of geometry overrides:
`python scripts/time_episode.py OUT.json [CALLS]`.  The overrides are read at every launch, so one process sweeps them all; each
setting is timed as CALLS back-to-back launches between two events (three repeats, microseconds per launch)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARS = ("MAPPO_EPISODE_LDS", "MAPPO_EPISODE_LDS_WAVES", "MAPPO_EPISODE_LDS_ACTOR_WGS", "MAPPO_EPISODE_WAVES", "MAPPO_EPISODE_NET_WAVES",
        "MAPPO_EPISODE_INS_WAVES", "MAPPO_EPISODE_COST_A")
SWEEP = [{"MAPPO_EPISODE_LDS": 0}, {}] + [{"MAPPO_EPISODE_LDS_WAVES": w} for w in (4, 8, 12, 16)] + \
        [{"MAPPO_EPISODE_LDS_ACTOR_WGS": g} for g in (116, 120, 124, 126, 128, 130, 132, 134, 136, 140)] + \
        [{"MAPPO_EPISODE_LDS_WAVES": 12, "MAPPO_EPISODE_LDS_ACTOR_WGS": g} for g in (124, 128, 132)]


def main(out, calls):
    from mappo_amd.config import get_config
    from mappo_amd.envs.synthetic import SyntheticMPEEnv
    from mappo_amd.runner.shared.mpe_runner import MPERunner
    dev = torch.device("cuda:0")
    N, M, D, A, T = 1024, 3, 18, 5, 25
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.use_centralized_V, a.layer_N, a.use_hip_graph = True, 1, False
    env = SyntheticMPEEnv(N, M, D, A, T, seed=1, device=dev)
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=M, device=dev, run_dir=None))
    r.warmup()
    pol, b = r.trainer.policy, r.buffer
    block = env.episode_block()
    nv = torch.empty(N * M, device=dev)
    res = []
    for s in SWEEP:
        for k in VARS:
            os.environ.pop(k, None)
        for k, v in s.items():
            os.environ[k] = str(v)
        us = []
        for _ in range(4):                                   # the first repeat warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                pol.collect_episode_fused(b, block, nv, True)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / calls)
        res.append(dict(setting=s, us_per_launch=[round(u, 2) for u in us[1:]]))
        print(json.dumps(res[-1]), flush=True)
    with open(out, "w") as f:
        json.dump(dict(shape=dict(N=N, M=M, D=D, A=A, T=T, layer_N=1), calls=calls, results=res), f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 200)
