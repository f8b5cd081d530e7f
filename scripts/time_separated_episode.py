"""Time the rollout of one episode of the SEPARATED runner on a GPU-resident MPE env with agents of different shapes, T = 25, two ways:
`python scripts/time_separated_episode.py OUT.json --scenario {comm,adversary,tag,push,crypto,world_comm} [--n 128] [--rollouts 20]`.

    comm       SimpleSpeakerListenerVecEnv (speaker 3 -> 3, listener 11 -> 5)
    adversary  SimpleAdversaryVecEnv (adversary 8 -> 5, two good agents 10 -> 5, per-agent rewards)
    tag        SimpleTagVecEnv (three adversaries 16 -> 5, one good agent 14 -> 5, per-agent rewards)
    push       SimplePushVecEnv (adversary 8 -> 5, good agent 19 -> 5, the two collide, per-agent rewards)
    crypto     SimpleCryptoVecEnv (Eve 4 -> 4, Bob and Alice 8 -> 4, nobody moves, per-agent rewards)
    world_comm SimpleWorldCommVecEnv (leader 34 -> MultiDiscrete (5, 4), three adversaries 34 -> 5, two good agents 28 -> 5, 192-wide
               centralized critics, per-agent rewards): stepwise through collect_into (this env's path is opt-in, so its baseline runs with
               MAPPO_WORLD_COMM_EPISODE unset); episode = mappo_rollout_episode_world_comm + one critic forward per agent

    stepwise   T x (one mappo_rollout_step per agent + the env's step launch + the agents' inserts) + one bootstrap launch per agent,
               launched from Python (the env's episode_flag, e.g. MAPPO_TAG_EPISODE, = 0)
    episode    the env's episode_launch (mappo_rollout_episode_comm / _adversary / _tag / _push / _crypto), one launch from Python (the flag = 1)

Each is MPERunner.rollout() as training calls it, so the per-agent GAE launches that follow the episode are inside every number.
Three untimed rollouts first, then REPEATS repeats of ROLLOUTS back-to-back rollouts, each repeat between two device
synchronisations on the host clock (the stepwise path is bound by the host's launch rate, which device events would not show).
Reported: microseconds per rollout, median and [min, max] over the repeats."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 7
# env class, and the agents whose reward is always negative (a check that the episode ran the scenario's own rewards; none in
# simple_crypto, where Eve's reward is -2 or 0, and none in simple_world_comm, where a contact pays the adversaries 5)
SCENARIOS = dict(comm=("SimpleSpeakerListenerVecEnv", (0, 1)), adversary=("SimpleAdversaryVecEnv", (0,)), tag=("SimpleTagVecEnv", ()),
                 push=("SimplePushVecEnv", (1,)), crypto=("SimpleCryptoVecEnv", ()), world_comm=("SimpleWorldCommVecEnv", ()))


def runner(env_cls, N, T):
    from mappo_amd.config import get_config
    from mappo_amd.runner.separated.mpe_runner import MPERunner
    dev = torch.device("cuda:0")
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = a.use_naive_recurrent_policy = False
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "MPE", 1
    a.use_centralized_V, a.layer_N, a.share_policy, a.use_hip_graph = True, 1, False, False
    torch.manual_seed(1)
    env = env_cls(N, episode_length=T, seed=1, device=dev)
    r = MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=env.M, device=dev, run_dir=None))
    r.warmup()
    return r


def main(out, scenario, N, rollouts):
    from mappo_amd import envs
    T = 25
    env_cls, negative = getattr(envs, SCENARIOS[scenario][0]), SCENARIOS[scenario][1]
    res = []
    one_launch = hasattr(env_cls, "episode_launch")
    for name, flag in (("stepwise", "0"), ("episode", "1")) if one_launch else (("stepwise", "0"),):
        if one_launch and flag == getattr(env_cls, "episode_default", None):
            os.environ.pop(env_cls.episode_flag, None)              # an opt-in env's baseline is the flag UNSET: what a default run does
        elif one_launch:
            os.environ[env_cls.episode_flag] = flag
        r = runner(env_cls, N, T)
        assert r._episode_ready() == (flag == "1")
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
        assert all(bool(torch.isfinite(b.rewards).all()) for b in r.buffer) and all(float(r.buffer[m].rewards.max()) < 0 for m in negative)
        res.append(dict(path=name, us_per_rollout=dict(median=round(statistics.median(us), 1), min=round(min(us), 1), max=round(max(us), 1)),
                        repeats=[round(u, 1) for u in us]))
        print(json.dumps(res[-1]), flush=True)
    with open(out, "w") as f:
        json.dump(dict(shape=dict(N=N, agents=[dict(obs=d, actions=n) for d, n in zip(env_cls.obs_dims, env_cls.act_dims)],
                                  share=sum(env_cls.obs_dims), T=T, layer_N=1),
                       rollouts_per_repeat=rollouts, repeats=REPEATS, results=res), f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--scenario", required=True, choices=sorted(SCENARIOS))
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--rollouts", type=int, default=20)
    args = ap.parse_args()
    main(args.out, args.scenario, args.n, args.rollouts)
