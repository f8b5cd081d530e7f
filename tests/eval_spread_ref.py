"""Float64 reference of one deterministic evaluation episode on simple_spread (mappo_eval_episode_spread, csrc/eval_spread.h),
independent of the kernels: the NumPy env of oracle/mpe_oracle.py with the host Philox reset draws of mpe_spread_np.py, stepped
under the oracle actor evaluated in float64 on the fp32 observation rows the kernel's actor reads.

An argmax is only comparable where the float64 top-two logit gap is clear of the fp32 kernels' logit error, so an env is marked
`near` — and left out of the comparison — when at any step any of its agents has a gap below MARGIN.  The rollout tests hold a
kernel's log-probs against float64 to tol = 4 err32 + 2e-6 (rollout_ref.err_and_tol; at most 6.5e-6 over every path recorded in
test_gpu_rollout_matrix.py) and treat an argmax within 2 tol as undecided; MARGIN = 2e-5 is that window at 1.5 x the largest
recorded tol.  The left-out share is capped at NEAR_CAP = 1 % of a case's envs; test_eval_episode_capi.py holds the committed
seeds to it on the CPU.

A plain helper module: no fixtures, no pytest settings."""
import functools

import numpy as np
import torch

import mpe_spread_np as MS
import rollout_ref as R
from oracle import mappo_oracle as O
from oracle import mpe_oracle as E

MARGIN = 2e-5
NEAR_CAP = 0.01
ENV_SEED = 11                      # the envs' Philox seed: start states (stream 1) and the reset draws inside the episode

# (N, M, L, T, env episode length, relu, layer_N, weight seed)
F64_CASES = [
    (100, 3, 3, 25, 7, True, 1, 31),          # 20 tiles in 5 workgroups; resets inside the episode (25 = 3 x 7 + 4)
    (40, 2, 2, 25, 25, False, 0, 32),         # 8 envs per tile, 5 tiles: a workgroup with one busy wave; the reset falls on the last step
]


def obs_dim(M, L):
    return 4 + 2 * L + 4 * (M - 1)


def make_actor(M, L, relu, layer_N, seed):
    """The oracle actor on the host (the weights every side of a comparison starts from)."""
    from test_gpu_kernels import _randomize
    torch.manual_seed(seed)
    net = O.ActorRef(O.default_args(use_ReLU=relu, layer_N=layer_N), obs_dim(M, L), 5)
    _randomize(net, seed + 1)
    return net


def start_state(N, M, L):
    """(pos [N, M, 2], lpos [N, L, 2]): what a reset to episode 1 draws; velocities 0, tstep 0 — and episode 0 in the tests, so the
    first reset inside the episode draws stream (ENV_SEED, 1) again, the next one stream 2."""
    return MS.reset_draws(ENV_SEED, 1, N, M, L)


@functools.lru_cache(maxsize=None)
def reference_episode(case):
    """dict(actions [T, N, M] int, returns [N, M] float64 (sum of the step rewards), near [N] bool, min_gap, pos / vel / lpos /
    tstep / episode: the final state) of F64_CASES entry `case`.  Computed once per process; callers must not modify it."""
    N, M, L, T, env_T, relu, layer_N, wseed = case
    actor = make_actor(M, L, relu, layer_N, wseed)
    pos, lpos = start_state(N, M, L)
    ref = E.SimpleSpreadRef(pos, np.zeros((N, M, 2)), lpos, env_T)
    episode = np.zeros(N, np.int64)

    def reset_states(n):
        episode[n] += 1
        p, l = MS.reset_draws(ENV_SEED, int(episode[n]), n + 1, M, L)
        return p[n], np.zeros((M, 2)), l[n]

    obs = ref.obs()
    actions, returns, near, min_gap = np.zeros((T, N, M), np.int64), np.zeros((N, M)), np.zeros(N, bool), np.inf
    for t in range(T):
        z, _ = R.actor_eval(actor, obs.astype(np.float32).reshape(N * M, -1))
        top2 = np.sort(z, axis=1)[:, -2:]
        gap = (top2[:, 1] - top2[:, 0]).reshape(N, M)
        near |= (gap < MARGIN).any(axis=1)
        min_gap = min(min_gap, float(gap.min()))
        actions[t] = np.argmax(z, axis=1).reshape(N, M)
        obs, rew, _ = ref.step(np.eye(5)[actions[t]], reset_states)
        returns += rew[:, :, 0]
    return dict(actions=actions, returns=returns, near=near, min_gap=min_gap, pos=ref.pos, vel=ref.vel, lpos=ref.lpos, tstep=ref.t,
                episode=episode)
