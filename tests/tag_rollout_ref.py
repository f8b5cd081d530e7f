"""Reference side of the separated rollout on MPE simple_tag (tests/test_gpu_tag_episode.py, tests/test_mpe_tag.py): oracle networks in
float64 / float32, the host Philox and the tolerances of tests/rollout_ref.py, the NumPy mirror of the env.  No GPU, no kernels.  A
plain helper module: no fixtures, no pytest settings."""
import numpy as np
import torch

from conftest import golden
from oracle import mappo_oracle as O
import mpe_tag_np as MT
import rollout_ref as R

N, T, ENV_T = 12, 4, 25                   # environments (the fixture's long episodes), rollout steps, env episode length
SEED, PARAM_SEED = 1, 7                   # args.seed of the runner (sampling), torch seed of the twins' parameters
NEAR_CAP = 0.02                           # the project's cap: share of (row, agent) pairs allowed within the exclusion margin
AGENT_SEED_STEP = 0xD1B54A32D192ED03      # separated/base_runner.py: agent m samples with seed + m * this


def agent_seed(m, seed=SEED):
    from mappo_amd.distributed import sampling_seed
    return (sampling_seed(seed, 0) + m * AGENT_SEED_STEP) & 0xFFFFFFFFFFFFFFFF


def twins(centralized=True, **kw):
    """One oracle policy per agent (adversaries 16 -> 5, the good agent 14 -> 5), parameters from the CPU generator."""
    torch.manual_seed(PARAM_SEED)
    oa = O.default_args(episode_length=T, n_rollout_threads=N, use_centralized_V=centralized, **kw)
    return [O.PolicyRef(oa, d, 62 if centralized else d, a) for d, a in zip(MT.OBS_DIMS, MT.ACT_DIMS)]


def initial_state():
    """The fixture's long episodes' start (the scripted ones, with their contacts, included): pos, vel, landmarks."""
    g = golden("mpe_tag")
    return g["long/pos0"][:N].copy(), g["long/vel0"][:N].copy(), g["long/lpos"][:N].copy()


def expected_step(actor, obs_rows, m, step, deterministic=False, rollout=1):
    """(Expected, tol) of agent m's actor on `obs_rows` [N, D_m] at step `step` of the runner's `rollout`-th rollout (1-based): the
    runner advances every agent's counter word by T before each rollout, so the counter is rollout * T + step; Philox index = row."""
    z, _ = R.actor_eval(actor, obs_rows, None, dtype=torch.float64)
    z32, _ = R.actor_eval(actor, obs_rows, None, dtype=torch.float32)
    _, tol = R.err_and_tol(z, z32)
    if deterministic:
        return R.expected_argmax(z, None, tol), tol
    return R.expected_sample(z, None, R.uniform24(agent_seed(m), rollout * T + step, np.arange(obs_rows.shape[0])), tol), tol


def reference_rollout():
    """The runner's first rollout on the reference side alone: the mirror driven by the expected actions."""
    pol = twins()
    env = MT.SimpleTagNp(*initial_state(), episode_length=ENV_T)
    obs = env.obs()
    out = dict(expected=[[] for _ in range(4)], actions=[[] for _ in range(4)], tol=[[] for _ in range(4)])
    for t in range(T):
        acts = []
        for m in range(4):
            e, tol = expected_step(pol[m].actor, obs[m].astype(np.float32), m, t)
            out["expected"][m].append(e); out["actions"][m].append(e.action); out["tol"][m].append(tol)
            acts.append(e.action)
        obs, _, _ = env.step(np.stack(acts, axis=1))
    return out
