"""Reference side of the separated rollout on MPE simple_crypto (tests/test_gpu_mpe_crypto.py, tests/test_mpe_crypto.py): oracle
networks in float64 / float32, the host Philox and the tolerances of tests/rollout_ref.py, the NumPy mirror of the env.  No GPU, no
kernels.  A plain helper module: no fixtures, no pytest settings."""
import numpy as np
import torch

from conftest import golden
from oracle import mappo_oracle as O
import mpe_crypto_np as MC
import rollout_ref as R

N, T, ENV_T, L = 12, 4, 25, 4             # environments (the fixture's long episodes with 4 landmarks), rollout steps, env episode length
SEED, PARAM_SEED = 1, 7                   # args.seed of the runner (sampling), torch seed of the twins' parameters
NEAR_CAP = 0.02                           # tests/test_gpu_multidiscrete.py: share of (row, agent) pairs allowed within the exclusion margin
AGENT_SEED_STEP = 0xD1B54A32D192ED03      # separated/base_runner.py: agent m samples with seed + m * this


def agent_seed(m, seed=SEED):
    from mappo_amd.distributed import sampling_seed
    return (sampling_seed(seed, 0) + m * AGENT_SEED_STEP) & 0xFFFFFFFFFFFFFFFF


def twins(centralized=True, **kw):
    """One oracle policy per agent (Eve 4 -> 4, Bob and Alice 8 -> 4), parameters from the CPU generator."""
    torch.manual_seed(PARAM_SEED)
    oa = O.default_args(episode_length=T, n_rollout_threads=N, use_centralized_V=centralized, **kw)
    return [O.PolicyRef(oa, d, MC.SHARE if centralized else d, a) for d, a in zip(MC.OBS_DIMS, MC.ACT_DIMS)]


def initial_state():
    """The start of the fixture's long episodes with 4 landmarks: goal, key (nothing said yet)."""
    g = golden("mpe_crypto")
    rows = g["long/num_landmarks"] == L
    assert int(rows.sum()) == N
    return g["long/goal"][rows].copy(), g["long/key"][rows].copy()


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
    env = MC.SimpleCryptoNp(*initial_state(), episode_length=ENV_T)
    obs = env.obs()
    out = dict(expected=[[], [], []], actions=[[], [], []], tol=[[], [], []])
    for t in range(T):
        acts = []
        for m in range(3):
            e, tol = expected_step(pol[m].actor, obs[m].astype(np.float32), m, t)
            out["expected"][m].append(e); out["actions"][m].append(e.action); out["tol"][m].append(tol)
            acts.append(e.action)
        obs, _, _ = env.step(np.stack(acts, axis=1))
    return out
