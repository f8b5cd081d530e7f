"""The cases of the one-launch SMAC-shaped recurrent episode's GPU tests (tests/test_gpu_episode_smac_recurrent.py) and, through the
host mirror of the synthetic env (tests/synth_ref.py), what each case's env output contains — so that the CPU suite
(tests/test_smac_rec_episode.py) can hold every seed to exercising every mask branch of the kernel.

A plain helper module: no fixtures, no pytest settings."""
import numpy as np

import synth_ref

P_DEATH, P_TERM = 0.2, 0.3

# (M, N, T, D, S, A, relu, layer_N, feature norm, centralized, naive, env seed); G M = 16 // M * M rows of a 16-row tile are used
CASES = [
    (3, 7, 6, 30, 48, 9, True, 1, True, True, False, 2),       # 15-row tiles: a lane idle in every tile; partial last tile
    (3, 7, 1, 4, 48, 2, False, 0, False, True, False, 1),      # T = 1
    (5, 4, 2, 64, 64, 17, True, 0, True, True, False, 1),      # G = 3, T = 2, a second head block
    (7, 3, 6, 30, 64, 32, False, 1, True, True, False, 1),     # G = 2: 14-row tiles; 32 actions
    (8, 2, 6, 4, 48, 9, True, 1, False, True, False, 1),       # one full tile
    (16, 3, 2, 30, 48, 17, False, 1, False, True, False, 1),   # one env per tile
    (16, 3, 6, 64, 64, 32, True, 0, True, True, False, 1),
    (1, 17, 6, 64, 48, 2, True, 0, True, True, False, 1),      # 16 envs per tile, the second tile holds one row
    (1, 17, 1, 30, 64, 32, False, 1, False, True, False, 1),
    (3, 7, 6, 30, 30, 9, False, 1, True, False, False, 1),     # use_centralized_V off: the critic reads obs
    (3, 7, 6, 30, 48, 9, True, 1, True, True, True, 2),        # use_naive_recurrent_policy
    (8, 2, 2, 64, 48, 9, False, 0, True, True, False, 2),
]
# the float64 case above 1024 rows (the stepwise path there is the two-launch step) and the small one: (M, N, T, D, S, A, relu, layer_N,
# feature norm, centralized, env seed, actor sampling seed = all_args.seed)
F64_CASES = [
    (3, 7, 6, 30, 48, 9, True, 1, True, True, 2, 1),
    (8, 130, 2, 30, 48, 9, False, 0, False, True, 1, 1),       # 1040 rows
]


def coverage(M, N, T, D, S, A, seed):
    """Counts over the T steps of the case's FIRST rollout: envs that end (all agents done) by termination, rows that are done in a live env
    (active_masks = 0), envs whose agents are all done WITHOUT a termination draw (every agent dead), unavailable actions on rows of a
    live env."""
    dead, c = np.zeros((N, M), dtype=bool), dict(terminated=0, dead_in_live_env=0, all_dead_no_termination=0, unavailable_in_live_env=0)
    for p in range(T):
        o = synth_ref.step(seed, 1 + p, N, M, D, S, A, P_DEATH, P_TERM, dead)
        env_done = o["dones"].all(axis=1)
        c["terminated"] += int(o["term"].sum())
        c["dead_in_live_env"] += int((o["dones"] & ~env_done[:, None]).sum())
        c["all_dead_no_termination"] += int((env_done & ~o["term"]).sum())
        c["unavailable_in_live_env"] += int(((o["avail"] == 0) & ~env_done[:, None, None]).sum())
        dead = o["dead_out"]
    return c


def required(M, T):
    """Which of coverage()'s counts a case must reach.  A dead row in a live env needs a second agent.  An env whose agents are all
    dead without a termination draw needs all M death draws (0.2 each) to fire before a termination (0.3 per step) resets them: one
    agent does that at once, three agents within six steps often enough to find a seed; five or more agents within at most six steps
    practically never (below 1e-3 per env), so those cases do not ask for it."""
    need = ["terminated", "unavailable_in_live_env"]
    if M >= 2:
        need.append("dead_in_live_env")
    if M == 1 or (M <= 3 and T >= 6):
        need.append("all_dead_no_termination")
    return need


# ---- host-reproducible weights and slot-0 rows of the float64 cases: the CPU suite runs the float64 reference ALONE on them ----
def make_args(M, N, T, relu=True, layer_N=1, fnorm=True, centralized=True, naive=False, recurrent=True, graph=False):
    from mappo_amd.config import get_config
    a = get_config().parse_known_args([])[0]
    a.algorithm_name = "rmappo" if recurrent else "mappo"
    a.use_recurrent_policy, a.use_naive_recurrent_policy = recurrent and not naive, recurrent and naive
    a.recurrent_N, a.data_chunk_length = 1, T
    a.episode_length, a.n_rollout_threads, a.env_name, a.seed = T, N, "StarCraft2", 1
    a.use_centralized_V, a.layer_N, a.use_ReLU, a.use_feature_normalization = centralized, layer_N, relu, fnorm
    a.use_hip_graph = graph
    return a


def perturbation(n, seed=7):
    """[n] float32 from a HOST generator: LayerNorm / feature-norm affines away from (1, 0), GRU biases away from 0, larger weights."""
    import torch
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.1


def host_networks(M, N, T, D, S, A, relu, layer_N, fnorm, centralized):
    """(actor, critic) on the CPU: the reference's seeded init plus perturbation() — the weights a float64 case runs on (the GPU test
    copies their flat vectors into its policy)."""
    import torch
    from mappo_amd.algorithms.r_mappo.algorithm.r_actor_critic import R_Actor, R_Critic
    from mappo_amd.utils.util import Discrete
    a = make_args(M, N, T, relu, layer_N, fnorm, centralized)
    torch.manual_seed(1)
    actor, critic = R_Actor(a, [D], Discrete(A), device="cpu"), R_Critic(a, [S if centralized else D], device="cpu")
    with torch.no_grad():
        actor.flat.add_(perturbation(actor.flat.numel(), 7))
        critic.flat.add_(perturbation(critic.flat.numel(), 8))
    return actor, critic


def host_slot0(N, M, D, S, A):
    """Slot 0 of obs / share_obs / available_actions (float32, action 0 always available), from a host generator."""
    import torch
    g = torch.Generator().manual_seed(11)
    obs, share = torch.randn(N, M, D, generator=g), torch.randn(N, M, S, generator=g)
    avail = (torch.rand(N, M, A, generator=g) < 0.7).float()
    avail[..., 0] = 1.0
    return obs, share, avail


def reference_skips(M, N, T, D, S, A, relu, layer_N, fnorm, centralized, seed, edge=1e-5):
    """The float64 reference ALONE over the case's episode (host weights, host slot 0, the env mirror's output, the host Philox draw
    keyed (sampling seed, k, buffer row), sampling counter word 0): the number of (step, row) pairs whose uniform lies within `edge`
    of an edge of the float64 CDF of the masked logits — the rows the GPU test may skip."""
    import torch
    import rec_ref
    from rollout_ref import philox_u32
    actor, _ = host_networks(M, N, T, D, S, A, relu, layer_N, fnorm, centralized)
    wa = rec_ref.weights64(actor, "act.action_out.linear")
    o = synth_ref.pool(seed, 1, N, M, D, S, A, P_DEATH, P_TERM, np.zeros((N, M), dtype=bool), T)
    obs0, _, avail0 = host_slot0(N, M, D, S, A)
    R = N * M
    h, mask, skipped = torch.zeros(R, 64, dtype=torch.float64), torch.ones(R, 1, dtype=torch.float64), 0
    for k in range(T):
        x = obs0.double().view(R, D) if k == 0 else torch.from_numpy(o["obs"][k - 1].astype(np.float32)).double().view(R, D)
        av = avail0.view(R, A) if k == 0 else torch.from_numpy(o["avail"][k - 1]).view(R, A)
        h_new, logits = rec_ref.step64(wa, actor.desc, "act.action_out.linear", x, h, mask)
        logits = torch.where(av == 0, torch.full_like(logits, -1e10), logits)
        cdf = torch.log_softmax(logits, dim=-1).exp().cumsum(dim=-1).numpy()
        u = (philox_u32(actor._seed, k, np.arange(R, dtype=np.int64)) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        skipped += int((np.abs(cdf - u[:, None]) <= edge).any(axis=1).sum())
        keep = torch.from_numpy(~o["dones"][k].all(axis=1)).double().view(N, 1).expand(N, M).reshape(R, 1)
        h, mask = h_new * keep, keep
    return skipped
