"""Reference side of the one-launch rollout episode on MPE simple_world_comm (tests/test_gpu_world_comm_episode.py,
tests/test_mpe_world_comm_episode.py).  The runner's stepwise path samples through collect_into (mlp_forward_kernel), which is not
the launch's tile16r_step to the bit, so the bit twin is built here from the C ABI: per step mappo_rollout_step_md for the leader and
mappo_rollout_step for agents 1 .. 5 on buffer slot t, mappo_mpe_world_comm_step in mode 1 on the [N, 7] indices, then the inserts.
Both step entry points want a narrow critic next to a narrow actor: a decentralized twin passes the agent's real critic and keeps its
values, a centralized one passes a throwaway narrow critic and discards them.  A plain helper module: no fixtures, no pytest
settings."""
import numpy as np
import torch

from conftest import golden
import mpe_world_comm_np as MW

M, HEADS = 6, (5, 4)
OBS_DIMS = (34, 34, 34, 34, 28, 28)
NAMES = ("obs", "share_obs", "actions", "action_log_probs", "rewards", "masks")
STATE = ("agent_pos", "agent_vel", "landmark_pos", "tstep", "episode")


def start_state(N):
    """Fixture start states tiled to N, then adjusted so that the first steps hold: a contact (the leader inside good agent 4's contact
    distance), a speed clamp (adversary 1 at speed 3: 0.75 x 3 - 0.9 > 1 whatever it does), two agents inside forest 0 (adversaries
    2 and 3) with a third outside it (adversary 1), and a good agent beyond 0.9 on one axis and beyond 1 on the other (both bound()
    branches)."""
    g = golden("mpe_world_comm")
    k = np.arange(N) % g["long/pos0"].shape[0]
    pos, vel, lpos = g["long/pos0"][k].copy(), g["long/vel0"][k].copy(), g["long/lpos"][k].copy()
    pos[:, 0] = pos[:, 4] + np.array([0.1, 0.0])
    vel[:, 1] = np.array([3.0, 0.0])
    pos[:, 2] = lpos[:, 3] + np.array([0.05, 0.0])
    pos[:, 3] = lpos[:, 3] - np.array([0.05, 0.05])
    pos[:, 1] = lpos[:, 3] + np.array([0.6, 0.0])
    pos[:, 5] = np.array([0.95, -1.2])
    return pos, vel, lpos


def slot0(state):
    """The six observations of `state` (nothing said yet) and the centralized share row, fp32."""
    o = [x.astype(np.float32) for x in MW.observation(state[0], state[1], state[2], np.zeros((state[0].shape[0], MW.C)))]
    return o, np.concatenate(o, axis=1)


class Twin:
    """The stepwise bit twin of one runner: its own copies of the six buffers' arrays and its own env state, the runner's networks,
    seeds and counter words."""

    def __init__(self, runner, env_state, narrow_critics):
        """env_state: the five state tensors to start from (cloned here); narrow_critics: per agent the (flat, desc) of a critic as
        wide as the agent's own observation — the real one when decentralized."""
        self.r, self.narrow = runner, narrow_critics
        self.buf = [{n: getattr(b, n).clone() for n in NAMES} for b in runner.buffer]
        self.values = [torch.zeros_like(b.value_preds) for b in runner.buffer]
        self.state = {k: env_state[k].clone() for k in STATE}

    def rollout(self, T, env_T, env_seed, centralized, deterministic=False):
        from mappo_amd import ops
        r = self.r
        N = r.n_rollout_threads
        dev = self.state["tstep"].device
        s = self.state
        for t in range(T):
            for m, p in enumerate(r.policy):
                b = self.buf[m]
                cf, cd = self.narrow[m]
                args = (p.actor.flat, p.actor.desc, cf, cd, (b["obs"][t], 0, 0), (b["obs"][t], 0, 0), 0, N)
                tail = (deterministic, p.actor._seed, t, p.actor._counter_dev, b["actions"][t], b["action_log_probs"][t], self.values[m][t])
                if m == 0:
                    ops.rollout_step_md(*args, HEADS, *tail)
                else:
                    ops.rollout_step(*args, None, *tail)
            acts = torch.cat([self.buf[m]["actions"][t].view(N, -1) for m in range(M)], dim=1).contiguous()
            obs = [torch.empty(N, d, device=dev) for d in OBS_DIMS]
            rew = torch.empty(N, M, device=dev)
            dones = torch.empty(N, M, dtype=torch.uint8, device=dev)
            ops.mpe_world_comm_step(s["agent_pos"], s["agent_vel"], s["landmark_pos"], s["tstep"], s["episode"], acts, 1, obs, rew, dones, N,
                                    env_T, env_seed)
            share = torch.cat(obs, dim=1)
            for m in range(M):
                b = self.buf[m]
                b["obs"][t + 1].copy_(obs[m])
                b["share_obs"][t + 1].copy_(share if centralized else obs[m])
                b["rewards"][t].copy_(rew[:, m:m + 1])
                b["masks"][t + 1].copy_(1.0 - dones[:, m:m + 1].float())

    def after_update(self):
        for b in self.buf:
            for n in ("obs", "share_obs", "masks"):
                b[n][0].copy_(b[n][-1])


# ---- the float64 side: oracle networks, the host Philox, the NumPy mirror (no GPU, no kernels) ------------------------------------
REF_N, REF_T, REF_ENV_T = 12, 4, 25       # environments, rollout steps, env episode length (no reset inside: the mirror has none)
SEED, PARAM_SEED = 1, 7                   # args.seed of the runner (sampling), torch seed of the twins' parameters
NEAR_CAP = 0.02                           # the project's cap: share of (row, agent) pairs allowed within the exclusion margin
AGENT_SEED_STEP = 0xD1B54A32D192ED03      # separated/base_runner.py: agent m samples with seed + m * this
ACT_DIMS = (9, 5, 5, 5, 5, 5)


def agent_seed(m, seed=SEED):
    from mappo_amd.distributed import sampling_seed
    return (sampling_seed(seed, 0) + m * AGENT_SEED_STEP) & 0xFFFFFFFFFFFFFFFF


def oracle_twins(centralized=True, **kw):
    """One oracle policy per agent (the leader 34 -> 9 logits = its two heads side by side, adversaries 34 -> 5, good agents
    28 -> 5), parameters from the CPU generator."""
    from oracle import mappo_oracle as O
    torch.manual_seed(PARAM_SEED)
    oa = O.default_args(episode_length=REF_T, n_rollout_threads=REF_N, use_centralized_V=centralized, **kw)
    return [O.PolicyRef(oa, d, 192 if centralized else d, a) for d, a in zip(OBS_DIMS, ACT_DIMS)]


def runner_actor_state(actor_ref, m):
    """An oracle actor's state dict as the runner's actor of agent m takes it: the leader's one head layer of 9 rows is the
    reference's two layers act.action_outs.{0, 1} of 5 and 4 rows."""
    sd = {k: v.detach().clone() for k, v in actor_ref.state_dict().items()}
    if m == 0:
        w, b = sd.pop("act.action_out.linear.weight"), sd.pop("act.action_out.linear.bias")
        lo = 0
        for j, d in enumerate(HEADS):
            sd[f"act.action_outs.{j}.linear.weight"], sd[f"act.action_outs.{j}.linear.bias"] = w[lo:lo + d].clone(), b[lo:lo + d].clone()
            lo += d
    return sd


def expected_step(actor, obs_rows, m, step, rollout=1):
    """([Expected per head], tol) of agent m's actor on `obs_rows` [N, D_m] at step `step` of the runner's `rollout`-th rollout
    (1-based): the runner advances every agent's counter word by T before each rollout, so the counter is rollout * T + step; head k
    of row n draws Philox index (k << 32) | n — the leader has two heads over logits [0, 5) and [5, 9), everybody else one."""
    import md_ref
    import rollout_ref as R
    z, _ = R.actor_eval(actor, obs_rows, None, dtype=torch.float64)
    z32, _ = R.actor_eval(actor, obs_rows, None, dtype=torch.float32)
    _, tol = R.err_and_tol(z, z32)
    rows = np.arange(obs_rows.shape[0], dtype=np.uint64)
    heads = HEADS if m == 0 else (ACT_DIMS[m],)
    out = []
    for k, (lo, hi) in enumerate(md_ref.head_slices(heads)):
        u = R.uniform24(agent_seed(m), rollout * REF_T + step, (np.uint64(k) << np.uint64(32)) | rows)
        out.append(R.expected_sample(z[:, lo:hi], None, u, tol))
    return out, tol


def reference_rollout():
    """The runner's first rollout on the reference side alone: the mirror driven by the expected actions.  near[m][t]: the rows of
    agent m that sit within the exclusion margin at step t (the leader: in either head)."""
    pol = oracle_twins()
    env = MW.SimpleWorldCommNp(*start_state(REF_N), episode_length=REF_ENV_T)
    obs = env.obs()
    out = dict(near=[[] for _ in range(M)], actions=[[] for _ in range(M)])
    for t in range(REF_T):
        cols = []
        for m in range(M):
            es, _ = expected_step(pol[m].actor, obs[m].astype(np.float32), m, t)
            out["near"][m].append(np.logical_or.reduce([e.near for e in es]))
            a = np.stack([e.action for e in es], axis=1)
            out["actions"][m].append(a)
            cols.append(a)
        obs, _, _ = env.step(np.concatenate(cols, axis=1).astype(np.int64))
    return out
