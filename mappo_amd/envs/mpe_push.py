"""GPU-vectorised MPE `simple_push` ("keep-away") behind the reference's vec-env contract for agents of DIFFERENT shapes and
DIFFERENT rewards:

    reset() -> [obs_adversary [N, 8], obs_good [N, 19]]
    step(actions) -> ([obs_adversary, obs_good], rewards [N, 2, 1], dones [N, 2] bool, infos)

(`onpolicy/envs/env_wrappers.py`, `onpolicy/envs/mpe/environment.py:117-148`, `scenarios/simple_push.py`).  The reference's
`train_mpe.py` starts it with `--scenario_name simple_push --num_agents 2 --num_landmarks 2`: agent 0, the adversary, sees its own
velocity, the two landmarks and the other agent but not which landmark is the goal, and is paid for being nearer to the goal than
the good agent is; agent 1, the good agent, also sees the goal, its own colour (which names the goal) and the landmarks' colours,
and is paid for being near the goal.  The two agents collide with each other — the adversary pushes the good agent away — and with
nothing else.  Both move (Discrete(5)).  The world is not collaborative, so `rewards[:, m]` is agent m's OWN reward.  The two
observation widths force `share_policy = False`.  N environments are stepped by ONE kernel launch (csrc/mpe_ragged_env.hip on
csrc/mpe_push_core.h) and everything stays in HBM, so the separated runner can run an episode as one launch (`episode_launch`,
mappo_rollout_episode_push).  What the six envs of this kind share — all but the description below — is in mpe_ragged.py.

`step` takes a list of per-agent tensors — each the reference's one-hot `[N, 5]` or indices `[N]` / `[N, 1]` — or one tensor: the
one-hots `[N, 2, 5]` or, with `accepts_index_actions`, indices `[N, 2]` / `[N, 2, 1]`.  Physics run in float64 as in the
reference's NumPy code, with outputs within 1e-6 of the fp32 cast of the reference's (tests/golden/mpe_push.npz; the contact force
goes through exp and log, which are not NumPy's to the bit); initial states come from a counter-based Philox stream (seed, episode,
env), not from NumPy's global generator."""
import torch

from .mpe_ragged import F64, I32, I64, RaggedMPEVecEnv


class SimplePushVecEnv(RaggedMPEVecEnv):
    scenario, M, L = "simple_push", 2, 2
    obs_dims, act_dims = (8, 19), (5, 5)
    episode_flag = "MAPPO_PUSH_EPISODE"
    state = (("agent_pos", F64, (M, 2), 0), ("agent_vel", F64, (M, 2), 0), ("landmark_pos", F64, (L, 2), 0),
             ("goal", I32, (), 0),                                 # landmark index of both agents' goal_a
             ("tstep", I32, (), 0), ("episode", I64, (), 0))
    env_ops = ("mpe_push_reset", "mpe_push_step", "rollout_episode_push")

    def __init__(self, n_rollout_threads, num_agents=2, episode_length=25, seed=1, device="cuda", num_landmarks=2):
        if (int(num_agents), int(num_landmarks)) != (2, 2):
            raise ValueError(f"simple_push is built for num_agents = 2: 1 adversary, 1 good agent, 2 landmarks (got num_agents {num_agents}, "
                             f"num_landmarks {num_landmarks})")
        super().__init__(n_rollout_threads, episode_length, seed, device)

    def set_state(self, agent_pos, agent_vel, landmark_pos, goal, tstep=0):
        """Test hook: load explicit states (float64 arrays / tensors [N, 2, 2], [N, 2, 2], [N, 2, 2]; goal [N] landmark indices).
        `episode`, the reset counter that keys the Philox stream, is left as it is."""
        self.agent_pos.copy_(torch.as_tensor(agent_pos, dtype=torch.float64))
        self.agent_vel.copy_(torch.as_tensor(agent_vel, dtype=torch.float64))
        self.landmark_pos.copy_(torch.as_tensor(landmark_pos, dtype=torch.float64))
        g = torch.as_tensor(goal).to(torch.int32)
        if int(g.min()) < 0 or int(g.max()) >= self.L:
            raise ValueError("goal must be landmark indices 0 .. 1")
        self.goal.copy_(g)
        self.tstep.fill_(int(tstep))
