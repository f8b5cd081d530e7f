"""GPU-vectorised MPE `simple_adversary` ("physical deception") behind the reference's vec-env contract for agents of DIFFERENT
shapes and DIFFERENT rewards:

    reset() -> [obs_adversary [N, 8], obs_good1 [N, 10], obs_good2 [N, 10]]
    step(actions) -> ([obs_adversary, obs_good1, obs_good2], rewards [N, 3, 1], dones [N, 3] bool, infos)

(`onpolicy/envs/env_wrappers.py`, `onpolicy/envs/mpe/environment.py:117-148`, `scenarios/simple_adversary.py`).  The reference's
`train_mpe.py` starts it with `--scenario_name simple_adversary --num_agents 3`: agent 0, the adversary, sees the two landmarks and
the two others but not which landmark is the goal; agents 1 and 2, the good agents, also see the goal.  Every agent moves
(Discrete(5)).  The world is not collaborative, so `rewards[:, m]` is agent m's OWN reward: the adversary is paid for reaching the
goal, the good agents for one of them being near it while the adversary is far.  The two observation widths force
`share_policy = False`.  N environments are stepped by ONE kernel launch (csrc/mpe_ragged_env.hip on csrc/mpe_adv_core.h) and
everything stays in HBM, so the separated runner can run an episode as one launch (`episode_launch`,
mappo_rollout_episode_adversary).  What the six envs of this kind share — all but the description below — is in mpe_ragged.py.

`step` takes a list of per-agent tensors — each the reference's one-hot `[N, 5]` or indices `[N]` / `[N, 1]` — or one tensor: the
one-hots `[N, 3, 5]` or, with `accepts_index_actions`, indices `[N, 3]` / `[N, 3, 1]`.  Physics run in float64 as in the
reference's NumPy code, with outputs equal to the fp32 cast of the reference's (tests/golden/mpe_adversary.npz); initial states
come from a counter-based Philox stream (seed, episode, env), not from NumPy's global generator."""
import torch

from .mpe_ragged import F64, I32, I64, RaggedMPEVecEnv


class SimpleAdversaryVecEnv(RaggedMPEVecEnv):
    scenario, M, L = "simple_adversary", 3, 2
    obs_dims, act_dims = (8, 10, 10), (5, 5, 5)
    episode_flag = "MAPPO_ADV_EPISODE"
    state = (("agent_pos", F64, (M, 2), 0), ("agent_vel", F64, (M, 2), 0), ("landmark_pos", F64, (L, 2), 0),
             ("goal", I32, (), 0),                                 # landmark index of every agent's goal_a
             ("tstep", I32, (), 0), ("episode", I64, (), 0))
    env_ops = ("mpe_adversary_reset", "mpe_adversary_step", "rollout_episode_adversary")
    episode_state_adversary = RaggedMPEVecEnv.episode_state       # the name this scenario's tests call

    def __init__(self, n_rollout_threads, num_agents=3, episode_length=25, seed=1, device="cuda"):
        if int(num_agents) != 3:
            raise ValueError(f"simple_adversary is built for num_agents = 3: 1 adversary, 2 good agents, 2 landmarks (got {num_agents})")
        super().__init__(n_rollout_threads, episode_length, seed, device)

    def set_state(self, agent_pos, agent_vel, landmark_pos, goal, tstep=0):
        """Test hook: load explicit states (float64 arrays / tensors [N, 3, 2], [N, 3, 2], [N, 2, 2]; goal [N] landmark indices)."""
        self.agent_pos.copy_(torch.as_tensor(agent_pos, dtype=torch.float64))
        self.agent_vel.copy_(torch.as_tensor(agent_vel, dtype=torch.float64))
        self.landmark_pos.copy_(torch.as_tensor(landmark_pos, dtype=torch.float64))
        g = torch.as_tensor(goal).to(torch.int32)
        if int(g.min()) < 0 or int(g.max()) >= self.L:
            raise ValueError("goal must be landmark indices 0 .. 1")
        self.goal.copy_(g)
        self.tstep.fill_(int(tstep))
