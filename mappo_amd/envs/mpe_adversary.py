"""GPU-vectorised MPE `simple_adversary` ("physical deception") behind the reference's vec-env contract for agents of DIFFERENT
shapes and DIFFERENT rewards:

    reset() -> [obs_adversary [N, 8], obs_good1 [N, 10], obs_good2 [N, 10]]
    step(actions) -> ([obs_adversary, obs_good1, obs_good2], rewards [N, 3, 1], dones [N, 3] bool, infos)

(`onpolicy/envs/env_wrappers.py`, `onpolicy/envs/mpe/environment.py:117-148`, `scenarios/simple_adversary.py`).  The reference's
`train_mpe.py` starts it with `--scenario_name simple_adversary --num_agents 3`: agent 0, the adversary, sees the two landmarks and
the two others but not which landmark is the goal; agents 1 and 2, the good agents, also see the goal.  Every agent moves
(Discrete(5)).  The world is not collaborative, so `rewards[:, m]` is agent m's OWN reward: the adversary is paid for reaching the
goal, the good agents for one of them being near it while the adversary is far.  The two observation widths force
`share_policy = False`.  N environments are stepped by ONE kernel launch (csrc/mpe_adv_env.hip) and everything stays in HBM, so the
separated runner can run an episode as one launch (`episode_launch`, mappo_rollout_episode_adversary).  What the three envs of this kind share is in mpe_ragged.py.

`step` takes a list of per-agent tensors — each the reference's one-hot `[N, 5]` or indices `[N]` / `[N, 1]` — or one tensor: the
one-hots `[N, 3, 5]` or, with `accepts_index_actions`, indices `[N, 3]` / `[N, 3, 1]`.  Physics run in float64 as in the
reference's NumPy code, with outputs equal to the fp32 cast of the reference's (tests/golden/mpe_adversary.npz); initial states
come from a counter-based Philox stream (seed, episode, env), not from NumPy's global generator."""
import torch

from .. import ops
from .mpe_ragged import RaggedMPEVecEnv


class SimpleAdversaryVecEnv(RaggedMPEVecEnv):
    M, L = 3, 2
    obs_dims, act_dims = (8, 10, 10), (5, 5, 5)
    episode_flag = "MAPPO_ADV_EPISODE"

    def __init__(self, n_rollout_threads, num_agents=3, episode_length=25, seed=1, device="cuda"):
        if int(num_agents) != 3:
            raise ValueError(f"simple_adversary is built for num_agents = 3: 1 adversary, 2 good agents, 2 landmarks (got {num_agents})")
        super().__init__(n_rollout_threads, episode_length, seed, device)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.agent_pos = torch.zeros(self.N, self.M, 2, **f64)
        self.agent_vel = torch.zeros(self.N, self.M, 2, **f64)
        self.landmark_pos = torch.zeros(self.N, self.L, 2, **f64)
        self.goal = torch.zeros(self.N, **i32)                     # landmark index of every agent's goal_a
        self.tstep = torch.zeros(self.N, **i32)
        self.episode = torch.zeros(self.N, dtype=torch.int64, device=self.device)

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

    def state_tensors(self):
        return dict(agent_pos=self.agent_pos, agent_vel=self.agent_vel, landmark_pos=self.landmark_pos, goal=self.goal, tstep=self.tstep,
                    episode=self.episode)

    def episode_state_adversary(self):
        """The capability behind the separated runner's one-launch episode on THIS env (mappo_rollout_episode_adversary steps the
        environments inside the rollout kernel): the six state tensors, which that launch reads and stores back, and what it needs
        to step them."""
        return dict(scenario="simple_adversary", N=self.N, M=self.M, L=self.L, T=self.T, seed=self.seed, **self.state_tensors())

    def episode_launch(self, agents, T, deterministic, counter, centralized):
        ops.rollout_episode_adversary(agents, T, self.N, self.T, self.seed, self.agent_pos, self.agent_vel, self.landmark_pos, self.goal,
                                      self.tstep, self.episode, deterministic, counter, centralized)

    def reset(self):
        obs = self._next_out()[:3]
        ops.mpe_adversary_reset(self.agent_pos, self.agent_vel, self.landmark_pos, self.goal, self.tstep, self.episode, *obs, self.N,
                                self.seed, self.M)
        return list(obs)

    def step(self, actions):
        mode, act = self._parse_actions(actions)
        o0, o1, o2, rew, dones = self._next_out()
        ops.mpe_adversary_step(self.agent_pos, self.agent_vel, self.landmark_pos, self.goal, self.tstep, self.episode, act, mode, o0, o1, o2,
                               rew.view(self.N, self.M), dones.view(torch.uint8), self.N, self.T, self.seed, self.M)
        return [o0, o1, o2], rew, dones, None
