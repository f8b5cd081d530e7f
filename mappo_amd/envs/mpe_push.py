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
observation widths force `share_policy = False`.  N environments are stepped by ONE kernel launch (csrc/mpe_push_env.hip) and
everything stays in HBM, so the separated runner can run an episode as one launch (`episode_launch`, mappo_rollout_episode_push).
What the envs of this kind share is in mpe_ragged.py.

`step` takes a list of per-agent tensors — each the reference's one-hot `[N, 5]` or indices `[N]` / `[N, 1]` — or one tensor: the
one-hots `[N, 2, 5]` or, with `accepts_index_actions`, indices `[N, 2]` / `[N, 2, 1]`.  Physics run in float64 as in the
reference's NumPy code, with outputs within 1e-6 of the fp32 cast of the reference's (tests/golden/mpe_push.npz; the contact force
goes through exp and log, which are not NumPy's to the bit); initial states come from a counter-based Philox stream (seed, episode,
env), not from NumPy's global generator."""
import torch

from .. import ops
from .mpe_ragged import RaggedMPEVecEnv


class SimplePushVecEnv(RaggedMPEVecEnv):
    M, L = 2, 2
    obs_dims, act_dims = (8, 19), (5, 5)
    episode_flag = "MAPPO_PUSH_EPISODE"

    def __init__(self, n_rollout_threads, num_agents=2, episode_length=25, seed=1, device="cuda", num_landmarks=2):
        if (int(num_agents), int(num_landmarks)) != (2, 2):
            raise ValueError(f"simple_push is built for num_agents = 2: 1 adversary, 1 good agent, 2 landmarks (got num_agents {num_agents}, "
                             f"num_landmarks {num_landmarks})")
        super().__init__(n_rollout_threads, episode_length, seed, device)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.agent_pos = torch.zeros(self.N, self.M, 2, **f64)
        self.agent_vel = torch.zeros(self.N, self.M, 2, **f64)
        self.landmark_pos = torch.zeros(self.N, self.L, 2, **f64)
        self.goal = torch.zeros(self.N, **i32)                     # landmark index of both agents' goal_a
        self.tstep = torch.zeros(self.N, **i32)
        self.episode = torch.zeros(self.N, dtype=torch.int64, device=self.device)

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

    def state_tensors(self):
        return dict(agent_pos=self.agent_pos, agent_vel=self.agent_vel, landmark_pos=self.landmark_pos, goal=self.goal, tstep=self.tstep,
                    episode=self.episode)

    def episode_launch(self, agents, T, deterministic, counter, centralized):
        ops.rollout_episode_push(agents, T, self.N, self.T, self.seed, self.agent_pos, self.agent_vel, self.landmark_pos, self.goal,
                                 self.tstep, self.episode, deterministic, counter, centralized)

    def reset(self):
        obs = self._next_out()[:2]
        ops.mpe_push_reset(self.agent_pos, self.agent_vel, self.landmark_pos, self.goal, self.tstep, self.episode, *obs, self.N, self.seed,
                           self.M)
        return list(obs)

    def step(self, actions):
        mode, act = self._parse_actions(actions)
        o0, o1, rew, dones = self._next_out()
        ops.mpe_push_step(self.agent_pos, self.agent_vel, self.landmark_pos, self.goal, self.tstep, self.episode, act, mode, o0, o1,
                          rew.view(self.N, self.M), dones.view(torch.uint8), self.N, self.T, self.seed, self.M)
        return [o0, o1], rew, dones, None
