"""GPU-vectorised MPE `simple_tag` (predator-prey) behind the reference's vec-env contract for agents of DIFFERENT shapes and
DIFFERENT rewards:

    reset() -> [obs_adv0 [N, 16], obs_adv1 [N, 16], obs_adv2 [N, 16], obs_good [N, 14]]
    step(actions) -> ([obs_adv0, obs_adv1, obs_adv2, obs_good], rewards [N, 4, 1], dones [N, 4] bool, infos)

(`onpolicy/envs/env_wrappers.py`, `onpolicy/envs/mpe/environment.py:117-148`, `scenarios/simple_tag.py`).  The reference's
`train_mpe.py` starts it with `--scenario_name simple_tag --num_adversaries 3 --num_good_agents 1 --num_landmarks 2`: agents 0..2, the
slower adversaries, are paid 10 for every adversary touching the good agent; agent 3, the faster and smaller good agent, loses 10 per
contact and pays for leaving the arena.  Agents collide with each other and with the two landmarks, and each has its own accel,
max_speed and size.  Every agent moves (Discrete(5)).  The world is not collaborative, so `rewards[:, m]` is agent m's OWN reward.
The two observation widths force `share_policy = False`.  N environments are stepped by ONE kernel launch (csrc/mpe_tag_env.hip) and
everything stays in HBM, so the separated runner can run an episode as one launch (`episode_launch`, mappo_rollout_episode_tag).
What the three envs of this kind share is in mpe_ragged.py.

`step` takes a list of per-agent tensors — each the reference's one-hot `[N, 5]` or indices `[N]` / `[N, 1]` — or one tensor: the
one-hots `[N, 4, 5]` or, with `accepts_index_actions`, indices `[N, 4]` / `[N, 4, 1]`.  Physics run in float64 as in the
reference's NumPy code, with outputs within 1e-6 of the fp32 cast of the reference's (tests/golden/mpe_tag.npz; the contact force
goes through exp and log, which are not NumPy's to the bit); initial states come from a counter-based Philox stream (seed, episode,
env), not from NumPy's global generator."""
import torch

from .. import ops
from .mpe_ragged import RaggedMPEVecEnv


class SimpleTagVecEnv(RaggedMPEVecEnv):
    M, L = 4, 2
    obs_dims, act_dims = (16, 16, 16, 14), (5, 5, 5, 5)
    episode_flag = "MAPPO_TAG_EPISODE"

    def __init__(self, n_rollout_threads, num_agents=4, episode_length=25, seed=1, device="cuda", num_adversaries=3, num_good_agents=1,
                 num_landmarks=2):
        if (int(num_agents), int(num_adversaries), int(num_good_agents), int(num_landmarks)) != (4, 3, 1, 2):
            raise ValueError(f"simple_tag is built for num_agents = 4: 3 adversaries, 1 good agent, 2 landmarks (got num_agents {num_agents}, "
                             f"num_adversaries {num_adversaries}, num_good_agents {num_good_agents}, num_landmarks {num_landmarks})")
        super().__init__(n_rollout_threads, episode_length, seed, device)
        f64 = dict(dtype=torch.float64, device=self.device)
        self.agent_pos = torch.zeros(self.N, self.M, 2, **f64)
        self.agent_vel = torch.zeros(self.N, self.M, 2, **f64)
        self.landmark_pos = torch.zeros(self.N, self.L, 2, **f64)
        self.tstep = torch.zeros(self.N, dtype=torch.int32, device=self.device)
        self.episode = torch.zeros(self.N, dtype=torch.int64, device=self.device)

    def set_state(self, agent_pos, agent_vel, landmark_pos, tstep=0):
        """Test hook: load explicit states (float64 arrays / tensors [N, 4, 2], [N, 4, 2], [N, 2, 2]).  `episode`, the reset counter
        that keys the Philox stream, is left as it is."""
        self.agent_pos.copy_(torch.as_tensor(agent_pos, dtype=torch.float64))
        self.agent_vel.copy_(torch.as_tensor(agent_vel, dtype=torch.float64))
        self.landmark_pos.copy_(torch.as_tensor(landmark_pos, dtype=torch.float64))
        self.tstep.fill_(int(tstep))

    def state_tensors(self):
        return dict(agent_pos=self.agent_pos, agent_vel=self.agent_vel, landmark_pos=self.landmark_pos, tstep=self.tstep, episode=self.episode)

    def episode_state_tag(self):
        """The capability behind the separated runner's one-launch episode on THIS env (mappo_rollout_episode_tag steps the
        environments inside the rollout kernel): the five state tensors, which that launch reads and stores back, and what it needs
        to step them."""
        return dict(scenario="simple_tag", N=self.N, M=self.M, L=self.L, T=self.T, seed=self.seed, **self.state_tensors())

    def episode_launch(self, agents, T, deterministic, counter, centralized):
        ops.rollout_episode_tag(agents, T, self.N, self.T, self.seed, self.agent_pos, self.agent_vel, self.landmark_pos, self.tstep,
                                self.episode, deterministic, counter, centralized)

    def reset(self):
        obs = self._next_out()[:4]
        ops.mpe_tag_reset(self.agent_pos, self.agent_vel, self.landmark_pos, self.tstep, self.episode, *obs, self.N, self.seed, self.M)
        return list(obs)

    def step(self, actions):
        mode, act = self._parse_actions(actions)
        o0, o1, o2, o3, rew, dones = self._next_out()
        ops.mpe_tag_step(self.agent_pos, self.agent_vel, self.landmark_pos, self.tstep, self.episode, act, mode, o0, o1, o2, o3,
                         rew.view(self.N, self.M), dones.view(torch.uint8), self.N, self.T, self.seed, self.M)
        return [o0, o1, o2, o3], rew, dones, None
