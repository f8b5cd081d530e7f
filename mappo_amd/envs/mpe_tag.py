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
everything stays in HBM, so the
separated runner can run an episode as one launch (`episode_state_tag`, mappo_rollout_episode_tag).

`step` takes a list of per-agent tensors — each the reference's one-hot `[N, 5]` or indices `[N]` / `[N, 1]` — or one tensor: the
one-hots `[N, 4, 5]` or, with `accepts_index_actions`, indices `[N, 4]` / `[N, 4, 1]`.  Physics run in float64 as in the
reference's NumPy code, with outputs within 1e-6 of the fp32 cast of the reference's (tests/golden/mpe_tag.npz; the contact force
goes through exp and log, which are not NumPy's to the bit); initial states come from a counter-based Philox stream (seed, episode,
env), not from NumPy's global generator."""
import torch

from .. import ops
from ..utils.util import Discrete


class SimpleTagVecEnv:
    graph_safe = True               # step() is one kernel launch on the current stream, no host-side data dependence
    accepts_device_actions = True
    accepts_index_actions = True    # step(actions [N, 4] fp32 indices) is accepted besides the one-hots
    consumes_actions = True
    ragged_obs = True               # the agents' observations differ in width: reset / step return a per-agent list
    M, L = 4, 2
    obs_dims, act_dims = (16, 16, 16, 14), (5, 5, 5, 5)

    def __init__(self, n_rollout_threads, num_agents=4, episode_length=25, seed=1, device="cuda", num_adversaries=3, num_good_agents=1,
                 num_landmarks=2):
        if (int(num_agents), int(num_adversaries), int(num_good_agents), int(num_landmarks)) != (4, 3, 1, 2):
            raise ValueError(f"simple_tag is built for num_agents = 4: 3 adversaries, 1 good agent, 2 landmarks (got num_agents {num_agents}, "
                             f"num_adversaries {num_adversaries}, num_good_agents {num_good_agents}, num_landmarks {num_landmarks})")
        self.N, self.T = int(n_rollout_threads), int(episode_length)
        self.device = torch.device(device)
        self.seed = int(seed)
        self.observation_space = [[d] for d in self.obs_dims]
        self.share_observation_space = [[sum(self.obs_dims)] for _ in range(self.M)]
        self.action_space = [Discrete(n) for n in self.act_dims]
        f64 = dict(dtype=torch.float64, device=self.device)
        self.agent_pos = torch.zeros(self.N, self.M, 2, **f64)
        self.agent_vel = torch.zeros(self.N, self.M, 2, **f64)
        self.landmark_pos = torch.zeros(self.N, self.L, 2, **f64)
        self.tstep = torch.zeros(self.N, dtype=torch.int32, device=self.device)
        self.episode = torch.zeros(self.N, dtype=torch.int64, device=self.device)
        # two output sets: a consumer may still read the previous env output while this step writes the next one
        self._out = [tuple(torch.empty(self.N, d, device=self.device) for d in self.obs_dims) +
                     (torch.empty(self.N, self.M, 1, device=self.device), torch.empty(self.N, self.M, dtype=torch.bool, device=self.device))
                     for _ in range(2)]
        self._k = 0

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

    def reset(self):
        obs = self._out[self._k][:4]
        ops.mpe_tag_reset(self.agent_pos, self.agent_vel, self.landmark_pos, self.tstep, self.episode, *obs, self.N, self.seed, self.M)
        self._k ^= 1
        return list(obs)

    def _bad_actions(self, what):
        return ValueError(f"SimpleTagVecEnv.step: {what}: expected a list of four per-agent tensors, each one-hot [N, 5] or "
                          f"indices [N] / [N, 1], or one tensor of one-hots [N, 4, 5] or indices [N, 4], with N = {self.N}")

    def step(self, actions):
        f32 = lambda a: (a if torch.is_tensor(a) else torch.as_tensor(a)).to(self.device, torch.float32)
        if isinstance(actions, (list, tuple)):
            if len(actions) != self.M:
                raise self._bad_actions(f"{len(actions)} per-agent entries")
            a = [f32(x) for x in actions]
            if all(tuple(x.shape) == (self.N, 5) for x in a):
                mode, act = 0, torch.stack(a, dim=1)
            elif all(tuple(x.shape) in ((self.N,), (self.N, 1)) for x in a):
                mode, act = 1, torch.stack([x.reshape(self.N) for x in a], dim=1)
            else:
                raise self._bad_actions(f"per-agent actions of shapes {[tuple(x.shape) for x in a]}")
        else:
            a = f32(actions)
            if tuple(a.shape) == (self.N, self.M, 5):
                mode, act = 0, a.contiguous()
            elif tuple(a.shape) in ((self.N, self.M), (self.N, self.M, 1)):
                mode, act = 1, a.reshape(self.N, self.M).contiguous()
            else:
                raise self._bad_actions(f"actions of shape {tuple(a.shape)}")
        o0, o1, o2, o3, rew, dones = self._out[self._k]
        self._k ^= 1
        ops.mpe_tag_step(self.agent_pos, self.agent_vel, self.landmark_pos, self.tstep, self.episode, act, mode, o0, o1, o2, o3,
                         rew.view(self.N, self.M), dones.view(torch.uint8), self.N, self.T, self.seed, self.M)
        return [o0, o1, o2, o3], rew, dones, None

    def close(self):
        pass
