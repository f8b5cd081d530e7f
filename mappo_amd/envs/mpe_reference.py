"""GPU-vectorised MPE `simple_reference` behind the reference's vec-env contract:

    reset() -> obs [N, 2, 21];  step(actions_env) -> (obs [N, 2, 21], rewards [N, 2, 1], dones [N, 2] bool, infos)

(`onpolicy/envs/env_wrappers.py:262-272`, `onpolicy/envs/mpe/environment.py:117-148`, `scenarios/simple_reference.py`).  The
scenario of the reference's `train_mpe_reference.sh`: 2 agents, 3 landmarks, each agent knows the landmark the OTHER one has to
reach and can only say so over a 10-symbol channel — action space MultiDiscrete([[0, 4], [0, 9]]) (move, say).  N environments
are stepped by ONE kernel launch (csrc/mpe_ref_env.hip: action -> force and communication, damping + integration, shared
reward, observations, time-limit done, reset-on-done) and everything stays in HBM, so the runner can capture an episode into a
hipGraph (`graph_safe`) or run it as one launch (`episode_state_reference`, mappo_rollout_episode_reference).

`step` takes the reference's `actions_env [N, 2, 15]` (the heads' one-hots side by side) or — `accepts_index_actions` — the
buffer's own head indices `[N, 2, 2]` (fp32).  Physics run in float64 as in the reference's NumPy code, with outputs equal to
the fp32 cast of the reference's (tests/golden/mpe_envs.npz); initial states come from a counter-based Philox stream
(seed, episode, env), not from NumPy's global generator."""
import torch

from .. import ops
from ..utils.util import MultiDiscrete


class SimpleReferenceVecEnv:
    graph_safe = True               # step() is one kernel launch on the current stream, no host-side data dependence
    accepts_device_actions = True
    accepts_index_actions = True    # step(actions [N, 2, 2] fp32 head indices) is accepted besides the one-hot actions_env
    consumes_actions = True
    M, L, dim_c, obs_dim = 2, 3, 10, 21

    def __init__(self, n_rollout_threads, num_agents=2, num_landmarks=3, episode_length=25, seed=1, device="cuda"):
        if int(num_agents) != 2 or int(num_landmarks) != 3:       # simple_reference.py:14-15 asserts 2 agents, :47-49 colours 3 landmarks
            raise ValueError(f"simple_reference has 2 agents and 3 landmarks (got {num_agents}, {num_landmarks})")
        self.N, self.T = int(n_rollout_threads), int(episode_length)
        self.device = torch.device(device)
        self.seed = int(seed)
        self.observation_space = [[self.obs_dim] for _ in range(self.M)]
        self.share_observation_space = [[self.obs_dim * self.M] for _ in range(self.M)]
        self.action_space = [MultiDiscrete([[0, 4], [0, self.dim_c - 1]]) for _ in range(self.M)]      # environment.py:62-86
        f64 = dict(dtype=torch.float64, device=self.device)
        self.agent_pos = torch.zeros(self.N, self.M, 2, **f64)
        self.agent_vel = torch.zeros(self.N, self.M, 2, **f64)
        self.landmark_pos = torch.zeros(self.N, self.L, 2, **f64)
        self.goal = torch.zeros(self.N, self.M, dtype=torch.int32, device=self.device)      # landmark index of each agent's goal_b
        self.tstep = torch.zeros(self.N, dtype=torch.int32, device=self.device)
        self.episode = torch.zeros(self.N, dtype=torch.int64, device=self.device)
        # two output sets: the runner's fused step reads the previous env output while this step writes the next one
        self._out = [(torch.empty(self.N, self.M, self.obs_dim, device=self.device), torch.empty(self.N, self.M, 1, device=self.device),
                      torch.empty(self.N, self.M, dtype=torch.bool, device=self.device)) for _ in range(2)]
        self._k = 0

    def set_state(self, agent_pos, agent_vel, landmark_pos, goals, tstep=0):
        """Test hook: load explicit states (float64 arrays / tensors [N, 2|3, 2], goals [N, 2] landmark indices)."""
        self.agent_pos.copy_(torch.as_tensor(agent_pos, dtype=torch.float64))
        self.agent_vel.copy_(torch.as_tensor(agent_vel, dtype=torch.float64))
        self.landmark_pos.copy_(torch.as_tensor(landmark_pos, dtype=torch.float64))
        g = torch.as_tensor(goals).to(torch.int32)
        if int(g.min()) < 0 or int(g.max()) >= self.L:
            raise ValueError("goals must be landmark indices 0 .. 2")
        self.goal.copy_(g)
        self.tstep.fill_(int(tstep))

    def episode_state_reference(self):
        """The capability behind the runner's one-launch episode on THIS env (mappo_rollout_episode_reference steps the
        environments inside the rollout kernel): the six state tensors, which that launch reads and stores back, and what it
        needs to step them."""
        return dict(scenario="simple_reference", agent_pos=self.agent_pos, agent_vel=self.agent_vel, landmark_pos=self.landmark_pos,
                    goal=self.goal, tstep=self.tstep, episode=self.episode, N=self.N, M=self.M, L=self.L, T=self.T, seed=self.seed)

    def reset(self):
        obs = self._out[self._k][0]
        ops.mpe_reference_reset(self.agent_pos, self.agent_vel, self.landmark_pos, self.goal, self.tstep, self.episode, obs, self.N,
                                self.seed)
        self._k ^= 1
        return obs

    def step(self, actions):
        a = actions if torch.is_tensor(actions) else torch.as_tensor(actions)
        if tuple(a.shape) == (self.N, self.M, 5 + self.dim_c):
            mode = 0
        elif tuple(a.shape) == (self.N, self.M, 2):
            mode = 1
        else:
            raise ValueError(f"SimpleReferenceVecEnv.step: actions of shape {tuple(a.shape)}: expected the heads' one-hots "
                             f"[N, 2, 15] or head indices [N, 2, 2] with N = {self.N}")
        obs, rew, dones = self._out[self._k]
        self._k ^= 1
        a = a.to(self.device, torch.float32)
        ops.mpe_reference_step(self.agent_pos, self.agent_vel, self.landmark_pos, self.goal, self.tstep, self.episode, a.contiguous(), mode,
                               obs, rew, dones.view(torch.uint8), self.N, self.T, self.seed)
        return obs, rew, dones, None

    def close(self):
        pass
