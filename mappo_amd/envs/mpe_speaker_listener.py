"""GPU-vectorised MPE `simple_speaker_listener` behind the reference's vec-env contract for agents of DIFFERENT shapes:

    reset() -> [obs_speaker [N, 3], obs_listener [N, 11]]
    step(actions) -> ([obs_speaker, obs_listener], rewards [N, 2, 1], dones [N, 2] bool, infos)

(`onpolicy/envs/env_wrappers.py`, `onpolicy/envs/mpe/environment.py:117-148`, `scenarios/simple_speaker_listener.py`).  The scenario
of the reference's `train_mpe_comm.sh`, which only runs with `share_policy = False`: agent 0, the speaker, does not move, sees the
colour of the goal landmark and says one of 3 symbols (Discrete(3)); agent 1, the listener, is silent, sees its velocity, the three
landmarks and the symbol, and moves (Discrete(5)).  N environments are stepped by ONE kernel launch (csrc/mpe_comm_env.hip) and
everything stays in HBM, so the separated runner can run an episode as one launch (`episode_state_comm`,
mappo_rollout_episode_comm).

`step` takes a list of per-agent tensors — each the reference's one-hot `[N, n_m]` or indices `[N]` / `[N, 1]` — or, with
`accepts_index_actions`, one index tensor `[N, 2]`.  Physics run in float64 as in the reference's NumPy code, with outputs equal
to the fp32 cast of the reference's (tests/golden/mpe_comm.npz); initial states come from a counter-based Philox stream
(seed, episode, env), not from NumPy's global generator."""
import torch

from .. import ops
from ..utils.util import Discrete


class SimpleSpeakerListenerVecEnv:
    graph_safe = True               # step() is one kernel launch on the current stream, no host-side data dependence
    accepts_device_actions = True
    accepts_index_actions = True    # step(actions [N, 2] fp32 indices) is accepted besides the per-agent one-hots
    consumes_actions = True
    ragged_obs = True               # the agents' observations differ in width: reset / step return a per-agent list
    M, L, dim_c = 2, 3, 3
    obs_dims, act_dims = (3, 11), (3, 5)

    def __init__(self, n_rollout_threads, num_agents=2, num_landmarks=3, episode_length=25, seed=1, device="cuda"):
        if int(num_agents) != 2:                                   # simple_speaker_listener.py:16 asserts 2 agents
            raise ValueError(f"simple_speaker_listener has num_agents = 2, a speaker and a listener (got {num_agents})")
        if int(num_landmarks) != 3:                                # :50-52 colours exactly 3 landmarks
            raise ValueError(f"simple_speaker_listener has num_landmarks = 3 (got {num_landmarks})")
        self.N, self.T = int(n_rollout_threads), int(episode_length)
        self.device = torch.device(device)
        self.seed = int(seed)
        self.observation_space = [[d] for d in self.obs_dims]
        self.share_observation_space = [[sum(self.obs_dims)] for _ in range(self.M)]
        self.action_space = [Discrete(n) for n in self.act_dims]
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.listener_pos = torch.zeros(self.N, 2, **f64)
        self.listener_vel = torch.zeros(self.N, 2, **f64)
        self.landmark_pos = torch.zeros(self.N, self.L, 2, **f64)
        self.goal = torch.zeros(self.N, **i32)                     # landmark index of the speaker's goal_b
        self.symbol = torch.full((self.N,), -1, **i32)             # what the channel holds; -1: none (after a reset)
        self.tstep = torch.zeros(self.N, **i32)
        self.episode = torch.zeros(self.N, dtype=torch.int64, device=self.device)
        # two output sets: a consumer may still read the previous env output while this step writes the next one
        self._out = [(torch.empty(self.N, self.obs_dims[0], device=self.device), torch.empty(self.N, self.obs_dims[1], device=self.device),
                      torch.empty(self.N, self.M, 1, device=self.device), torch.empty(self.N, self.M, dtype=torch.bool, device=self.device))
                     for _ in range(2)]
        self._k = 0

    def set_state(self, listener_pos, listener_vel, landmark_pos, goal, tstep=0):
        """Test hook: load explicit states (float64 arrays / tensors [N, 2], [N, 2], [N, 3, 2]; goal [N] landmark indices).  The
        channel is cleared."""
        self.listener_pos.copy_(torch.as_tensor(listener_pos, dtype=torch.float64))
        self.listener_vel.copy_(torch.as_tensor(listener_vel, dtype=torch.float64))
        self.landmark_pos.copy_(torch.as_tensor(landmark_pos, dtype=torch.float64))
        g = torch.as_tensor(goal).to(torch.int32)
        if int(g.min()) < 0 or int(g.max()) >= self.L:
            raise ValueError("goal must be landmark indices 0 .. 2")
        self.goal.copy_(g)
        self.symbol.fill_(-1)
        self.tstep.fill_(int(tstep))

    def state_tensors(self):
        return dict(listener_pos=self.listener_pos, listener_vel=self.listener_vel, landmark_pos=self.landmark_pos, goal=self.goal,
                    symbol=self.symbol, tstep=self.tstep, episode=self.episode)

    def episode_state_comm(self):
        """The capability behind the separated runner's one-launch episode on THIS env (mappo_rollout_episode_comm steps the
        environments inside the rollout kernel): the seven state tensors, which that launch reads and stores back, and what it
        needs to step them."""
        return dict(scenario="simple_speaker_listener", N=self.N, M=self.M, L=self.L, T=self.T, seed=self.seed, **self.state_tensors())

    def reset(self):
        obs_s, obs_l = self._out[self._k][:2]
        ops.mpe_comm_reset(self.listener_pos, self.listener_vel, self.landmark_pos, self.goal, self.symbol, self.tstep, self.episode, obs_s,
                           obs_l, self.N, self.seed)
        self._k ^= 1
        return [obs_s, obs_l]

    def _bad_actions(self, what):
        return ValueError(f"SimpleSpeakerListenerVecEnv.step: {what}: expected a list of two per-agent tensors, each one-hot [N, 3] / "
                          f"[N, 5] or indices [N] / [N, 1], or one index tensor [N, 2], with N = {self.N}")

    def step(self, actions):
        f32 = lambda a: (a if torch.is_tensor(a) else torch.as_tensor(a)).to(self.device, torch.float32)
        if isinstance(actions, (list, tuple)):
            if len(actions) != self.M:
                raise self._bad_actions(f"{len(actions)} per-agent entries")
            a = [f32(x) for x in actions]
            if all(tuple(x.shape) == (self.N, n) for x, n in zip(a, self.act_dims)):
                mode, a_s, a_l = 0, a[0].contiguous(), a[1].contiguous()
            elif all(tuple(x.shape) in ((self.N,), (self.N, 1)) for x in a):
                mode, a_s, a_l = 1, torch.stack([x.reshape(self.N) for x in a], dim=1), None
            else:
                raise self._bad_actions(f"per-agent actions of shapes {[tuple(x.shape) for x in a]}")
        else:
            a = f32(actions)
            if tuple(a.shape) not in ((self.N, self.M), (self.N, self.M, 1)):
                raise self._bad_actions(f"actions of shape {tuple(a.shape)}")
            mode, a_s, a_l = 1, a.reshape(self.N, self.M).contiguous(), None
        obs_s, obs_l, rew, dones = self._out[self._k]
        self._k ^= 1
        ops.mpe_comm_step(self.listener_pos, self.listener_vel, self.landmark_pos, self.goal, self.symbol, self.tstep, self.episode, a_s, a_l,
                          mode, obs_s, obs_l, rew.view(self.N, self.M), dones.view(torch.uint8), self.N, self.T, self.seed)
        return [obs_s, obs_l], rew, dones, None

    def close(self):
        pass
