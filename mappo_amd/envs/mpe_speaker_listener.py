"""GPU-vectorised MPE `simple_speaker_listener` behind the reference's vec-env contract for agents of DIFFERENT shapes:

    reset() -> [obs_speaker [N, 3], obs_listener [N, 11]]
    step(actions) -> ([obs_speaker, obs_listener], rewards [N, 2, 1], dones [N, 2] bool, infos)

(`onpolicy/envs/env_wrappers.py`, `onpolicy/envs/mpe/environment.py:117-148`, `scenarios/simple_speaker_listener.py`).  The scenario
of the reference's `train_mpe_comm.sh`, which only runs with `share_policy = False`: agent 0, the speaker, does not move, sees the
colour of the goal landmark and says one of 3 symbols (Discrete(3)); agent 1, the listener, is silent, sees its velocity, the three
landmarks and the symbol, and moves (Discrete(5)).  N environments are stepped by ONE kernel launch (csrc/mpe_comm_env.hip) and
everything stays in HBM, so the separated runner can run an episode as one launch (`episode_launch`,
mappo_rollout_episode_comm).  What the three envs of this kind share is in mpe_ragged.py.

`step` takes a list of per-agent tensors — each the reference's one-hot `[N, n_m]` or indices `[N]` / `[N, 1]` — or, with
`accepts_index_actions`, one index tensor `[N, 2]`.  Physics run in float64 as in the reference's NumPy code, with outputs equal
to the fp32 cast of the reference's (tests/golden/mpe_comm.npz); initial states come from a counter-based Philox stream
(seed, episode, env), not from NumPy's global generator."""
import torch

from .. import ops
from .mpe_ragged import RaggedMPEVecEnv


class SimpleSpeakerListenerVecEnv(RaggedMPEVecEnv):
    M, L, dim_c = 2, 3, 3
    obs_dims, act_dims = (3, 11), (3, 5)
    episode_flag = "MAPPO_COMM_EPISODE"

    def __init__(self, n_rollout_threads, num_agents=2, num_landmarks=3, episode_length=25, seed=1, device="cuda"):
        if int(num_agents) != 2:                                   # simple_speaker_listener.py:16 asserts 2 agents
            raise ValueError(f"simple_speaker_listener has num_agents = 2, a speaker and a listener (got {num_agents})")
        if int(num_landmarks) != 3:                                # :50-52 colours exactly 3 landmarks
            raise ValueError(f"simple_speaker_listener has num_landmarks = 3 (got {num_landmarks})")
        super().__init__(n_rollout_threads, episode_length, seed, device)
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.listener_pos = torch.zeros(self.N, 2, **f64)
        self.listener_vel = torch.zeros(self.N, 2, **f64)
        self.landmark_pos = torch.zeros(self.N, self.L, 2, **f64)
        self.goal = torch.zeros(self.N, **i32)                     # landmark index of the speaker's goal_b
        self.symbol = torch.full((self.N,), -1, **i32)             # what the channel holds; -1: none (after a reset)
        self.tstep = torch.zeros(self.N, **i32)
        self.episode = torch.zeros(self.N, dtype=torch.int64, device=self.device)

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

    def episode_launch(self, agents, T, deterministic, counter, centralized):
        ops.rollout_episode_comm(agents[0], agents[1], T, self.N, self.T, self.seed, self.listener_pos, self.listener_vel, self.landmark_pos,
                                 self.goal, self.symbol, self.tstep, self.episode, deterministic, counter, centralized)

    def reset(self):
        obs_s, obs_l = self._next_out()[:2]
        ops.mpe_comm_reset(self.listener_pos, self.listener_vel, self.landmark_pos, self.goal, self.symbol, self.tstep, self.episode, obs_s,
                           obs_l, self.N, self.seed)
        return [obs_s, obs_l]

    def step(self, actions):
        mode, act = self._parse_actions(actions)
        a_s, a_l = act if mode == 0 else (act, None)                # one-hots: two tensors of different widths
        obs_s, obs_l, rew, dones = self._next_out()
        ops.mpe_comm_step(self.listener_pos, self.listener_vel, self.landmark_pos, self.goal, self.symbol, self.tstep, self.episode, a_s, a_l,
                          mode, obs_s, obs_l, rew.view(self.N, self.M), dones.view(torch.uint8), self.N, self.T, self.seed)
        return [obs_s, obs_l], rew, dones, None
