"""GPU-vectorised MPE `simple_speaker_listener` behind the reference's vec-env contract for agents of DIFFERENT shapes:

    reset() -> [obs_speaker [N, 3], obs_listener [N, 11]]
    step(actions) -> ([obs_speaker, obs_listener], rewards [N, 2, 1], dones [N, 2] bool, infos)

(`onpolicy/envs/env_wrappers.py`, `onpolicy/envs/mpe/environment.py:117-148`, `scenarios/simple_speaker_listener.py`).  The scenario
of the reference's `train_mpe_comm.sh`, which only runs with `share_policy = False`: agent 0, the speaker, does not move, sees the
colour of the goal landmark and says one of 3 symbols (Discrete(3)); agent 1, the listener, is silent, sees its velocity, the three
landmarks and the symbol, and moves (Discrete(5)).  N environments are stepped by ONE kernel launch (csrc/mpe_comm_env.hip) and
everything stays in HBM, so the separated runner can run an episode as one launch (`episode_launch`,
mappo_rollout_episode_comm).  What the six envs of this kind share is in mpe_ragged.py; this one's `step` passes the two agents'
one-hots as two pointers and its episode takes the two agents one by one.

`step` takes a list of per-agent tensors — each the reference's one-hot `[N, n_m]` or indices `[N]` / `[N, 1]` — or, with
`accepts_index_actions`, one index tensor `[N, 2]`.  Physics run in float64 as in the reference's NumPy code, with outputs equal
to the fp32 cast of the reference's (tests/golden/mpe_comm.npz); initial states come from a counter-based Philox stream
(seed, episode, env), not from NumPy's global generator."""
import torch

from .. import ops
from .mpe_ragged import F64, I32, I64, RaggedMPEVecEnv


class SimpleSpeakerListenerVecEnv(RaggedMPEVecEnv):
    scenario, M, L, dim_c = "simple_speaker_listener", 2, 3, 3
    obs_dims, act_dims = (3, 11), (3, 5)
    episode_flag = "MAPPO_COMM_EPISODE"
    state = (("listener_pos", F64, (2,), 0), ("listener_vel", F64, (2,), 0), ("landmark_pos", F64, (L, 2), 0),
             ("goal", I32, (), 0),                                 # landmark index of the speaker's goal_b
             ("symbol", I32, (), -1),                              # what the channel holds; -1: none (after a reset)
             ("tstep", I32, (), 0), ("episode", I64, (), 0))
    env_ops = ("mpe_comm_reset", "mpe_comm_step", "rollout_episode_comm")      # step and the episode take their own forms, below
    shape_args = ()
    episode_state_comm = RaggedMPEVecEnv.episode_state            # the name this scenario's tests call

    def __init__(self, n_rollout_threads, num_agents=2, num_landmarks=3, episode_length=25, seed=1, device="cuda"):
        if int(num_agents) != 2:                                   # simple_speaker_listener.py:16 asserts 2 agents
            raise ValueError(f"simple_speaker_listener has num_agents = 2, a speaker and a listener (got {num_agents})")
        if int(num_landmarks) != 3:                                # :50-52 colours exactly 3 landmarks
            raise ValueError(f"simple_speaker_listener has num_landmarks = 3 (got {num_landmarks})")
        super().__init__(n_rollout_threads, episode_length, seed, device)

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

    def episode_launch(self, agents, T, deterministic, counter, centralized):
        ops.rollout_episode_comm(agents[0], agents[1], T, self.N, self.T, self.seed, *self._tensors, deterministic, counter, centralized)

    def step(self, actions):
        mode, act = self._parse_actions(actions)
        a_s, a_l = act if mode == 0 else (act, None)                # one-hots: two tensors of different widths
        obs_s, obs_l, rew, dones = self._next_out()
        ops.mpe_comm_step(*self._tensors, a_s, a_l, mode, obs_s, obs_l, rew.view(self.N, self.M), dones.view(torch.uint8), self.N, self.T,
                          self.seed)
        return [obs_s, obs_l], rew, dones, None
