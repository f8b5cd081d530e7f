"""GPU-vectorised MPE `simple_world_comm` behind the reference's vec-env contract for agents of DIFFERENT shapes, DIFFERENT rewards and
DIFFERENT action spaces:

    reset() -> [obs_adv0 .. obs_adv3 [N, 34], obs_good0, obs_good1 [N, 28]]
    step(actions) -> ([the six observations], rewards [N, 6, 1], dones [N, 6] bool, infos)

(`onpolicy/envs/env_wrappers.py`, `onpolicy/envs/mpe/environment.py:117-256`, `scenarios/simple_world_comm.py`).  The reference's
`train_mpe.py` starts it with `--scenario_name simple_world_comm --num_adversaries 4 --num_good_agents 2 --num_landmarks 1`: agents
0..3, the slower adversaries, chase agents 4 and 5, the faster and smaller good agents, who collect two food items and may hide in two
forests.  An agent sees another one only if both are in the same forest or both are in none — except agent 0, the adversaries'
LEADER, who sees everybody and says one of four words that every adversary hears in the same step.  So `action_space[0]` is
`MultiDiscrete([[0, 4], [0, 3]])` (move, word) and the other five are `Discrete(5)`; the separated runner takes such an env because it
declares `accepts_multidiscrete_agents`.  The world is not collaborative, so `rewards[:, m]` is agent m's OWN reward.  The two
observation widths force `share_policy = False`.  N environments are stepped by ONE kernel launch (csrc/mpe_world_comm_env.hip) and
everything stays in HBM, so the separated runner can run an episode as one launch (`episode_launch`, an attribute the env has only then,
mappo_rollout_episode_world_comm: the six actors and the env steps; the critics run once afterwards, `episode_critics_after`).  That
path is opt-in, MAPPO_WORLD_COMM_EPISODE=1 (`episode_default` is "0"): it samples with the one-launch step's arithmetic, which is not
the stepwise collect's to the bit.  What the six envs of this kind share is in mpe_ragged.py.

`step` takes
  * the reference's one-hots as a per-agent list: `[N, 9]` for the leader (its two heads side by side), `[N, 5]` for the others;
  * or indices: one tensor `[N, 7]` in the column order leader move, leader word, agents 1..5 (`accepts_index_actions`), or a
    per-agent list of `[N, 2]` for the leader and `[N]` / `[N, 1]` for the others.
Physics run in float64 as in the reference's NumPy code, with float outputs within 1e-6 of the fp32 cast of the reference's
(tests/golden/mpe_world_comm.npz; the contact force goes through exp and log, which are not NumPy's to the bit) and the in_forest
flags, the zeros of hidden agents, the word and the dones equal; initial states come from a counter-based Philox stream (seed,
episode, env), not from NumPy's global generator."""
import os

import torch

from ..utils.util import Discrete, MultiDiscrete
from .mpe_ragged import F64, I32, I64, RaggedMPEVecEnv


class SimpleWorldCommVecEnv(RaggedMPEVecEnv):
    scenario, M, L = "simple_world_comm", 6, 5                      # L: landmark, food0, food1, forest0, forest1
    obs_dims, act_dims = (34, 34, 34, 34, 28, 28), (9, 5, 5, 5, 5, 5)
    state = (("agent_pos", F64, (M, 2), 0), ("agent_vel", F64, (M, 2), 0), ("landmark_pos", F64, (L, 2), 0), ("tstep", I32, (), 0),
             ("episode", I64, (), 0))
    env_ops = ("mpe_world_comm_reset", "mpe_world_comm_step", "rollout_episode_world_comm")
    accepts_multidiscrete_agents = True                             # step takes K index columns / K one-hots side by side per such agent
    episode_flag = "MAPPO_WORLD_COMM_EPISODE"                       # "1": the separated runner's one-launch episode; unset / "0": stepwise
    episode_default = "0"                                           # opt-in: the stepwise collect does not sample with the launch's bits
    episode_critics_after = True                                    # the launch runs actors + env; the runner runs the critics after it

    def __init__(self, n_rollout_threads, num_agents=6, episode_length=25, seed=1, device="cuda", num_adversaries=4, num_good_agents=2,
                 num_landmarks=1):
        if (int(num_agents), int(num_adversaries), int(num_good_agents), int(num_landmarks)) != (6, 4, 2, 1):
            raise ValueError(f"simple_world_comm is built for num_agents = 6: 4 adversaries (the first their leader), 2 good agents, "
                             f"1 landmark (got num_agents {num_agents}, num_adversaries {num_adversaries}, num_good_agents "
                             f"{num_good_agents}, num_landmarks {num_landmarks})")
        super().__init__(n_rollout_threads, episode_length, seed, device)
        self.action_space = [MultiDiscrete([[0, 4], [0, 3]])] + [Discrete(5) for _ in range(self.M - 1)]      # environment.py:62-90

    def set_state(self, agent_pos, agent_vel, landmark_pos, tstep=0):
        """Test hook: load explicit states (float64 arrays / tensors [N, 6, 2], [N, 6, 2], [N, 5, 2]).  `episode`, the reset counter
        that keys the Philox stream, is left as it is."""
        self.agent_pos.copy_(torch.as_tensor(agent_pos, dtype=torch.float64))
        self.agent_vel.copy_(torch.as_tensor(agent_vel, dtype=torch.float64))
        self.landmark_pos.copy_(torch.as_tensor(landmark_pos, dtype=torch.float64))
        self.tstep.fill_(int(tstep))

    @property
    def episode_launch(self):
        """The capability behind the separated runner's one-launch episode.  It is opt-in, so an env of a run that did not ask for it
        (MAPPO_WORLD_COMM_EPISODE unset or "0") does not have the attribute at all: whoever asks `hasattr(env, "episode_launch")`
        — the runner, and everything written before this path existed — sees the stepwise env it always saw.
        Caveats: the answer follows os.environ at the time of the access, not of construction; the runner gates on
        episode_default by itself, so this does no work of its own there; and it is the instance that lacks the attribute — the
        class always shows the property (scripts/time_separated_episode.py asks the class)."""
        if os.environ.get(self.episode_flag, self.episode_default) == "0":
            raise AttributeError("episode_launch: the one-launch episode of simple_world_comm is opt-in (MAPPO_WORLD_COMM_EPISODE=1)")
        return super().episode_launch

    def _obs_args(self, obs):
        return (obs,)                                               # six outputs: the entry points take them as one pointer array

    def _bad_actions(self, what):
        return ValueError(f"{type(self).__name__}.step: {what}: expected a list of 6 per-agent tensors — one-hots [N, 9] (the leader's move "
                          f"and word side by side) and [N, 5] x 5, or indices [N, 2] (move, word) and [N] / [N, 1] x 5 — or one index tensor "
                          f"[N, 7] (leader move, leader word, agents 1..5), with N = {self.N}")

    def _parse_actions(self, actions):
        """-> (mode, packed).  mode 0: the list of per-agent one-hots [N, 9], [N, 5] x 5; mode 1: indices [N, 7]."""
        N, M = self.N, self.M
        f32 = lambda a: (a if torch.is_tensor(a) else torch.as_tensor(a)).to(self.device, torch.float32)
        if isinstance(actions, (list, tuple)):
            if len(actions) != M:
                raise self._bad_actions(f"{len(actions)} per-agent entries")
            a = [f32(x) for x in actions]
            if all(tuple(x.shape) == (N, n) for x, n in zip(a, self.act_dims)):
                return 0, [x.contiguous() for x in a]
            if tuple(a[0].shape) == (N, 2) and all(tuple(x.shape) in ((N,), (N, 1)) for x in a[1:]):
                return 1, torch.cat([a[0]] + [x.reshape(N, 1) for x in a[1:]], dim=1)
            raise self._bad_actions(f"per-agent actions of shapes {[tuple(x.shape) for x in a]}")
        a = f32(actions)
        if tuple(a.shape) == (N, M + 1):
            return 1, a.contiguous()
        raise self._bad_actions(f"actions of shape {tuple(a.shape)}")
