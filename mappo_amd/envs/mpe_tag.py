"""GPU-vectorised MPE `simple_tag` (predator-prey) behind the reference's vec-env contract for agents of DIFFERENT shapes and
DIFFERENT rewards:

    reset() -> [obs_adv0 [N, 16], obs_adv1 [N, 16], obs_adv2 [N, 16], obs_good [N, 14]]
    step(actions) -> ([obs_adv0, obs_adv1, obs_adv2, obs_good], rewards [N, 4, 1], dones [N, 4] bool, infos)

(`onpolicy/envs/env_wrappers.py`, `onpolicy/envs/mpe/environment.py:117-148`, `scenarios/simple_tag.py`).  The reference's
`train_mpe.py` starts it with `--scenario_name simple_tag --num_adversaries 3 --num_good_agents 1 --num_landmarks 2`: agents 0..2, the
slower adversaries, are paid 10 for every adversary touching the good agent; agent 3, the faster and smaller good agent, loses 10 per
contact and pays for leaving the arena.  Agents collide with each other and with the two landmarks, and each has its own accel,
max_speed and size.  Every agent moves (Discrete(5)).  The world is not collaborative, so `rewards[:, m]` is agent m's OWN reward.
The two observation widths force `share_policy = False`.  N environments are stepped by ONE kernel launch (csrc/mpe_ragged_env.hip
on csrc/mpe_tag_core.h) and everything stays in HBM, so the separated runner can run an episode as one launch (`episode_launch`,
mappo_rollout_episode_tag).  What the six envs of this kind share — all but the description below — is in mpe_ragged.py.

`step` takes a list of per-agent tensors — each the reference's one-hot `[N, 5]` or indices `[N]` / `[N, 1]` — or one tensor: the
one-hots `[N, 4, 5]` or, with `accepts_index_actions`, indices `[N, 4]` / `[N, 4, 1]`.  Physics run in float64 as in the
reference's NumPy code, with outputs within 1e-6 of the fp32 cast of the reference's (tests/golden/mpe_tag.npz; the contact force
goes through exp and log, which are not NumPy's to the bit); initial states come from a counter-based Philox stream (seed, episode,
env), not from NumPy's global generator."""
import torch

from .mpe_ragged import F64, I32, I64, RaggedMPEVecEnv


class SimpleTagVecEnv(RaggedMPEVecEnv):
    scenario, M, L = "simple_tag", 4, 2
    obs_dims, act_dims = (16, 16, 16, 14), (5, 5, 5, 5)
    episode_flag = "MAPPO_TAG_EPISODE"
    state = (("agent_pos", F64, (M, 2), 0), ("agent_vel", F64, (M, 2), 0), ("landmark_pos", F64, (L, 2), 0), ("tstep", I32, (), 0),
             ("episode", I64, (), 0))
    env_ops = ("mpe_tag_reset", "mpe_tag_step", "rollout_episode_tag")
    episode_state_tag = RaggedMPEVecEnv.episode_state             # the name this scenario's tests call

    def __init__(self, n_rollout_threads, num_agents=4, episode_length=25, seed=1, device="cuda", num_adversaries=3, num_good_agents=1,
                 num_landmarks=2):
        if (int(num_agents), int(num_adversaries), int(num_good_agents), int(num_landmarks)) != (4, 3, 1, 2):
            raise ValueError(f"simple_tag is built for num_agents = 4: 3 adversaries, 1 good agent, 2 landmarks (got num_agents {num_agents}, "
                             f"num_adversaries {num_adversaries}, num_good_agents {num_good_agents}, num_landmarks {num_landmarks})")
        super().__init__(n_rollout_threads, episode_length, seed, device)

    def set_state(self, agent_pos, agent_vel, landmark_pos, tstep=0):
        """Test hook: load explicit states (float64 arrays / tensors [N, 4, 2], [N, 4, 2], [N, 2, 2]).  `episode`, the reset counter
        that keys the Philox stream, is left as it is."""
        self.agent_pos.copy_(torch.as_tensor(agent_pos, dtype=torch.float64))
        self.agent_vel.copy_(torch.as_tensor(agent_vel, dtype=torch.float64))
        self.landmark_pos.copy_(torch.as_tensor(landmark_pos, dtype=torch.float64))
        self.tstep.fill_(int(tstep))
