"""GPU-vectorised MPE `simple_crypto` behind the reference's vec-env contract for agents of DIFFERENT shapes and DIFFERENT rewards:

    reset() -> [obs_eve [N, 4], obs_bob [N, 8], obs_alice [N, 8]]
    step(actions) -> ([obs_eve, obs_bob, obs_alice], rewards [N, 3, 1], dones [N, 3] bool, infos)

(`onpolicy/envs/env_wrappers.py`, `onpolicy/envs/mpe/environment.py:117-148`, `scenarios/simple_crypto.py`).  The reference's
`train_mpe.py` starts it with `--scenario_name simple_crypto --num_agents 3 --num_landmarks 2` (3 and 4 landmarks work as well;
beyond 4 the reference itself raises an IndexError).  Agent 0, the adversary "Eve", hears what the speaker said; agent 1, the good
listener "Bob", also holds the key; agent 2, the speaker "Alice", sees the goal and the key.  Nobody moves: every agent only says one
of `dim_c` = 4 symbols (Discrete(4)), and landmark k's colour is the one-hot e_k.  The world is not collaborative, so `rewards[:, m]`
is agent m's OWN reward: with d(a) = |c_a - e_goal|^2, Eve gets -d(Eve), Bob and Alice d(Eve) - d(Bob) — every value -2, 0 or 2.
The two observation widths force `share_policy = False`.  N environments are stepped by ONE kernel launch (csrc/mpe_ragged_env.hip
on csrc/mpe_crypto_core.h) and everything stays in HBM, so the separated runner can run an episode as one launch (`episode_launch`,
mappo_rollout_episode_crypto).  What the six envs of this kind share — all but the description below — is in mpe_ragged.py.

`step` takes a list of per-agent tensors — each the reference's one-hot `[N, 4]` or indices `[N]` / `[N, 1]` — or one tensor: the
one-hots `[N, 3, 4]` or, with `accepts_index_actions`, indices `[N, 3]` / `[N, 3, 1]`.  The whole state is integers (goal, key, the
symbol each agent last said), every output is a one-hot, zeros or -2 / 0 / 2, and so equals the fp32 cast of the reference's
(tests/golden/mpe_crypto.npz); goal and key come from a counter-based Philox stream (seed, episode, env), not from NumPy's global
generator."""
import torch

from .mpe_ragged import I32, I64, RaggedMPEVecEnv


class SimpleCryptoVecEnv(RaggedMPEVecEnv):
    scenario, M, C = "simple_crypto", 3, 4
    obs_dims, act_dims = (4, 8, 8), (4, 4, 4)
    episode_flag = "MAPPO_CRYPTO_EPISODE"
    state = (("goal", I32, (), 0),                                 # landmark index of every agent's goal_a
             ("key", I32, (), 0),                                  # landmark index of the speaker's key
             ("comm", I32, (M,), -1),                              # the symbol each agent last said, -1: nothing said
             ("tstep", I32, (), 0), ("episode", I64, (), 0))
    env_ops = ("mpe_crypto_reset", "mpe_crypto_step", "rollout_episode_crypto")
    shape_args, episode_shape_args = ("M", "L"), ("L",)            # L, this env's num_landmarks, is the instance's

    def __init__(self, n_rollout_threads, num_agents=3, num_landmarks=2, episode_length=25, seed=1, device="cuda"):
        if int(num_agents) != 3 or not 2 <= int(num_landmarks) <= 4:
            raise ValueError(f"simple_crypto is built for num_agents = 3 (adversary Eve, listener Bob, speaker Alice) and num_landmarks = 2, "
                             f"3 or 4, a landmark's colour being a one-hot of dim_c = 4 (got num_agents {num_agents}, num_landmarks "
                             f"{num_landmarks})")
        self.L = int(num_landmarks)
        super().__init__(n_rollout_threads, episode_length, seed, device)

    def set_state(self, goal, key, comm=-1, tstep=0):
        """Test hook: load explicit states (goal, key [N] landmark indices 0 .. L - 1; comm [N, 3] symbols 0 .. 3 or -1 for an
        agent that has said nothing, or one such value for all)."""
        g, k = (torch.as_tensor(x).to(torch.int32).reshape(self.N) for x in (goal, key))
        c = torch.as_tensor(comm).to(torch.int32).expand(self.N, self.M)
        for name, t in (("goal", g), ("key", k)):
            if int(t.min()) < 0 or int(t.max()) >= self.L:
                raise ValueError(f"{name} must be landmark indices 0 .. {self.L - 1}")
        if int(c.min()) < -1 or int(c.max()) >= self.C:
            raise ValueError(f"comm must be symbols 0 .. {self.C - 1}, or -1 for nothing said")
        self.goal.copy_(g)
        self.key.copy_(k)
        self.comm.copy_(c)
        self.tstep.fill_(int(tstep))
