"""What the six GPU-resident MPE envs with agents of DIFFERENT shapes share (mpe_speaker_listener, mpe_adversary, mpe_tag, mpe_push,
mpe_crypto, mpe_world_comm): the vec-env flags the runners read, the per-agent spaces, the state tensors, the two recycled output
sets, the forms of `actions` that `step` accepts, and `reset`, `step` and `episode_launch` — the separated runner's one-launch
episode, which the env variable `episode_flag` = "0" switches off.

A scenario's class DESCRIBES itself and this class does the rest: `scenario`, `M`, `L`, `obs_dims`, `act_dims`, `episode_flag`;
`state`, its state tensors as (name, dtype, per-env shape, fill value) in the order its entry points take them — each becomes an
attribute of that name, [N, *shape]; `env_ops`, the names of its reset, step and episode functions in mappo_amd.ops; and
`shape_args` / `episode_shape_args`, the attributes those functions take after the seed (reset, step) or after `centralized`
(episode).  What is left in a scenario's module is its own: the shapes its constructor refuses, the `set_state` test hook, and an
override where its entry points have another form (the speaker-listener's split action pointers, world_comm's MultiDiscrete leader
and opt-in episode)."""
import torch

from .. import ops
from ..utils.util import Discrete

F64, I32, I64 = torch.float64, torch.int32, torch.int64


class RaggedMPEVecEnv:
    graph_safe = True               # step() is one kernel launch on the current stream, no host-side data dependence
    accepts_device_actions = True
    accepts_index_actions = True    # step(actions [N, M] fp32 indices) is accepted besides the one-hots
    consumes_actions = True
    ragged_obs = True               # the agents' observations differ in width: reset / step return a per-agent list
    shape_args, episode_shape_args = ("M",), ()

    def __init__(self, n_rollout_threads, episode_length, seed, device):
        self.N, self.T = int(n_rollout_threads), int(episode_length)
        self.device = torch.device(device)
        self.seed = int(seed)
        self._tensors = tuple(torch.full((self.N, *shape), fill, dtype=dtype, device=self.device) for _, dtype, shape, fill in self.state)
        for (name, *_), t in zip(self.state, self._tensors):
            setattr(self, name, t)
        self._shape = tuple(getattr(self, a) for a in self.shape_args)
        self._episode_shape = tuple(getattr(self, a) for a in self.episode_shape_args)
        self.observation_space = [[d] for d in self.obs_dims]
        self.share_observation_space = [[sum(self.obs_dims)] for _ in range(self.M)]
        self.action_space = [Discrete(n) for n in self.act_dims]
        # two output sets (M observations, rewards, dones): a consumer may still read the previous env output while this step
        # writes the next one
        self._out = [tuple(torch.empty(self.N, d, device=self.device) for d in self.obs_dims) +
                     (torch.empty(self.N, self.M, 1, device=self.device), torch.empty(self.N, self.M, dtype=torch.bool, device=self.device))
                     for _ in range(2)]
        self._k = 0
        self._one_width = len(set(self.act_dims)) == 1              # then one tensor of one-hots [N, M, A] is a form of `actions`

    def _next_out(self):
        out = self._out[self._k]
        self._k ^= 1
        return out

    def state_tensors(self):
        return dict(zip((s[0] for s in self.state), self._tensors))

    def episode_state(self):
        """The capability behind the separated runner's one-launch episode on THIS env (its mappo_rollout_episode_* steps the
        environments inside the rollout kernel): the state tensors, which that launch reads and stores back, and what it needs to
        step them."""
        return dict(scenario=self.scenario, N=self.N, M=self.M, L=self.L, T=self.T, seed=self.seed, **self.state_tensors())

    # the ops are looked up by name at the call, as `ops.f(...)` would be: tests count the launches by replacing ops' attribute
    def episode_launch(self, agents, T, deterministic, counter, centralized):
        getattr(ops, self.env_ops[2])(agents, T, self.N, self.T, self.seed, *self._tensors, deterministic, counter, centralized,
                                      *self._episode_shape)

    def reset(self):
        obs = self._next_out()[:self.M]
        getattr(ops, self.env_ops[0])(*self._tensors, *self._obs_args(obs), self.N, self.seed, *self._shape)
        return list(obs)

    def step(self, actions):
        mode, act = self._parse_actions(actions)
        *obs, rew, dones = self._next_out()
        getattr(ops, self.env_ops[1])(*self._tensors, act, mode, *self._obs_args(obs), rew.view(self.N, self.M), dones.view(torch.uint8),
                                      self.N, self.T, self.seed, *self._shape)
        return obs, rew, dones, None

    def _obs_args(self, obs):
        """The M output tensors as the env's reset and step functions take them: one argument each."""
        return obs

    def _bad_actions(self, what):
        hot = " / ".join(f"[N, {n}]" for n in dict.fromkeys(self.act_dims))
        one = (f"one tensor of one-hots [N, {self.M}, {self.act_dims[0]}] or indices [N, {self.M}]" if self._one_width else
               f"one index tensor [N, {self.M}]")
        return ValueError(f"{type(self).__name__}.step: {what}: expected a list of {self.M} per-agent tensors, each one-hot {hot} or "
                          f"indices [N] / [N, 1], or {one}, with N = {self.N}")

    def _parse_actions(self, actions):
        """-> (mode, packed).  mode 0, one-hots: [N, M, A], or the list of per-agent [N, A_m] where the widths differ; mode 1: indices
        [N, M].  Accepted: a list of M per-agent tensors, each the reference's one-hot [N, A_m] or indices [N] / [N, 1]; or one tensor,
        indices [N, M] / [N, M, 1] or (one action width only) one-hots [N, M, A]."""
        N, M = self.N, self.M
        f32 = lambda a: (a if torch.is_tensor(a) else torch.as_tensor(a)).to(self.device, torch.float32)
        if isinstance(actions, (list, tuple)):
            if len(actions) != M:
                raise self._bad_actions(f"{len(actions)} per-agent entries")
            a = [f32(x) for x in actions]
            if all(tuple(x.shape) == (N, n) for x, n in zip(a, self.act_dims)):
                return 0, torch.stack(a, dim=1) if self._one_width else [x.contiguous() for x in a]
            if all(tuple(x.shape) in ((N,), (N, 1)) for x in a):
                return 1, torch.stack([x.reshape(N) for x in a], dim=1)
            raise self._bad_actions(f"per-agent actions of shapes {[tuple(x.shape) for x in a]}")
        a = f32(actions)
        if self._one_width and tuple(a.shape) == (N, M, self.act_dims[0]):
            return 0, a.contiguous()
        if tuple(a.shape) in ((N, M), (N, M, 1)):
            return 1, a.reshape(N, M).contiguous()
        raise self._bad_actions(f"actions of shape {tuple(a.shape)}")

    def close(self):
        pass
