"""MPERunner for share_policy=False — API of `onpolicy/runner/separated/mpe_runner.py:13-268`: every agent has its own policy,
trainer and SeparatedReplayBuffer; an iteration is T x (collect, env.step, insert), compute, train, all per agent.

Data stay in HBM: `collect` runs each agent's actor + critic kernels on its buffer slot (outputs land in the slot,
R_MAPPOPolicy.collect_into), `insert` stores the agent's column of the env output.  The share_obs of an agent under
use_centralized_V is the concatenation of all agents' observations of the thread (separated/mpe_runner.py:84-96,160-166).

Agents may differ in shape (MPE simple_speaker_listener: observations of 3 and 11 features, Discrete(3) and Discrete(5)): the env's
observations are then a list of per-agent tensors (mappo_amd.envs.mpe_speaker_listener) or the reference's host form, an object
array [N, M] of per-agent arrays; one-hot widths come from each agent's own action space.  On such an env feed-forward policies
collect through mappo_rollout_step (one launch per agent for actor + critic), and on a GPU-resident env of mappo_amd.envs.mpe_ragged
(speaker_listener, adversary, tag, push, crypto) the whole episode — every agent's networks, the env steps and the inserts — is
ONE launch with the same buffer contents and env state, bit for bit.  No scenario is named below: the env brings `episode_launch`,
and `episode_flag`, the env variable that, set to 0, keeps the stepwise path (A/B runs, tests).

One agent may be MultiDiscrete among Discrete ones where the env declares `accepts_multidiscrete_agents` (the GPU-resident
simple_world_comm: its leader moves and speaks): that agent's buffer carries [T, N, K] actions and log-probs, `collect` keeps all K
columns, `pack_actions` builds what the env takes, and every agent collects through collect_into — mappo_rollout_step does not
cover such a run.  Its one-launch episode (mappo_rollout_episode_world_comm) is OPT-IN, MAPPO_WORLD_COMM_EPISODE=1 (the env's
`episode_default` is "0"): the launch samples through tile16r_step, collect_into through mlp_forward_kernel, and the two do not
round alike, so the default stays what it was.  That launch runs the six actors and the environments only (the env declares
`episode_critics_after`): each critic then runs ONCE on the agent's share_obs viewed as [(T + 1) N, S] — the wide kernels at the
centralized S = 192 — straight into value_preds, slot T being the bootstrap value, and the GAE scan follows: 1 + 6 + 6 launches
where the stepwise path has about 490.  Recurrent policies, layer_N = 2 or the flag unset keep the stepwise path."""
import os
import time

import numpy as np
import torch

from mappo_amd.utils.util import head_dims_of

from .base_runner import Runner, _t2n, env_takes_device_actions


def pack_actions(acts, action_spaces, index_form):
    """The agents' sampled indices -> what `envs.step` takes, where some agent is MultiDiscrete.  acts: per-agent integer tensors (any
    device), [N] / [N, 1] for a Discrete agent and [N, K] for a MultiDiscrete one.  index_form: ONE fp32 tensor [N, sum K_m], the
    agents' columns side by side in agent order (simple_world_comm: leader move, leader word, agents 1..5) — for a device env with
    accepts_index_actions.  Otherwise the reference's per-agent list (separated/mpe_runner.py:118-124): np.eye(n)[a] for Discrete(n),
    np.eye(high_i + 1)[action[:, i]] of a MultiDiscrete agent's heads side by side."""
    N = acts[0].shape[0]
    cols = [a.reshape(N, -1).long() for a in acts]
    if index_form:
        return torch.cat(cols, dim=1).to(torch.float32)
    out = []
    for a, space in zip(cols, action_spaces):
        dims = head_dims_of(space)
        if a.shape[1] != len(dims):
            raise ValueError(f"pack_actions: {a.shape[1]} action columns for {space}")
        out.append(torch.cat([torch.eye(d, dtype=torch.float32, device=a.device)[a[:, j]] for j, d in enumerate(dims)], dim=1))
    return out


class MPERunner(Runner):
    def __init__(self, config):
        super().__init__(config)
        self._eye = None
        # a MultiDiscrete agent among the others (base_runner._build let it through: the env declares accepts_multidiscrete_agents):
        # K action / log-prob columns for that agent, so per-agent lists where the homogeneous path stacks
        self._multi = any(s.__class__.__name__ == "MultiDiscrete" for s in self.envs.action_space[:self.num_agents])
        obs_dims = [self.buffer[m].obs.shape[-1] for m in range(self.num_agents)]
        act_dims = [self.envs.action_space[m].n for m in range(self.num_agents)]
        # agents of different shapes: per-agent observation lists, per-agent one-hot widths
        self._ragged = bool(getattr(self.envs, "ragged_obs", False)) or len(set(obs_dims)) > 1 or len(set(act_dims)) > 1
        self._eyes = {}
        self._next_values = None

    def run(self):
        self.warmup()
        start = time.time()
        episodes = int(self.num_env_steps) // self.episode_length // self.n_rollout_threads
        for episode in range(episodes):
            train_infos, _ = self.run_episode(episode, episodes)
            total_num_steps = (episode + 1) * self.episode_length * self.n_rollout_threads
            if episode % self.save_interval == 0 or episode == episodes - 1:
                if self.save_dir is not None:
                    self.save()
            if episode % self.log_interval == 0:
                end = time.time()
                print("\\n Scenario {} Algo {} Exp {} updates {}/{} episodes, total num timesteps {}/{}, FPS {}.\\n".format(
                    getattr(self.all_args, "scenario_name", "synthetic"), self.algorithm_name, self.experiment_name, episode, episodes,
                    total_num_steps, self.num_env_steps, int(total_num_steps / (end - start))))
                for agent_id in range(self.num_agents):
                    train_infos[agent_id]["average_episode_rewards"] = float(self.buffer[agent_id].rewards.mean().item()) * self.episode_length
                self.log_train(train_infos, total_num_steps)
            if episode % self.eval_interval == 0 and self.use_eval:
                self.eval(total_num_steps)

    def run_episode(self, episode=0, episodes=1):
        if self.use_linear_lr_decay:
            for agent_id in range(self.num_agents):
                self.trainer[agent_id].policy.lr_decay(episode, episodes)
        infos = self.rollout()
        return self.train(), infos

    def rollout(self, deterministic=False):
        """T x (collect, env.step, insert) + compute() — as one launch where the env and the policies allow it."""
        infos = None
        if self._ragged:
            # a fresh sampling stream per episode, as the shared runner's rollout: step t of this episode draws with counter
            # t + *_counter_dev, every agent from its own word
            for p in self.policy:
                p.actor._counter_dev.add_(self.episode_length)
        if self._episode_ready():
            self._collect_episode(deterministic)
            return infos
        for step in range(self.episode_length):
            values, actions, action_log_probs, rnn_states, rnn_states_critic, actions_env = self.collect(step, deterministic)
            obs, rewards, dones, infos = self.envs.step(actions_env)
            self.insert((obs, rewards, dones, infos, values, actions, action_log_probs, rnn_states, rnn_states_critic))
        self.compute()
        return infos

    def _dev(self, x, dtype=torch.float32):
        if torch.is_tensor(x):
            return x.to(self.device) if x.dtype == torch.bool and dtype == torch.bool else x.to(self.device, dtype)
        return torch.as_tensor(np.asarray(x), dtype=dtype).to(self.device)

    def _share(self, obs_t):
        N = obs_t.shape[0]
        return obs_t.reshape(N, -1)                                 # all agents' obs of a thread, side by side

    def _obs_agents(self, obs):
        """Env observations -> (per-agent device tensors [N, D_m], share [N, sum D_m]).  Accepted forms: a tensor / array [N, M, D];
        a list of M per-agent tensors; the reference's host form for agents of different shapes, an object array [N, M] of
        per-agent arrays (separated/mpe_runner.py:160-166: np.array(list(obs[:, agent_id])), share = chain(*o) per thread)."""
        if isinstance(obs, (list, tuple)):
            per = [self._dev(o) for o in obs]
        elif isinstance(obs, np.ndarray) and obs.dtype == object:
            per = [self._dev(np.array(list(obs[:, agent_id]), dtype=np.float32)) for agent_id in range(self.num_agents)]
        else:
            obs = self._dev(obs)
            return [obs[:, agent_id] for agent_id in range(self.num_agents)], self._share(obs)
        if len(per) != self.num_agents:
            raise ValueError(f"the env returned observations of {len(per)} agents, the runner has {self.num_agents}")
        return per, torch.cat(per, dim=1)

    def _fused_ff(self):
        """Agents of different shapes with feed-forward policies the one-launch step covers: collect and the bootstrap value go
        through mappo_rollout_step (the arithmetic the one-launch episode reproduces bit for bit).  Homogeneous runs keep
        collect_into."""
        return self._ragged and all(p.can_fuse_step() and max(p.actor.desc.in_dim, p.critic.desc.in_dim) <= 64 and not p.actor.head_dims
                                    for p in self.policy)

    def _actions_env(self, envs, acts):
        """acts: per-agent index tensors [N] -> what envs.step takes.  Same shapes: np.eye(n)[action], [N, M, n], as ever.  Different
        shapes: indices [N, M] for an env that decodes them itself (accepts_index_actions), else a per-agent list of one-hots
        [N, n_m] — NumPy arrays for a host env.  With a MultiDiscrete agent acts are [N, K_m] and pack_actions builds either form."""
        if self._multi:
            device = env_takes_device_actions(envs)
            out = pack_actions(acts, envs.action_space, bool(getattr(envs, "accepts_index_actions", False)) and device)
            return out if device else [_t2n(x) for x in out]
        if not self._ragged:
            n_act = envs.action_space[0].n
            if self._eye is None or self._eye.shape[0] != n_act:
                self._eye = torch.eye(n_act, device=self.device)
            actions_env = self._eye[torch.stack(acts, dim=1)]                     # np.eye(n)[action] per agent, [N, M, n]
            return actions_env if env_takes_device_actions(envs) else _t2n(actions_env)
        if getattr(envs, "accepts_index_actions", False) and env_takes_device_actions(envs):
            return torch.stack(acts, dim=1).to(torch.float32)
        out = []
        for agent_id, a in enumerate(acts):
            n_act = envs.action_space[agent_id].n
            if n_act not in self._eyes:
                self._eyes[n_act] = torch.eye(n_act, device=self.device)
            out.append(self._eyes[n_act][a])
        return out if env_takes_device_actions(envs) else [_t2n(x) for x in out]

    # separated/mpe_runner.py:81-96
    def warmup(self):
        obs, share = self._obs_agents(self.envs.reset())
        for agent_id in range(self.num_agents):
            b = self.buffer[agent_id]
            b.share_obs[0].copy_(share if self.use_centralized_V else obs[agent_id])
            b.obs[0].copy_(obs[agent_id])

    # ---- one rollout episode in one launch (env.episode_launch: mappo_rollout_episode_comm / _adversary / _tag / _push / _crypto /
    # _world_comm) ----
    def _episode_ready(self):
        """The env is GPU-resident and steps inside the launch (it has episode_launch, and its env variable episode_flag — where unset,
        the env's episode_default, "1" unless it says otherwise — is not "0"),
        the policies are what its kernel is built for (feed-forward, narrow, layer_N <= 1, one layer_N and activation in all
        networks, the env's own widths) and the buffers have the device layout the launch writes.  Anything else takes the stepwise
        path."""
        env = self.envs
        if not hasattr(env, "episode_launch") or os.environ.get(env.episode_flag, getattr(env, "episode_default", "1")) == "0" or self.num_agents != env.M:
            return False
        return self._episode_shapes_ready(env, env.episode.device)

    _comm_episode_ready = _adversary_episode_ready = _tag_episode_ready = _episode_ready     # the names the per-scenario GPU tests call

    def _episode_shapes_ready(self, env, dev):
        """dev: where the env's tensors landed."""
        after = bool(getattr(env, "episode_critics_after", False))
        if after:
            # the launch runs the actors alone and the critics follow on the host (a MultiDiscrete head and a 192-wide critic are
            # not _fused_ff): feed-forward networks, the critic sharing the actor's layer_N and activation
            if not self._ragged or any(p.actor.desc.recurrent or p.critic.desc.recurrent
                                       or (p.critic.desc.layer_N, p.critic.desc.use_relu) != (p.actor.desc.layer_N, p.actor.desc.use_relu)
                                       for p in self.policy):
                return False
        elif not self._fused_ff():
            return False
        d0 = self.policy[0].actor.desc
        S = sum(env.obs_dims)
        for agent_id, p in enumerate(self.policy):
            a, c, b = p.actor.desc, p.critic.desc, self.buffer[agent_id]
            if (dev != p.flat_params.device or a.layer_N > 1 or (a.layer_N, a.use_relu) != (d0.layer_N, d0.use_relu)
                    or (a.in_dim, a.out_dim) != (env.obs_dims[agent_id], env.act_dims[agent_id])
                    or c.in_dim != (S if self.use_centralized_V else env.obs_dims[agent_id])
                    or b.n_rollout_threads != env.N or b.episode_length != self.episode_length
                    or not all(t.is_contiguous() and t.dtype == torch.float32
                               for t in (b.obs, b.share_obs, b.rewards, b.masks, b.actions, b.action_log_probs, b.value_preds))):
                return False
        return True

    @torch.no_grad()
    def _collect_episode(self, deterministic=False):
        """T x (collect, env.step, insert) + compute() as one launch + one GAE scan per agent — and, where the env's launch leaves the
        critics out (episode_critics_after), one critic forward per agent over all T + 1 slots in between."""
        N, T = self.n_rollout_threads, self.episode_length
        if self._next_values is None:
            self._next_values = [torch.empty(N, device=self.device) for _ in range(self.num_agents)]
        from mappo_amd import ops
        ags = [ops.comm_agent(p.actor.flat, p.actor.desc, p.critic.flat, p.critic.desc, p.actor._seed, p.actor._counter_dev, b.obs, b.share_obs,
                              b.rewards, b.masks, b.actions, b.action_log_probs, b.value_preds, self._next_values[agent_id])
               for agent_id, (p, b) in enumerate(zip(self.policy, self.buffer))]
        self.envs.episode_launch(ags, self.episode_length, deterministic, 0, self.use_centralized_V)
        after = bool(getattr(self.envs, "episode_critics_after", False))
        for agent_id, (tr, b) in enumerate(zip(self.trainer, self.buffer)):
            b.step = 0
            tr.prep_rollout()
            if after:                                               # get_values' forward, once: slot T is the bootstrap value
                rows = (T + 1) * N
                tr.policy.critic(b.share_obs.view(rows, -1), b.rnn_states_critic[-1], b.masks[-1], out=b.value_preds.view(rows, 1))
            b.compute_returns(b.value_preds[T].view(N) if after else self._next_values[agent_id], tr.value_normalizer)

    @torch.no_grad()
    def compute(self):
        if not self._fused_ff():
            return super().compute()
        # the bootstrap value through mappo_rollout_step's critic, as the stepwise collect below
        N = self.n_rollout_threads
        if self._next_values is None:
            self._next_values = [torch.empty(N, device=self.device) for _ in range(self.num_agents)]
        for agent_id, (tr, b) in enumerate(zip(self.trainer, self.buffer)):
            tr.prep_rollout()
            nv = tr.policy.collect_step_fused(b, self.episode_length, None, self.use_centralized_V, values_only=self._next_values[agent_id])
            b.compute_returns(nv, tr.value_normalizer)

    # separated/mpe_runner.py:98-151
    @torch.no_grad()
    def collect(self, step, deterministic=False):
        N = self.n_rollout_threads
        values, actions, logps, rnn_a, rnn_c = [], [], [], [], []
        fused = self._fused_ff()
        for agent_id in range(self.num_agents):
            tr, b = self.trainer[agent_id], self.buffer[agent_id]
            tr.prep_rollout()
            if fused:                                               # actor + critic of the agent in one launch, on buffer slot `step`
                act, ra, rc = tr.policy.collect_step_fused(b, step, None, self.use_centralized_V, deterministic=deterministic), None, None
            else:
                act, ra, rc = tr.policy.collect_into(b, step, deterministic=deterministic)       # outputs land in b.{actions, action_log_probs, value_preds}[step]
            values.append(b.value_preds[step]); actions.append(act.view(N, -1)); logps.append(b.action_log_probs[step])
            rnn_a.append(ra); rnn_c.append(rc)
        stack = lambda xs: torch.stack([x.view(N, *x.shape[1:]) if x is not None else torch.zeros(N, self.recurrent_N, self.hidden_size,
                                                                                                 device=self.device) for x in xs], dim=1)
        if self._multi:                                             # [N, K_m] per agent: all K columns of a MultiDiscrete agent, lists
            actions_env = self._actions_env(self.envs, [a.long() for a in actions])
            return torch.stack(values, dim=1), actions, logps, stack(rnn_a), stack(rnn_c), actions_env
        actions = torch.stack(actions, dim=1)                       # [N, M, 1]
        actions_env = self._actions_env(self.envs, [actions[:, agent_id, 0].long() for agent_id in range(self.num_agents)])
        return torch.stack(values, dim=1), actions, torch.stack(logps, dim=1), stack(rnn_a), stack(rnn_c), actions_env

    # separated/mpe_runner.py:153-178
    def insert(self, data):
        obs, rewards, dones, infos, values, actions, action_log_probs, rnn_states, rnn_states_critic = data
        N = self.n_rollout_threads
        (obs, share), rewards = self._obs_agents(obs), self._dev(rewards)
        dones = self._dev(dones, torch.bool).view(N, self.num_agents)
        masks = (~dones).to(torch.float32).view(N, self.num_agents, 1)
        recurrent = self.trainer[0]._use_recurrent_policy or self.trainer[0]._use_naive_recurrent
        for agent_id in range(self.num_agents):
            b = self.buffer[agent_id]
            ra = rc = None
            if recurrent:
                keep = masks[:, agent_id].view(N, 1, 1)
                ra = rnn_states[:, agent_id].reshape(N, self.recurrent_N, -1) * keep
                rc = rnn_states_critic[:, agent_id].reshape(N, self.recurrent_N, -1) * keep
            b.insert_env(share if self.use_centralized_V else obs[agent_id], obs[agent_id], rewards[:, agent_id].reshape(N, 1),
                         masks[:, agent_id], ra, rc)

    # separated/mpe_runner.py:180-236
    @torch.no_grad()
    def eval(self, total_num_steps):
        envs = self.eval_envs
        if envs is None:
            return
        obs, _ = self._obs_agents(envs.reset())
        N = obs[0].shape[0]
        rnn = [torch.zeros(N, self.recurrent_N, self.hidden_size, device=self.device) for _ in range(self.num_agents)]
        masks = torch.ones(N, self.num_agents, 1, device=self.device)
        rews = []
        for _ in range(self.episode_length):
            acts = []
            for agent_id in range(self.num_agents):
                self.trainer[agent_id].prep_rollout()
                a, rnn[agent_id] = self.trainer[agent_id].policy.act(obs[agent_id], rnn[agent_id], masks[:, agent_id], deterministic=True)
                acts.append(a.view(N, -1) if self._multi else a.view(N))
            obs, rewards, dones, _ = envs.step(self._actions_env(envs, [a.long() for a in acts]))
            obs, _ = self._obs_agents(obs)
            dones = self._dev(dones, torch.bool).view(N, self.num_agents)
            rews.append(self._dev(rewards).view(N, self.num_agents).clone())    # a device env hands out recycled output tensors
            masks = (~dones).to(torch.float32).view(N, self.num_agents, 1)
            for agent_id in range(self.num_agents):
                rnn[agent_id] = rnn[agent_id].view(N, self.recurrent_N, -1) * masks[:, agent_id].view(N, 1, 1)
        rew = torch.stack(rews)                                       # [T, N, M]
        for agent_id in range(self.num_agents):
            avg = float(rew[:, :, agent_id].sum(0).mean().item())
            print("eval average episode rewards of agent%i: " % agent_id + str(avg))
            self.log_env({f"agent{agent_id}/eval_average_episode_rewards": [avg]}, total_num_steps)
