"""Runner for share_policy=False — API of `onpolicy/runner/separated/base_runner.py:14-160`: one R_MAPPOPolicy, R_MAPPO trainer
and SeparatedReplayBuffer PER AGENT (lists indexed by agent id), all on the HIP kernels of the shared path.  Every agent's
networks live in their own flat parameter buffer; `compute` / `train` run the agents one after the other (the same
launches as the shared runner with M = 1).  The ROLLOUT of agents with feed-forward policies on the GPU-resident
MPE envs is batched into one launch (separated/mpe_runner.py, mappo_rollout_episode_*).

With MAPPO_SEPARATED_GROUP_TRAIN=1 `train` batches the agents' PPO updates as well: per epoch one update launch
(mappo_actor_critic_update_group) and one optimiser call (mappo_reduce_clip_adam_group, two launches) for up to 8 agents,
between per-agent prologues and epilogues, the whole sequence in one hipGraph — bit for bit what the sequential path
computes.  It applies when EVERY agent's trainer qualifies (R_MAPPO.phase_ready: fused dual update on the 16-sample-tile
kernel — both networks feed-forward with at most 64 inputs, Discrete head of at most 16 actions, layer_N <= 1 — whole-buffer
minibatch, single process); otherwise, and without the flag, all agents train sequentially as before (simple_world_comm with
its 192-wide critics and MultiDiscrete leader, rmappo, num_mini_batch > 1).  Measurements: DESIGN.md §5."""
import os

import torch

from mappo_amd.runner.shared.base_runner import Runner as _SharedRunner, _t2n, env_takes_device_actions  # noqa: F401
from mappo_amd.utils.separated_buffer import SeparatedReplayBuffer


class Runner(_SharedRunner):
    def __init__(self, config):
        self._separated_config = config
        super().__init__(config)

    def _build(self, config):
        """Called by the shared Runner's constructor in place of the single policy / trainer / buffer."""
        from mappo_amd.algorithms.r_mappo.r_mappo import R_MAPPO as TrainAlgo
        from mappo_amd.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy as Policy
        self.policy, self.trainer, self.buffer = [], [], []
        # a MultiDiscrete agent among the others: only on an env that declares it takes such an agent's K index columns / K one-hots
        # side by side (accepts_multidiscrete_agents, e.g. SimpleWorldCommVecEnv); its buffer then carries [T, N, K] actions
        multi_ok = bool(getattr(self.envs, "accepts_multidiscrete_agents", False))
        for agent_id in range(self.num_agents):
            if self.envs.action_space[agent_id].__class__.__name__ == "MultiDiscrete" and not multi_ok:
                raise NotImplementedError("MultiDiscrete action space under the separated runner (share_policy = False): the K-wide action "
                                          "columns are built for the shared MPERunner only")
        for agent_id in range(self.num_agents):
            share_space = self.envs.share_observation_space[agent_id] if self.use_centralized_V else self.envs.observation_space[agent_id]
            self.policy.append(Policy(self.all_args, self.envs.observation_space[agent_id], share_space, self.envs.action_space[agent_id],
                                      device=self.device))
            # every agent samples from its own Philox stream (same args.seed, same step counter and row index otherwise)
            self.policy[-1].actor._seed = (self.policy[-1].actor._seed + agent_id * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        if self.model_dir is not None:
            self.restore()
        for agent_id in range(self.num_agents):
            share_space = self.envs.share_observation_space[agent_id] if self.use_centralized_V else self.envs.observation_space[agent_id]
            self.trainer.append(TrainAlgo(self.all_args, self.policy[agent_id], device=self.device, dist_group=config.get("dist_group")))
            self.buffer.append(SeparatedReplayBuffer(self.all_args, self.envs.observation_space[agent_id], share_space,
                                                     self.envs.action_space[agent_id], device=self.device))

    # separated/base_runner.py:110-118
    @torch.no_grad()
    def compute(self):
        for agent_id in range(self.num_agents):
            tr, b = self.trainer[agent_id], self.buffer[agent_id]
            tr.prep_rollout()
            next_value = tr.policy.get_values(b.share_obs[-1], b.rnn_states_critic[-1], b.masks[-1])
            b.compute_returns(next_value, tr.value_normalizer)

    # separated/base_runner.py:120-129
    def train(self):
        if self._group_train_ready():
            return self._train_grouped()
        train_infos = []
        for agent_id in range(self.num_agents):
            self.trainer[agent_id].prep_training()
            train_infos.append(self.trainer[agent_id].train(self.buffer[agent_id]))
            self.buffer[agent_id].after_update()
        return train_infos

    # ---- MAPPO_SEPARATED_GROUP_TRAIN=1: the agents' PPO updates side by side -------------------------------------------------
    GROUP_FLAG = "MAPPO_SEPARATED_GROUP_TRAIN"
    GROUP_MAX = 8                      # agents per grouped launch (MAPPO_MAX_GROUP); more agents split into groups of at most this many
    _group_graphs = None
    _group_warned = False

    def _group_train_ready(self):
        """Opt-in, and all or nothing: one agent whose trainer does not qualify (R_MAPPO.phase_ready: recurrent, wide critic,
        MultiDiscrete, num_mini_batch > 1, ...) or that disagrees with the others in (layer_N, activation, feature normalisation)
        keeps the whole run on the sequential path above, with one warning."""
        if os.environ.get(self.GROUP_FLAG, "0") == "0":
            return False
        d0 = self.policy[0].actor.desc
        same = lambda d: (d.layer_N, d.use_relu, d.use_feature_norm) == (d0.layer_N, d0.use_relu, d0.use_feature_norm)
        bad = [m for m, tr in enumerate(self.trainer) if not (tr.phase_ready() and same(tr.policy.actor.desc))]
        if bad and not self._group_warned:
            import warnings
            warnings.warn(f"{self.GROUP_FLAG}: agent(s) {bad} do not qualify for the grouped PPO update; every agent trains sequentially")
            self._group_warned = True
        return not bad

    def _train_grouped(self):
        """Per-agent prologues, per epoch ONE update launch and ONE optimiser call (two launches) per group of at most 8 agents,
        per-agent epilogues with after_update's copies inside: the launches a sequential train() makes per agent, bit for bit,
        2 A + 3 E ceil(A / 8) + A of them instead of A (3 + 3 E) + A.  Captured into one hipGraph after a warm eager pass, like
        R_MAPPO.train."""
        from mappo_amd import ops
        trs, bufs = self.trainer, self.buffer
        G = min(int(self.GROUP_MAX), ops._lib.MAX_GROUP)
        groups = [range(i, min(i + G, len(trs))) for i in range(0, len(trs), G)]

        def body():
            for tr, b in zip(trs, bufs):
                tr.phase_prologue(b)
            for epoch in range(trs[0].ppo_epoch):
                for g in groups:
                    ops.actor_critic_update_group([trs[m].phase_update_job(epoch) for m in g])
                    ops.reduce_clip_adam_group([trs[m].phase_optim_job() for m in g])
            for tr, b in zip(trs, bufs):
                tr.phase_epilogue(b, after_update=True)

        for tr in trs:
            tr.prep_training()
            tr.phase_sync()
        if not all(tr._use_graph for tr in trs):
            body()
        else:
            if self._group_graphs is None:
                self._group_graphs = {}
            key = tuple(id(b) for b in bufs)                  # (the runner holds its buffers: the ids cannot be reused)
            state = self._group_graphs.get(key)
            if state is None:
                body()                                        # eager: allocates workspaces
                self._group_graphs[key] = "warm"
            else:
                if state == "warm":
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        body()
                    self._group_graphs[key] = state = g
                state.replay()
        return [tr.phase_info() for tr in trs]

    # separated/base_runner.py:131-146: actor_agent{i}.pt / critic_agent{i}.pt (+ vnorm_agent{i}.pt as the shared runner adds)
    def save(self):
        for agent_id in range(self.num_agents):
            pol, tr = self.policy[agent_id], self.trainer[agent_id]
            torch.save(pol.actor.state_dict(), os.path.join(self.save_dir, f"actor_agent{agent_id}.pt"))
            torch.save(pol.critic.state_dict(), os.path.join(self.save_dir, f"critic_agent{agent_id}.pt"))
            if tr.value_normalizer is not None:
                torch.save(tr.value_normalizer.state_dict(), os.path.join(self.save_dir, f"vnorm_agent{agent_id}.pt"))

    def restore(self):
        for agent_id in range(self.num_agents):
            pol = self.policy[agent_id]
            pol.actor.load_state_dict(torch.load(os.path.join(str(self.model_dir), f"actor_agent{agent_id}.pt"), weights_only=True))
            pol.critic.load_state_dict(torch.load(os.path.join(str(self.model_dir), f"critic_agent{agent_id}.pt"), weights_only=True))

    def restore_value_normalizers(self):
        for agent_id in range(self.num_agents):
            path = os.path.join(str(self.model_dir), f"vnorm_agent{agent_id}.pt")
            if self.trainer[agent_id].value_normalizer is not None and os.path.exists(path):
                self.trainer[agent_id].value_normalizer.load_state_dict(torch.load(path, weights_only=True))

    def log_train(self, train_infos, total_num_steps):
        for agent_id, info in enumerate(train_infos):
            super().log_train({f"agent{agent_id}/{k}": v for k, v in info.items()}, total_num_steps)
