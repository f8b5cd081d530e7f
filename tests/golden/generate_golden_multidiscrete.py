#!/usr/bin/env python3
"""Generate tests/golden/multidiscrete.npz by IMPORTING the reference's hot-path modules (build container only), with the
simple_reference action space MultiDiscrete([[0, 4], [0, 9]]) (envs/mpe/environment.py:82-86).

Run:  python tests/golden/generate_golden_multidiscrete.py            (needs the reference checkout; writes the .npz here)

Same recipe as generate_golden.py: the reference package is imported through an empty namespace module, only data (inputs and the
reference's outputs) is written.  Shapes: obs 21, share_obs 42, heads (5, 10), M = 2 agents, N = 4 threads, T = 6 steps,
layer_N = 1, ppo_epoch = 1, num_mini_batch = 1.  Two cases: c0 default flags with every row active, c1 with inactive rows
(use_policy_active_masks is on by default: their rows leave the policy loss and the entropy).  Per case:
  init/{actor,critic}/*      (c0) the state dicts right after construction under torch.manual_seed(seed) (init scheme, RNG order, keys)
  actor0, critic0, vn0       the perturbed state every run below starts from
  buf/*                      a filled buffer, returns computed by the reference's compute_returns
  sample/*, upd/*            one feed_forward_generator minibatch (the whole buffer), R_MAPPO.ppo_update on it: the gradient of every
                             parameter (unclipped: the norms stay below max_grad_norm) and its six return values
  train/*                    R_MAPPO.train on the buffer from the same start: train_info and the state dicts after it"""
import copy
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("MAPPO_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
pkg = types.ModuleType("onpolicy")
pkg.__path__ = [os.path.join(REF, "onpolicy")]
sys.modules["onpolicy"] = pkg

from onpolicy.config import get_config                                             # noqa: E402
from onpolicy.utils.shared_buffer import SharedReplayBuffer                       # noqa: E402
from onpolicy.utils.valuenorm import ValueNorm                                     # noqa: E402
from onpolicy.algorithms.r_mappo.r_mappo import R_MAPPO                            # noqa: E402
from onpolicy.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy       # noqa: E402

TUPLE = ("share_obs", "obs", "rnn_states", "rnn_states_critic", "actions", "value_preds", "returns",
         "masks", "active_masks", "old_action_log_probs", "adv_targ", "available_actions")
BUF_NAMES = ("share_obs", "obs", "rnn_states", "rnn_states_critic", "value_preds", "returns", "actions", "action_log_probs",
             "rewards", "masks", "bad_masks", "active_masks")


class MultiDiscrete:  # matched by class name in the reference (utils/util.py:43-44, act.py:27-33)
    def __init__(self, pairs):
        arr = np.array(pairs)
        self.low, self.high = arr[:, 0], arr[:, 1]
        self.num_discrete_space = self.low.shape[0]
        self.shape = self.num_discrete_space


class Box:  # the observation spaces are passed as plain lists, as in generate_golden.py; kept for envs that hand out Box
    def __init__(self, shape):
        self.shape = shape


def make_args(**kw):
    a = get_config().parse_known_args([])[0]
    a.use_recurrent_policy = False
    a.use_naive_recurrent_policy = False
    for k, v in kw.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    return a


def sd_arrays(prefix, module):
    return {f"{prefix}/{k}": v.detach().cpu().numpy().copy() for k, v in module.state_dict().items()}


def vn_state(vn):
    return np.array([vn.running_mean.item(), vn.running_mean_sq.item(), vn.debiasing_term.item()], dtype=np.float32)


def main():
    T, N, M, D, S, heads = 6, 4, 2, 21, 42, (5, 10)
    space = MultiDiscrete([[0, d - 1] for d in heads])
    out = {}
    for case, inactive in enumerate((0.0, 0.25)):
        seed = 900 + case
        torch.manual_seed(seed)
        rng = np.random.default_rng(seed)
        a = make_args(episode_length=T, n_rollout_threads=N, lr=7e-4, critic_lr=7e-4, ppo_epoch=1, num_mini_batch=1, layer_N=1)
        pol = R_MAPPOPolicy(a, [D], [S], space)
        p = f"c{case}"
        out[p + "/dims"] = np.array([T, N, M, D, S, a.hidden_size, seed] + list(heads))
        out[p + "/hyper"] = np.array([a.clip_param, a.entropy_coef, a.value_loss_coef, a.huber_delta, a.max_grad_norm, a.lr, a.critic_lr,
                                      a.opti_eps, a.weight_decay], dtype=np.float64)
        out[p + "/actor_keys"] = np.array(list(pol.actor.state_dict().keys()))
        if case == 0:
            out.update(sd_arrays(p + "/init/actor", pol.actor)); out.update(sd_arrays(p + "/init/critic", pol.critic))
        with torch.no_grad():
            for net in (pol.actor, pol.critic):
                for n_, p_ in net.named_parameters():
                    if "norm" in n_ or "bias" in n_ or ".2." in n_:
                        p_.add_(0.1 * torch.randn_like(p_))
                    if "action_outs" in n_ and "weight" in n_:
                        p_.mul_(30.0)
        out.update(sd_arrays(p + "/actor0", pol.actor)); out.update(sd_arrays(p + "/critic0", pol.critic))
        vn0 = ValueNorm(1)
        for _ in range(2):
            vn0.update(torch.from_numpy((rng.standard_normal((32, 1)) * 2 + 0.5).astype(np.float32)))
        out[p + "/vn0"] = vn_state(vn0)

        buf = SharedReplayBuffer(a, M, [D], [S], space)
        assert buf.available_actions is None and buf.actions.shape == (T, N, M, len(heads))
        f = np.float32
        for name in ("share_obs", "obs", "value_preds", "rewards"):
            arr = getattr(buf, name)
            arr[...] = rng.standard_normal(arr.shape).astype(f)
        buf.value_preds[...] *= 0.3
        buf.actions[...] = np.stack([rng.integers(0, d, (T, N, M)) for d in heads], -1).astype(f)
        buf.masks[...] = (rng.random(buf.masks.shape) > 0.15).astype(f)
        buf.bad_masks[...] = (rng.random(buf.masks.shape) > 0.15).astype(f)
        buf.active_masks[...] = (rng.random(buf.masks.shape) >= inactive).astype(f)
        # old log-probs: the policy's own, off by a little noise — ratios around 1, some of them beyond the clip range
        B = T * N * M
        z = np.zeros((B, 1, a.hidden_size), f)
        with torch.no_grad():
            lp, _ = pol.actor.evaluate_actions(buf.obs[:-1].reshape(B, D), z, buf.actions.reshape(B, -1), np.ones((B, 1), f), None,
                                               buf.active_masks[:-1].reshape(B, 1))
        assert tuple(lp.shape) == (B, len(heads))
        buf.action_log_probs[...] = (lp.numpy() + 0.15 * rng.standard_normal(lp.shape)).astype(f).reshape(buf.action_log_probs.shape)
        nv = rng.standard_normal((N, M, 1)).astype(f)
        vn_r = copy.deepcopy(vn0)
        buf.compute_returns(nv, vn_r)
        for n in BUF_NAMES:
            out[f"{p}/buf/{n}"] = getattr(buf, n).copy()

        # ---- one ppo_update on the whole buffer as one minibatch ----
        pol_u = copy.deepcopy(pol)
        pol_u.actor_optimizer = torch.optim.Adam(pol_u.actor.parameters(), lr=a.lr, eps=a.opti_eps, weight_decay=a.weight_decay)
        pol_u.critic_optimizer = torch.optim.Adam(pol_u.critic.parameters(), lr=a.critic_lr, eps=a.opti_eps, weight_decay=a.weight_decay)
        tr_u = R_MAPPO(a, pol_u)
        tr_u.value_normalizer = copy.deepcopy(vn0)
        adv = rng.standard_normal(buf.rewards.shape).astype(f)
        torch.manual_seed(2000 + seed)
        sample = next(buf.feed_forward_generator(adv, 1))
        for nm, arr in zip(TUPLE, sample):
            if arr is not None:
                out[f"{p}/sample/{nm}"] = arr
        vl, cgn, pl, ent, agn, imp = tr_u.ppo_update(sample, True)
        assert float(agn) < a.max_grad_norm and float(cgn) < a.max_grad_norm            # so .grad is the unclipped gradient
        assert tuple(imp.shape) == (B, len(heads))
        out[p + "/upd/stats"] = np.array([vl.item(), float(cgn), pl.item(), ent.item(), float(agn), imp.mean().item()], dtype=np.float64)
        out[p + "/upd/imp"] = imp.detach().numpy()
        for tag, net in (("actor", pol_u.actor), ("critic", pol_u.critic)):
            for n_, p_ in net.named_parameters():
                if p_.grad is not None:
                    out[f"{p}/upd/{tag}_grad/{n_}"] = p_.grad.numpy().copy()
        out[p + "/upd/vn"] = vn_state(tr_u.value_normalizer)

        # ---- train() from the same start ----
        tr = R_MAPPO(a, pol)
        tr.value_normalizer = copy.deepcopy(vn0)
        torch.manual_seed(3000 + seed)
        tr.prep_training()
        info = tr.train(buf)
        out[p + "/train/info_keys"] = np.array(list(info.keys()))
        out[p + "/train/info"] = np.array([float(v) for v in info.values()], dtype=np.float64)
        out.update(sd_arrays(p + "/train/actor", pol.actor)); out.update(sd_arrays(p + "/train/critic", pol.critic))
        out[p + "/train/vn"] = vn_state(tr.value_normalizer)
    out["n_cases"] = np.array(2)
    path = os.path.join(OUT, "multidiscrete.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
