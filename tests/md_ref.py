"""Test-side reference of the MultiDiscrete semantics (act.py:27-33,65-76,139-152 and r_mappo.py:124-141 of the reference), in
float64 torch: K Categorical heads over consecutive slices of the actor's logits, per-head log-probs and ratios, the clipped terms
summed over the heads, the entropy averaged over them.  A plain helper module: no fixtures, no pytest settings."""
import torch


def head_slices(head_dims):
    out, lo = [], 0
    for d in head_dims:
        out.append((lo, lo + int(d)))
        lo += int(d)
    return out


def evaluate_heads(logits, head_dims, actions):
    """logits [B, A], actions [B, K] -> (log-probs [B, K], entropies [B, K])."""
    lps, ents = [], []
    for j, (lo, hi) in enumerate(head_slices(head_dims)):
        lpa = torch.log_softmax(logits[:, lo:hi], dim=-1)
        lps.append(lpa.gather(1, actions[:, j:j + 1].long()))
        ents.append(-(lpa.exp() * lpa).sum(-1, keepdim=True))
    return torch.cat(lps, 1), torch.cat(ents, 1)


def policy_terms(logits, head_dims, actions, old_logp, adv, active, clip_param, use_policy_active_masks):
    """(policy_loss, entropy, ratio mean, ratios [B, K]) as the issue's table states them; adv / active are [B, 1]."""
    lp, H = evaluate_heads(logits, head_dims, actions)
    r = torch.exp(lp - old_logp)
    s = torch.min(r * adv, torch.clamp(r, 1.0 - clip_param, 1.0 + clip_param) * adv).sum(-1, keepdim=True)
    if use_policy_active_masks:
        den = active.sum()
        pl = -(s * active).sum() / den
        ent = ((H * active).sum(0) / den).mean()
    else:
        pl = -s.mean()
        ent = H.mean(0).mean()
    return pl, ent, r.mean(), r


def oracle_nets(O, args, sd_actor, sd_critic, D, S, head_dims):
    """The reference's MultiDiscrete actor / critic state dicts loaded into the oracle's networks: the heads' weight rows and biases
    side by side are ONE linear layer of sum d_j rows (act.action_outs.{j}.linear -> act.action_out.linear)."""
    K = len(head_dims)
    sd = {k: torch.as_tensor(v) for k, v in sd_actor.items()}
    sd["act.action_out.linear.weight"] = torch.cat([sd.pop(f"act.action_outs.{j}.linear.weight") for j in range(K)], 0)
    sd["act.action_out.linear.bias"] = torch.cat([sd.pop(f"act.action_outs.{j}.linear.bias") for j in range(K)], 0)
    actor, critic = O.ActorRef(args, D, int(sum(head_dims))), O.CriticRef(args, S)
    actor.load_state_dict(sd)
    critic.load_state_dict({k: torch.as_tensor(v) for k, v in sd_critic.items()})
    return actor, critic


def split_head_grads(grads, head_dims):
    """Gradients keyed like the oracle actor -> keyed like the reference's (per-head rows of the one head matrix)."""
    out = {k: v for k, v in grads.items() if not k.startswith("act.action_out.")}
    for j, (lo, hi) in enumerate(head_slices(head_dims)):
        out[f"act.action_outs.{j}.linear.weight"] = grads["act.action_out.linear.weight"][lo:hi]
        out[f"act.action_outs.{j}.linear.bias"] = grads["act.action_out.linear.bias"][lo:hi]
    return out
