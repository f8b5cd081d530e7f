"""Float64 torch reference of ONE rollout step of a recurrent network (r_actor_critic.py:43-70,146-165): MLPBase trunk (feature
norm, fc1, fc2.., each Linear -> activation -> LayerNorm; mlp.py:18-55), the single-step GRU on `h * mask` (rnn.py:25-29), rnn.norm,
and the output layer.  Shared by the tests of the recurrent rollout paths; reads the weights out of the flat parameter vector."""
import torch
import torch.nn.functional as F


def weights64(net, head_prefix):
    """{state_dict key: float64 CPU tensor} of a FlatActor / FlatCritic (`net.flat`, `net.desc`)."""
    from mappo_amd.flat import net_layout, unpack_to_dict
    layout, _ = net_layout(net.desc, head_prefix)
    return {k: v.detach().double().cpu() for k, v in unpack_to_dict(net.flat, layout).items()}


def step64(w, desc, head_prefix, x, h, mask):
    """x [R, D], h [R, 64], mask [R, 1] (float64) -> (next state [R, 64], head output [R, A])."""
    H = desc.hidden
    act = torch.relu if desc.use_relu else torch.tanh
    if desc.use_feature_norm:
        x = F.layer_norm(x, (x.shape[-1],), w["base.feature_norm.weight"], w["base.feature_norm.bias"])
    x = F.layer_norm(act(F.linear(x, w["base.mlp.fc1.0.weight"], w["base.mlp.fc1.0.bias"])), (H,), w["base.mlp.fc1.2.weight"],
                     w["base.mlp.fc1.2.bias"])
    for l in range(desc.layer_N):
        x = F.layer_norm(act(F.linear(x, w[f"base.mlp.fc2.{l}.0.weight"], w[f"base.mlp.fc2.{l}.0.bias"])), (H,),
                         w[f"base.mlp.fc2.{l}.2.weight"], w[f"base.mlp.fc2.{l}.2.bias"])
    hm = h * mask
    gi = F.linear(x, w["rnn.rnn.weight_ih_l0"], w["rnn.rnn.bias_ih_l0"])
    gh = F.linear(hm, w["rnn.rnn.weight_hh_l0"], w["rnn.rnn.bias_hh_l0"])
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    h_new = (1.0 - z) * n + z * hm
    y = F.layer_norm(h_new, (H,), w["rnn.norm.weight"], w["rnn.norm.bias"])
    return h_new, F.linear(y, w[head_prefix + ".weight"], w[head_prefix + ".bias"])
