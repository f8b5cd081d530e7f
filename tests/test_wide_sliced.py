"""in_dim 513..2048 (layer 1 in K slices, mlp_wide_sliced.h): what can be checked without a GPU.

The C ABI admits in_dim <= 2048 (MAPPO_MAX_IN_DIM) and refuses 2049 by name; R_Actor / R_Critic refuse it at construction; every
entry point that keeps a narrower limit (512 or 64) refuses a 513-wide descriptor before any launch and names that limit; and the
float64 side of the update cases of tests/test_gpu_wide_sliced.py keeps at least 90 % of its rows outside the ReLU margin."""
import ctypes as C

import numpy as np
import pytest
import torch

from mappo_amd import _lib
from oracle import mappo_oracle as O

P = C.c_void_p(4096)                          # never dereferenced: the checks come before any launch


def _desc(in_dim, out_dim=5, layer_N=1, recurrent=0):
    return _lib.NetDesc(in_dim, 64, out_dim, layer_N, 1, 1, recurrent)


def _call(name, descs, ints=16, head_dims=(2, 3)):
    """Call entry point `name` with placeholder arguments built from its ctypes signature: `descs` fill the descriptor slots in
    order (for the per-agent entry points: descs[0] / descs[1] are every agent's actor / critic), every pointer is P, every other
    integer `ints`."""
    lib = _lib.load()
    argtypes = getattr(lib, name).argtypes
    descs = list(descs)
    cfg = _lib.PpoCfg(0.2, 0.01, 1.0, 10.0, 1, 1, 1, 1, 0, 0)
    slot = _lib.SmacSlot(*([4096] * 9))
    heads = (C.c_int32 * len(head_dims))(*head_dims)
    agents = (_lib.CommAgent * 8)()                # more than any scenario has
    for ag in agents:
        ag.actor_params = ag.critic_params = 4096
        ag.actor_desc, ag.critic_desc = descs[0], descs[-1]
        for f in ("obs_buf", "share_buf", "rew_buf", "mask_buf", "actions", "logp", "values", "next_values"):
            setattr(ag, f, 4096)
    args = []
    for t in argtypes:
        if t is C.c_void_p:
            args.append(P)
        elif t == C.POINTER(_lib.NetDesc):
            args.append(C.byref(descs.pop(0)))
        elif t == C.POINTER(_lib.PpoCfg):
            args.append(C.byref(cfg))
        elif t == C.POINTER(_lib.SmacSlot):
            args.append(C.byref(slot))
        elif t == C.POINTER(_lib.CommAgent):
            args.append(agents)
        elif t == C.POINTER(C.c_int32):
            args.append(heads)
        elif args and args[-1] is heads:
            args.append(len(head_dims))           # n_heads follows head_dims
        else:
            args.append(ints)
    rc = getattr(lib, name)(*args)
    return rc, lib.mappo_last_error().decode()


def test_abi_admits_2048_and_refuses_2049():
    lib = _lib.load()
    assert lib.mappo_abi_version() >= 13
    rc, msg = _call("mappo_mlp_forward", [_desc(2049)])
    assert rc == -1 and "2048" in msg and "2049" in msg, msg
    for fn in ("mappo_actor_act", "mappo_mlp_features", "mappo_actor_update", "mappo_trunk_backward", "mappo_wide_l1_backward"):
        rc, msg = _call(fn, [_desc(2049)])
        assert rc == -1 and "2048" in msg, (fn, msg)
    assert lib.mappo_net_param_count(C.byref(_desc(2048))) == 2 * 2048 + 64 * 2048 + 64 + 128 + (64 * 64 + 64 + 128) + 5 * 64 + 5
    # the workspace and slab counts do not depend on the width; the blocked layout now serves every width of the 16-sample-tile path
    assert lib.mappo_wide_layout(C.byref(_desc(2048)), 1) == lib.mappo_wide_layout(C.byref(_desc(512)), 1)
    assert lib.mappo_wide_layout(C.byref(_desc(600, 1, 1, 1)), 3) == lib.mappo_wide_layout(C.byref(_desc(300, 1, 1, 1)), 3)


def test_networks_refuse_2049_at_construction():
    from mappo_amd.algorithms.r_mappo.algorithm.r_actor_critic import R_Actor, R_Critic
    from mappo_amd.utils.util import Discrete
    a = O.default_args()
    with pytest.raises(NotImplementedError, match="2048"):
        R_Actor(a, [2049], Discrete(5), device="cpu")
    with pytest.raises(NotImplementedError, match="2048"):
        R_Critic(a, [2049], device="cpu")


OUT_OF_SCOPE = [  # entry point, descriptors, words its message must contain
    ("mappo_actor_critic_update", [_desc(513), _desc(513, 1)], ["actor_critic_update", "64"]),
    ("mappo_rollout_episode", [_desc(513), _desc(513, 1)], ["rollout_episode", "64"]),
    ("mappo_mlp_features_seq", [_desc(513, 5, 1, 1)], ["mlp_features_seq", "512"]),
    ("mappo_trunk_backward_seq", [_desc(513, 5, 1, 1)], ["trunk_backward_seq", "512"]),
    ("mappo_recurrent_rollout_step", [_desc(513, 5, 1, 1), _desc(513, 1, 1, 1)], ["recurrent_rollout_step", "512"]),
    ("mappo_recurrent_step_dual", [_desc(513, 5, 1, 1), _desc(513, 1, 1, 1)], ["recurrent_step_dual", "512"]),
    ("mappo_actor_act_md", [_desc(513)], ["actor_act_md", "in_dim 513", "64"]),
    ("mappo_rollout_step_md", [_desc(513), _desc(513, 1)], ["rollout_step_md", "in_dim 513", "64"]),
    ("mappo_actor_update_md", [_desc(513)], ["actor_update_md", "in_dim 513", "64"]),
    ("mappo_actor_critic_update_md", [_desc(513), _desc(513, 1)], ["actor_critic_update_md", "in_dim 513", "64"]),
    # the one-launch episodes on the device envs: the scenario fixes the width, and the message names it
    ("mappo_rollout_episode_spread", [_desc(513), _desc(513, 1)], ["rollout_episode_spread", "in_dim 513", "64"]),
    ("mappo_rollout_episode_reference", [_desc(513, 15), _desc(513, 1)], ["rollout_episode_reference", "in_dim 513", "64"]),
    ("mappo_rollout_episode_comm", [_desc(513), _desc(513, 1)], ["rollout_episode_comm", "in_dim 513", "the scenario has in_dim 3 "]),
    ("mappo_rollout_episode_adversary", [_desc(513), _desc(513, 1)], ["rollout_episode_adversary", "in_dim 513", "the scenario has in_dim 8 "]),
    ("mappo_rollout_episode_tag", [_desc(513), _desc(513, 1)], ["rollout_episode_tag", "in_dim 513", "the scenario has in_dim 16 "]),
    ("mappo_rollout_episode_push", [_desc(513), _desc(513, 1)], ["rollout_episode_push", "in_dim 513", "the scenario has in_dim 8 "]),
    ("mappo_rollout_episode_crypto", [_desc(513), _desc(513, 1)], ["rollout_episode_crypto", "in_dim 513", "the scenario has in_dim 4 "]),
    ("mappo_rollout_episode_world_comm", [_desc(513), _desc(513, 1)], ["rollout_episode_world_comm", "in_dim 513", "the scenario has in_dim 34 "]),
    # a mixed pair (one network within the tuned kernels' 512 columns, the other beyond): refused by name, the Python layer runs
    # the networks one by one (R_MAPPOPolicy.can_fuse_step / recurrent.can_step_dual)
    ("mappo_rollout_step", [_desc(300), _desc(600, 1)], ["rollout_step", "512", "600"]),
    ("mappo_mlp_features_dual", [_desc(600, 5, 1, 1), _desc(300, 1, 1, 1)], ["mlp_features_dual", "512", "600"]),
]


@pytest.mark.parametrize("fn,descs,words", OUT_OF_SCOPE, ids=[c[0] for c in OUT_OF_SCOPE])
def test_out_of_scope_entry_points_name_their_limit(fn, descs, words):
    # integer arguments: 16 everywhere, except where an env refuses such agent / landmark counts before it looks at the networks
    kw = dict(ints=3) if fn == "mappo_rollout_episode_crypto" else {}
    if fn == "mappo_rollout_episode_reference":
        kw = dict(head_dims=(5, 10))
    rc, msg = _call(fn, descs, **kw)
    assert rc == -1, (fn, rc, msg)
    for w in words:
        assert w in msg, (fn, msg)


def test_policy_takes_the_separate_launch_path():
    """513..2048 columns on either network: no fused step, no dual update, no dual recurrent step — and no exception.  (The
    policy itself needs a GPU; its path selection only reads the two descriptors.)"""
    from types import SimpleNamespace as NS
    from mappo_amd.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    from mappo_amd import recurrent
    for rec in (0, 1):
        for D, S in ((40, 600), (300, 600), (600, 1200), (2048, 2048)):
            actor, critic = NS(desc=_desc(D, 5, 1, rec), _recurrent_N=1), NS(desc=_desc(S, 1, 1, rec), _recurrent_N=1)
            pol = NS(actor=actor, critic=critic)
            assert not R_MAPPOPolicy.can_fuse_step(pol) and not R_MAPPOPolicy.can_dual_update(pol)
            assert not recurrent.can_step_dual(actor, critic)


# ---- the float64 side of the update cases -----------------------------------------------------------------------------
UPDATE_CASES = [(513, 17, 1), (1000, 33, 1), (2048, 48, 1),     # (D, B, layer_N); the critic's width is D as well
                (600, 33, 2)]                                   # layer_N = 2: the K-chunked update kernel (mlp_upd.h) beyond 512 columns


def update_inputs(D, B, with_rows, relu=True, LN=1):
    """Networks and loss inputs of one update case (shared with tests/test_gpu_wide_sliced.py).  Rows whose ReLU pre-activations
    or loss terms lie within 1e-4 of a kink are DEACTIVATED (active = 0) rather than redrawn: both sides then skip them."""
    from test_gpu_kernels import _randomize, _relu_margin, _loss_margin
    torch.manual_seed(D + B)
    rng = np.random.default_rng(D * 7 + B + (1 if with_rows else 0))
    a = O.default_args(use_ReLU=relu, layer_N=LN, use_feature_normalization=True)
    A = 5
    actor, critic = O.ActorRef(a, D, A), O.CriticRef(a, D)
    _randomize(actor, D + 3); _randomize(critic, D + 4)
    f = np.float32
    n_rows = B + 16 if with_rows else B
    rows = rng.permutation(n_rows)[:B].astype(np.int32) if with_rows else np.arange(B, dtype=np.int32)
    obs = rng.standard_normal((n_rows, D)).astype(f)
    sobs = rng.standard_normal((n_rows, D)).astype(f)
    avail = (rng.random((n_rows, A)) > 0.3).astype(f)
    actions = rng.integers(0, A, n_rows).astype(f)
    avail[np.arange(n_rows), actions.astype(int)] = 1.0
    old_logp = (-np.abs(rng.standard_normal(n_rows)) * 0.3 - np.log(A)).astype(f)
    adv = rng.standard_normal(n_rows).astype(f)
    active = (rng.random(n_rows) > 0.25).astype(f)
    ret = (rng.standard_normal(n_rows) * 3).astype(f)
    with torch.no_grad():
        v_now = critic(torch.from_numpy(sobs), None, None)[0].numpy().reshape(-1)
    v_old = (v_now + rng.standard_normal(n_rows) * 0.25).astype(f)
    vn = O.ValueNormRef()
    vn.update(ret[:8].reshape(-1, 1)); vn.update(ret[rows].reshape(-1, 1))
    m = _loss_margin(a, actor, critic, obs, sobs, actions, avail, active, old_logp, v_old, ret, vn)
    if relu:
        m = np.minimum(m, np.minimum(_relu_margin(actor, torch.from_numpy(obs)), _relu_margin(critic, torch.from_numpy(sobs))))
    near = m < 1e-4
    active[near] = 0.0
    return dict(a=a, actor=actor, critic=critic, rows=rows, obs=obs, sobs=sobs, avail=avail, actions=actions, old_logp=old_logp, adv=adv,
                active=active, ret=ret, v_old=v_old, vn=vn, near=near[rows], A=A, LN=LN)


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("D,B,LN", UPDATE_CASES)
def test_update_cases_keep_their_rows(D, B, LN, with_rows):
    """At most 10 % of a case's rows are deactivated for lying within the margin of a kink, and some active rows remain."""
    c = update_inputs(D, B, with_rows, LN=LN)
    assert c["near"].sum() <= 0.1 * B, (D, B, int(c["near"].sum()))
    assert c["active"][c["rows"]].sum() >= 0.5 * B
