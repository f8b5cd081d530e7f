"""MultiDiscrete action spaces, the part that needs no GPU: the space helpers, the K-wide buffer arrays, the synthetic env's
action_dims, the one-hot the runner hands the env, and the argument checks of the mappo_*_md entry points — every limit is
refused on the host, before anything touches a device, with a message that names it."""
import ctypes as C

import numpy as np
import pytest
import torch

from mappo_amd import _lib
from mappo_amd.utils.util import Discrete, MultiDiscrete, get_shape_from_act_space, head_dims_of


def test_space_helpers():
    sp = MultiDiscrete([[0, 4], [0, 9]])
    assert sp.__class__.__name__ == "MultiDiscrete" and sp.shape == 2
    assert list(sp.low) == [0, 0] and list(sp.high) == [4, 9]
    assert get_shape_from_act_space(sp) == 2 and head_dims_of(sp) == (5, 10)
    assert head_dims_of(MultiDiscrete([[1, 3], [2, 2], [0, 6]])) == (3, 1, 7)
    assert get_shape_from_act_space(Discrete(5)) == 1 and head_dims_of(Discrete(5)) == (5,)
    with pytest.raises(ValueError):
        MultiDiscrete([[3, 1]])

    class Box:
        pass
    with pytest.raises(NotImplementedError):
        get_shape_from_act_space(Box())


def _args():
    from oracle import mappo_oracle as O
    return O.default_args(episode_length=6, n_rollout_threads=4)


@pytest.mark.parametrize("cls", ["shared", "separated"])
def test_buffer_shapes(cls):
    sp = MultiDiscrete([[0, 4], [0, 9]])
    a = _args()
    if cls == "shared":
        from mappo_amd.utils.shared_buffer import SharedReplayBuffer
        b = SharedReplayBuffer(a, 2, [21], [42], sp, device="cpu")
        assert tuple(b.actions.shape) == (6, 4, 2, 2) and tuple(b.action_log_probs.shape) == (6, 4, 2, 2)
    else:
        from mappo_amd.utils.separated_buffer import SeparatedReplayBuffer
        b = SeparatedReplayBuffer(a, [21], [42], sp, device="cpu")
        assert b.actions.shape[-1] == 2 and b.action_log_probs.shape[-1] == 2
    assert b.available_actions is None


def test_runner_onehot():
    """actions_env: the heads' one-hots side by side (the env itself lives on the device: tests/test_gpu_multidiscrete.py)."""
    from mappo_amd.runner.shared.mpe_runner import onehot_actions
    sp = MultiDiscrete([[0, 4], [0, 9]])
    acts = torch.tensor([[[0, 9], [4, 0]], [[2, 3], [1, 7]], [[3, 3], [0, 0]]], dtype=torch.float32)
    oh = onehot_actions(acts, sp).numpy()
    want = np.concatenate([np.eye(5)[acts[..., 0].long().numpy()], np.eye(10)[acts[..., 1].long().numpy()]], -1)    # mpe_runner.py:111-117
    assert oh.shape == (3, 2, 15) and (oh == want).all()
    d = onehot_actions(torch.tensor([[[1.0], [4.0]]]), Discrete(5)).numpy()
    assert (d == np.eye(5)[[[1, 4]]]).all()


# ---- the C ABI refuses what the kernels are not built for ------------------------------------------------------------
def _desc(in_dim=21, out_dim=15, layer_N=1, recurrent=0):
    return _lib.NetDesc(in_dim, 64, out_dim, layer_N, 1, 1, recurrent)


BAD = [  # name, actor desc, head dims, avail non-NULL, words the message must contain
    ("K=5", _desc(out_dim=10), (2, 2, 2, 2, 2), False, ["n_heads", "4"]),
    ("sum", _desc(out_dim=15), (5, 9), False, ["sum", "out_dim"]),
    ("d=0", _desc(out_dim=15), (15, 0), False, ["head_dims[1]", "at least 1"]),
    ("A=17", _desc(out_dim=17), (7, 10), False, ["out_dim 17", "16"]),
    ("D=65", _desc(in_dim=65), (5, 10), False, ["in_dim 65", "64"]),
    ("LN=2", _desc(layer_N=2), (5, 10), False, ["layer_N 2"]),
    ("rec", _desc(recurrent=1), (5, 10), False, ["recurrent"]),
    ("avail", _desc(), (5, 10), True, ["avail"]),
]


@pytest.mark.parametrize("name,desc,heads,avail,words", BAD, ids=[b[0] for b in BAD])
def test_md_entry_points_reject(name, desc, heads, avail, words):
    lib = _lib.load()
    assert lib.mappo_abi_version() >= 4
    hd = (C.c_int32 * len(heads))(*heads)
    K = len(heads)
    p = C.c_void_p(4096)                      # never dereferenced: the checks come before any launch
    av = p if avail else None
    dc = _desc(in_dim=42, out_dim=1, layer_N=min(desc.layer_N, 1))
    cfg = _lib.PpoCfg(0.2, 0.01, 1.0, 10.0, 1, 1, 1, 1, 0, 0)
    calls = {
        "mappo_actor_act_md": lambda: lib.mappo_actor_act_md(p, C.byref(desc), p, av, hd, K, 16, 0, 1, 0, None, p, p, None),
        "mappo_rollout_step_md": lambda: lib.mappo_rollout_step_md(p, C.byref(desc), p, C.byref(dc), p, 0, 0, p, 0, 0, 0, 16, av, hd, K, 0, 1, 0,
                                                                   None, p, p, p, None, None, None, 0, 0, None, 0, 0, None, None, 0, None),
        "mappo_actor_update_md": lambda: lib.mappo_actor_update_md(p, C.byref(desc), p, None, 16, av, hd, K, p, p, p, p, p, C.byref(cfg), p,
                                                                   1 << 20, 0, p, None, 0, None),
        "mappo_actor_critic_update_md": lambda: lib.mappo_actor_critic_update_md(p, C.byref(desc), p, p, C.byref(dc), p, None, 16, av, hd, K, p,
                                                                                 p, p, p, p, p, None, p, C.byref(cfg), p, 1 << 20, 0, 1 << 19,
                                                                                 p, p, None),
    }
    for fn, call in calls.items():
        assert call() == -1, fn
        msg = lib.mappo_last_error().decode()
        for w in words:
            assert w in msg, (fn, msg)


def test_actor_refuses_unsupported_md_shapes():
    """R_Actor names the limit at construction (no device needed: the check comes before any allocation)."""
    from oracle import mappo_oracle as O
    from mappo_amd.algorithms.r_mappo.algorithm.r_actor_critic import R_Actor
    sp = MultiDiscrete([[0, 4], [0, 9]])
    cases = [(O.default_args(use_recurrent_policy=True), [21], sp, "recurrent"), (O.default_args(), [65], sp, "in_dim <= 64"),
             (O.default_args(layer_N=2), [21], sp, "layer_N"), (O.default_args(), [21], MultiDiscrete([[0, 8], [0, 7]]), "<= 16"),
             (O.default_args(), [21], MultiDiscrete([[0, 1]] * 5), "4 heads")]
    for a, obs, space, word in cases:
        with pytest.raises(NotImplementedError, match=word):
            R_Actor(a, obs, space, device="cpu")


# ---- the fixture generated from the reference (tests/golden/generate_golden_multidiscrete.py) ------------------------------
def _fixture_case(c):
    from conftest import golden, sub
    g = golden("multidiscrete")
    d = sub(g, f"c{c}")
    T, N, M, D, S, H, seed = [int(x) for x in d["dims"][:7]]
    heads = tuple(int(x) for x in d["dims"][7:])
    return d, (T, N, M, D, S, H, seed), heads


def test_state_dict_keys_shapes_and_seeded_init_equal_the_fixture():
    """Same keys in the same order, same shapes, and under the same torch seed the same initial weights as the reference's
    MultiDiscrete policy (one Categorical(64, d_j) per head, constructed in order; absolute 2e-5: orthogonal_'s QR runs in the host's
    LAPACK, see test_gpu_e2e.test_reference_seeded_init_matches)."""
    from oracle import mappo_oracle as O
    from conftest import sub
    from mappo_amd.algorithms.r_mappo.algorithm.r_actor_critic import R_Actor, R_Critic
    d, (T, N, M, D, S, H, seed), heads = _fixture_case(0)
    torch.manual_seed(seed)
    a = O.default_args(lr=7e-4, critic_lr=7e-4)
    actor = R_Actor(a, [D], MultiDiscrete([[0, h - 1] for h in heads]), device="cpu")
    critic = R_Critic(a, [S], device="cpu")
    assert list(actor.state_dict().keys()) == [str(k) for k in d["actor_keys"]]
    ref_a, ref_c = {k[len("init/actor/"):]: v for k, v in d.items() if k.startswith("init/actor/")}, \
        {k[len("init/critic/"):]: v for k, v in d.items() if k.startswith("init/critic/")}
    assert set(critic.state_dict().keys()) == set(ref_c.keys())
    for net, ref in ((actor, ref_a), (critic, ref_c)):
        for k, v in net.state_dict().items():
            assert tuple(v.shape) == tuple(ref[k].shape), k
            np.testing.assert_allclose(v.numpy(), ref[k], rtol=1e-5, atol=2e-5, err_msg=k)


@pytest.mark.parametrize("case", [0, 1])
def test_float64_restatement_reproduces_the_reference(case):
    """tests/md_ref.py (what every GPU update test is held against) on the reference's own minibatch: the gradient of every
    parameter and the statistics of R_MAPPO.ppo_update, to 1e-6 (gradients: of the tensor's largest entry; the reference computes in
    float32)."""
    import md_ref
    from oracle import mappo_oracle as O
    d, (T, N, M, D, S, H, seed), heads = _fixture_case(case)
    hy = d["hyper"]
    a = O.default_args(clip_param=float(hy[0]), entropy_coef=float(hy[1]), value_loss_coef=float(hy[2]), huber_delta=float(hy[3]))
    pre = lambda p: {k[len(p):]: v for k, v in d.items() if k.startswith(p)}
    actor, critic = md_ref.oracle_nets(O, a, pre("actor0/"), pre("critic0/"), D, S, heads)
    actor, critic = actor.double(), critic.double()
    s = pre("sample/")
    t = lambda x: torch.from_numpy(np.asarray(x)).double()
    act = t(s["active_masks"])
    z = actor.act.logits(actor.features(t(s["obs"]), None, None)[0], None)
    pl, ent, ratio, r = md_ref.policy_terms(z, heads, t(s["actions"]), t(s["old_action_log_probs"]), t(s["adv_targ"]), act, a.clip_param,
                                            a.use_policy_active_masks)
    vals = critic(t(s["share_obs"]), None, None)[0]
    vn = O.ValueNormRef(); vn.load_state(d["vn0"]); vn.update(s["returns"])
    tgt = vn.normalize(torch.from_numpy(s["returns"])).double()
    dummy = torch.zeros_like(tgt)
    _, vl, _ = O.ppo_losses_ref(a, dummy, dummy.sum(), vals, dummy, t(s["adv_targ"]), act, t(s["value_preds"]), tgt)
    (pl - a.entropy_coef * ent).backward()
    (vl * a.value_loss_coef).backward()
    ga = md_ref.split_head_grads({k: p.grad.numpy() for k, p in actor.named_parameters() if p.grad is not None}, heads)
    gc = {k: p.grad.numpy() for k, p in critic.named_parameters() if p.grad is not None}
    agn = np.sqrt(sum((v ** 2).sum() for v in ga.values())); cgn = np.sqrt(sum((v ** 2).sum() for v in gc.values()))
    got = np.array([vl.item(), cgn, pl.item(), ent.item(), agn, ratio.item()])
    ref = d["upd/stats"]
    print("stats rel err", np.abs(got - ref) / np.abs(ref))
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)
    np.testing.assert_allclose(r.detach().numpy(), d["upd/imp"], rtol=1e-5, atol=0)
    worst = 0.0
    for tag, grads in (("actor", ga), ("critic", gc)):
        ref_g = pre(f"upd/{tag}_grad/")
        assert set(ref_g) == set(grads), set(ref_g) ^ set(grads)
        for k, v in grads.items():
            err = np.abs(v - ref_g[k]).max() / max(np.abs(ref_g[k]).max(), 1e-12)
            worst = max(worst, err)
            assert err <= 1e-6, f"{tag} {k}: max err / max|ref| = {err:.3e}"
    print("worst gradient error", worst)
