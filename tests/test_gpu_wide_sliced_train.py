"""in_dim 513..2048 at trainer level: a policy with one or both networks beyond 512 columns is constructed on the GPU and driven
through R_MAPPO.train (mappo and rmappo) against the oracle, through a captured hipGraph against the eager sequence, and through
two MPERunner iterations on the synthetic env.  Shapes: T = 4, N = 4, M = 2 with obs 40 / share_obs 600 (a mixed pair: the actor
keeps the narrow kernels, the critic takes the sliced ones) and obs 600 / share_obs 1200 (both sliced).

This is what exercises the Python path selection at these widths: collect_into instead of the fused step, one launch per network
for the recurrent step, the feature-major recurrent update (the `narrow` test of recurrent._update_recurrent), the update dispatch
of r_mappo.py with the wide workspace, and graph capture of all of it.  Tolerances: those of the trainer-level tests at narrower
widths (test_gpu_e2e.test_runner_iteration_vs_oracle, test_gpu_gru.test_recurrent_train_straddling_chunks_vs_oracle)."""
import numpy as np
import pytest
import torch

from oracle import mappo_oracle as O
from test_gpu_e2e import M, make_args, close, BUF_NAMES, _oracle_twin   # noqa: F401  (M: the trainer-level fixture)

pytestmark = pytest.mark.gpu

T, N, Ma, A, L = 4, 4, 2, 5, 2
SHAPES = [(40, 600), (600, 1200)]


def _fill(buf, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    for n in ("share_obs", "obs", "rewards"):
        arr = getattr(buf, n); arr.copy_(torch.from_numpy(rng.standard_normal(tuple(arr.shape)).astype(f)))
    for n in ("rnn_states", "rnn_states_critic"):
        arr = getattr(buf, n); arr.copy_(torch.from_numpy((rng.standard_normal(tuple(arr.shape)) * 0.5).astype(f)))
    buf.value_preds.copy_(torch.from_numpy((rng.standard_normal(tuple(buf.value_preds.shape)) * 0.3).astype(f)))
    buf.returns.copy_(torch.from_numpy((rng.standard_normal(tuple(buf.returns.shape)) * 2).astype(f)))
    buf.actions.copy_(torch.from_numpy(rng.integers(0, A, tuple(buf.actions.shape)).astype(f)))
    buf.action_log_probs.copy_(torch.from_numpy((-np.abs(rng.standard_normal(tuple(buf.actions.shape))) * 0.3 - np.log(A)).astype(f)))
    buf.masks.copy_(torch.from_numpy((rng.random(tuple(buf.masks.shape)) > 0.15).astype(f)))
    buf.active_masks.copy_(torch.from_numpy((rng.random(tuple(buf.masks.shape)) > 0.2).astype(f)))


def _kw(rec, **more):
    kw = dict(episode_length=T, n_rollout_threads=N, lr=7e-4, critic_lr=7e-4, ppo_epoch=2, num_mini_batch=1)
    if rec:
        kw.update(use_recurrent_policy=True, data_chunk_length=L)
    kw.update(more)
    return kw


@pytest.mark.parametrize("D,S", SHAPES)
@pytest.mark.parametrize("rec", [False, True], ids=["mappo", "rmappo"])
def test_train_vs_oracle(M, rec, D, S):
    """R_MAPPO.train on a random buffer against the oracle's train() from the same weights: train_info, both networks' parameters
    after ppo_epoch updates, the ValueNorm state."""
    a = make_args(M, perm_device="cpu", **_kw(rec))
    torch.manual_seed(D + S)
    pol = M.R_MAPPOPolicy(a, [D], [S], M.Discrete(A))
    assert not pol.can_fuse_step() and not pol.can_dual_update()
    tr = M.R_MAPPO(a, pol)
    buf = M.SharedReplayBuffer(a, Ma, [D], [S], M.Discrete(A))
    _fill(buf, D)
    oa = O.default_args(**_kw(rec))
    opol = O.PolicyRef(oa, D, S, A)
    opol.actor.load_state_dict({k: v.cpu() for k, v in pol.actor.state_dict().items()})
    opol.critic.load_state_dict({k: v.cpu() for k, v in pol.critic.state_dict().items()})
    ob = O.BufferRef(oa, Ma, D, S, A)
    for n in BUF_NAMES:
        getattr(ob, n)[...] = getattr(buf, n).cpu().numpy()
    ovn = O.ValueNormRef()
    torch.manual_seed(11)
    oinfo = O.train_ref(oa, opol, ovn, ob)
    torch.manual_seed(11)
    info = tr.train(buf)
    for k in oinfo:
        close(info[k], oinfo[k], 1e-4, 1e-6, k)
    for net, onet, tag in ((pol.actor, opol.actor, "actor"), (pol.critic, opol.critic, "critic")):
        osd = onet.state_dict()
        for k, v in net.state_dict().items():
            close(v, osd[k].numpy(), 1e-4, 6e-6, f"{tag} {k}")
    close(tr.value_normalizer.state, ovn.state(), 2e-6, 1e-9)


@pytest.mark.parametrize("D,S", SHAPES)
@pytest.mark.parametrize("rec", [False, True], ids=["mappo", "rmappo"])
def test_train_graph_replay_equals_eager(M, rec, D, S):
    """Three train() calls from the same weights on the same buffer: eager every time, against eager -> capture -> replay.  The
    feed-forward sequence has no permutation (num_mini_batch = 1, rows streamed in place) and must agree bit for bit; the recurrent
    one draws its chunk permutation on the device, the same stream in both runs."""
    torch.manual_seed(D + S + 1)
    init = None
    out = {}
    for use_graph in (False, True):
        a = make_args(M, use_hip_graph=use_graph, **_kw(rec))
        pol = M.R_MAPPOPolicy(a, [D], [S], M.Discrete(A))
        if init is None:
            init = pol.flat_params.clone()
        else:
            pol.flat_params.copy_(init)
        tr = M.R_MAPPO(a, pol)
        buf = M.SharedReplayBuffer(a, Ma, [D], [S], M.Discrete(A))
        _fill(buf, S)
        torch.manual_seed(5)
        infos = [tr.train(buf) for _ in range(3)]
        torch.cuda.synchronize()
        if use_graph:
            assert any(isinstance(g, torch.cuda.CUDAGraph) for g in tr._graphs.values()), "train() was not captured"
        out[use_graph] = (pol.flat_params.clone(), infos, tr.value_normalizer.state.clone())
    (pe, ie, ve), (pg, ig, vg) = out[False], out[True]
    assert torch.isfinite(pg).all() and not torch.equal(pg, init)
    np.testing.assert_array_equal(pg.cpu().numpy(), pe.cpu().numpy())
    np.testing.assert_array_equal(vg.cpu().numpy(), ve.cpu().numpy())
    for a_, b_ in zip(ig, ie):
        assert a_ == b_


@pytest.mark.parametrize("rec", [False, True], ids=["mappo", "rmappo"])
def test_runner_two_iterations(M, rec):
    """MPERunner on the synthetic env with obs 600 / share_obs 1200 (the env's centralized state is M x obs, so the 40 / 600 pair
    does not exist there): one iteration to warm up, then a rollout whose log-probs and values the oracle recomputes from the
    stored observations (and GRU states), its bootstrap + GAE, and the second train() against the oracle's."""
    D, S = 600, 1200
    a = make_args(M, seed=1, env_name="MPE", perm_device="cpu", **_kw(rec, **(dict(algorithm_name="rmappo") if rec else {})))
    torch.manual_seed(1)
    env = M.SyntheticMPEEnv(N, Ma, D, A, T, seed=1)
    runner = M.MPERunner(dict(all_args=a, envs=env, eval_envs=None, num_agents=Ma, device=torch.device("cuda"), run_dir=None))
    assert not runner.policy.can_fuse_step()
    oa = O.default_args(**_kw(rec))
    runner.warmup()
    info0, _ = runner.run_episode()
    assert all(np.isfinite(v) for v in info0.values())
    opol, ovn = _oracle_twin(runner, oa, D, S, A)
    runner.rollout()
    b = runner.buffer
    R = N * Ma
    c = lambda x: x.cpu()
    with torch.no_grad():
        for step in range(T):
            h_a = c(b.rnn_states[step]).reshape(R, 1, 64) if rec else None
            h_c = c(b.rnn_states_critic[step]).reshape(R, 1, 64) if rec else None
            mk = c(b.masks[step]).reshape(R, 1) if rec else None
            lp, _, _ = opol.actor.evaluate_actions(c(b.obs[step]).reshape(R, D), h_a, c(b.actions[step]).reshape(R, 1), mk)
            v, _ = opol.critic(c(b.share_obs[step]).reshape(R, S), h_c, mk)
            close(b.action_log_probs[step].reshape(R, 1), lp.numpy(), 1e-5, 3e-6, f"logp step {step}")
            close(b.value_preds[step].reshape(R, 1), v.numpy(), 1e-5, 3e-6, f"value step {step}")
    np.testing.assert_array_equal(b.share_obs[2, :, 0].cpu().numpy(), b.obs[2].reshape(N, -1).cpu().numpy())
    ob = O.BufferRef(oa, Ma, D, S, A)
    for n in BUF_NAMES:
        if n != "returns":
            getattr(ob, n)[...] = getattr(b, n).cpu().numpy()
    with torch.no_grad():
        nv, _ = opol.critic(torch.from_numpy(np.concatenate(ob.share_obs[-1])),
                            torch.from_numpy(np.concatenate(ob.rnn_states_critic[-1])) if rec else None,
                            torch.from_numpy(np.concatenate(ob.masks[-1])) if rec else None)
    ob.compute_returns(np.array(np.split(nv.numpy(), N)), ovn)
    close(b.returns[:T], ob.returns[:T], 1e-5, 3e-6)
    torch.manual_seed(21)
    oinfo = O.train_ref(oa, opol, ovn, ob)
    torch.manual_seed(21)
    info = runner.train()
    for k in oinfo:
        close(info[k], oinfo[k], 1e-4, 1e-6, k)
    for net, onet, tag in ((runner.policy.actor, opol.actor, "actor"), (runner.policy.critic, opol.critic, "critic")):
        osd = onet.state_dict()
        for k, v in net.state_dict().items():
            close(v, osd[k].numpy(), 1e-4, 6e-6, f"{tag} {k}")
    close(runner.trainer.value_normalizer.state, ovn.state(), 2e-6, 1e-9)
