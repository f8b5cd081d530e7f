"""Tensor-level wrappers over the C ABI (include/mappo_hip.h).  torch is plumbing here: device memory,
streams, shapes.  Every function enqueues on torch's current stream of the tensors' device and returns
without synchronising."""
import ctypes as C

import torch

from . import _lib
from ._lib import NetDesc, PpoCfg


def _ptr(t, dtype=torch.float32, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError("tensor required")
    if not t.is_cuda:
        raise _lib.MappoHipError("mappo_amd ops need tensors in HBM (cuda/hip device); got a CPU tensor — "
                                 "there is no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _u64(x):
    return int(x) & (2 ** 64 - 1)


def _ptrs(tensors, dtypes):
    """Pointers of an env's state tensors, in the order of its entry points, each with the dtype the kernels read it as."""
    return [_ptr(t, d) for t, d in zip(tensors, dtypes, strict=True)]


def _env_call(symbol, *args):
    """An entry point that ends in the stream argument: call it on the current stream, check its return code under its name."""
    _lib.check(getattr(_lib.load(), symbol)(*args, _stream()), symbol)


def _ws(nbytes, device):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def net_desc(in_dim, out_dim, layer_N=1, use_relu=True, use_feature_norm=True, recurrent=False, hidden=64):
    return NetDesc(int(in_dim), int(hidden), int(out_dim), int(layer_N), int(bool(use_relu)),
                   int(bool(use_feature_norm)), int(bool(recurrent)))


def net_param_count(desc):
    return int(_lib.load().mappo_net_param_count(C.byref(desc)))


# ---- K1 -------------------------------------------------------------------------------------------
def insert_mpe(obs, rewards, dones, obs_dst, share_dst, rew_dst, mask_dst, centralized):
    """obs [N, M, D] (innermost stride 1), rewards [N, M(, 1)], dones [N, M] bool — device tensors, arbitrary outer strides."""
    N, M, D = obs.shape
    if rewards.dim() == 3:
        rewards = rewards[..., 0]
    assert obs.is_cuda and obs.dtype == torch.float32 and obs.stride(2) == 1 and rewards.dtype == torch.float32 and dones.dtype == torch.bool
    rc = _lib.load().mappo_insert_mpe(C.c_void_p(obs.data_ptr()), obs.stride(0), obs.stride(1), C.c_void_p(rewards.data_ptr()),
                                      rewards.stride(0), rewards.stride(1), C.c_void_p(dones.data_ptr()), dones.stride(0),
                                      dones.stride(1), _ptr(obs_dst), _ptr(share_dst), _ptr(rew_dst), _ptr(mask_dst), int(N), int(M),
                                      int(D), int(bool(centralized)), _stream())
    _lib.check(rc, "mappo_insert_mpe")


def insert_mpe_rnn(obs, rewards, dones, obs_dst, share_dst, rew_dst, mask_dst, centralized, rnn_states, rnn_states_critic, rnn_dst,
                   rnn_critic_dst):
    """insert_mpe + rnn_dst / rnn_critic_dst = states * (1 - done) in the same launch (contiguous fp32 [N*M, H] state arrays)."""
    N, M, D = obs.shape
    if rewards.dim() == 3:
        rewards = rewards[..., 0]
    assert obs.is_cuda and obs.dtype == torch.float32 and obs.stride(2) == 1 and rewards.dtype == torch.float32 and dones.dtype == torch.bool
    H = rnn_states.numel() // (N * M)
    assert rnn_states.numel() == rnn_states_critic.numel() == rnn_dst.numel() == rnn_critic_dst.numel() == N * M * H
    rc = _lib.load().mappo_insert_mpe_rnn(C.c_void_p(obs.data_ptr()), obs.stride(0), obs.stride(1), C.c_void_p(rewards.data_ptr()),
                                          rewards.stride(0), rewards.stride(1), C.c_void_p(dones.data_ptr()), dones.stride(0),
                                          dones.stride(1), _ptr(obs_dst), _ptr(share_dst), _ptr(rew_dst), _ptr(mask_dst), int(N), int(M),
                                          int(D), int(bool(centralized)), _ptr(rnn_states), _ptr(rnn_states_critic), _ptr(rnn_dst),
                                          _ptr(rnn_critic_dst), int(H), _stream())
    _lib.check(rc, "mappo_insert_mpe_rnn")


def insert_smac(obs, share_obs, avail, rewards, dones, bad, rnn_states, rnn_states_critic, obs_dst, share_dst, avail_dst, rew_dst, mask_dst,
                bad_dst, active_dst, rnn_dst, rnn_critic_dst):
    """SMAC rollout insert in one launch (mappo_insert_smac): contiguous fp32 obs [N, M, D] / share_obs [N, M, S] / avail [N, M, A] (or
    None), rewards [N, M(, 1)] (any strides), dones [N, M] bool, bad [N, M] bool contiguous or None, states [N*M, ., H] or None."""
    N, M, D = obs.shape
    S = share_obs.shape[-1]
    if rewards.dim() == 3:
        rewards = rewards[..., 0]
    A = avail.shape[-1] if avail is not None else 0
    H = rnn_states.numel() // (N * M) if rnn_states is not None else 0
    n = lambda t: _ptr(t, allow_none=True)
    rc = _lib.load().mappo_insert_smac(_ptr(obs), _ptr(share_obs), n(avail), C.c_void_p(rewards.data_ptr()), rewards.stride(0),
                                       rewards.stride(1), C.c_void_p(dones.data_ptr()), dones.stride(0), dones.stride(1),
                                       C.c_void_p(bad.data_ptr()) if bad is not None else None, n(rnn_states), n(rnn_states_critic),
                                       _ptr(obs_dst), _ptr(share_dst), n(avail_dst), _ptr(rew_dst), _ptr(mask_dst), _ptr(bad_dst),
                                       _ptr(active_dst), n(rnn_dst), n(rnn_critic_dst), int(N), int(M), int(D), int(S), int(A), int(H),
                                       _stream())
    _lib.check(rc, "mappo_insert_smac")


def recurrent_rollout_step(actor_params, actor_desc, critic_params, critic_desc, obs, share_obs, avail, rewards, dones, bad, actor_h, critic_h,
                           actor_h_next, critic_h_next, deterministic, seed, counter, counter_dev, actions, logp, values, slot):
    """mappo_recurrent_rollout_step: SMAC insert of the pending env output (obs [N, M, D], share_obs [N, M, S], avail [N, M, A] or None,
    rewards [N, M(, 1)], dones [N, M] bool, bad [N, M] bool or None; states [N*M, ., 64]) into the arrays of `slot` (dict: obs, share_obs,
    available_actions, rewards, masks, bad_masks, active_masks, rnn_states, rnn_states_critic) + get_actions / get_values on it."""
    N, M, _ = obs.shape
    if rewards.dim() == 3:
        rewards = rewards[..., 0]
    sl = _lib.SmacSlot(*[(slot[k].data_ptr() if slot.get(k) is not None else None) for k, _ in _lib.SmacSlot._fields_])
    for k, _ in _lib.SmacSlot._fields_:
        t = slot.get(k)
        if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise ValueError(f"slot[{k}] must be a contiguous fp32 device tensor")
    n = lambda t: _ptr(t, allow_none=True)
    rc = _lib.load().mappo_recurrent_rollout_step(
        _ptr(actor_params), C.byref(actor_desc), _ptr(critic_params), C.byref(critic_desc), _ptr(obs), _ptr(share_obs), n(avail),
        C.c_void_p(rewards.data_ptr()), rewards.stride(0), rewards.stride(1), C.c_void_p(dones.data_ptr()), dones.stride(0), dones.stride(1),
        C.c_void_p(bad.data_ptr()) if bad is not None else None, _ptr(actor_h), _ptr(critic_h), _ptr(actor_h_next), _ptr(critic_h_next),
        int(N), int(M), int(bool(deterministic)), int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1),
        _ptr(counter_dev, torch.int64, allow_none=True), _ptr(actions), _ptr(logp), _ptr(values), C.byref(sl), _stream())
    _lib.check(rc, "mappo_recurrent_rollout_step")


def recurrent_rows(perm, L, T, R, num_mini_batch):
    """perm [E, data_chunks] int64 (device) -> rows [E, nmb, L*mbs], h0_rows [E, nmb, mbs] int32 (mappo_recurrent_rows)."""
    E, chunks = perm.shape
    mbs = chunks // num_mini_batch
    rows = torch.empty(E, num_mini_batch, L * mbs, dtype=torch.int32, device=perm.device)
    h0 = torch.empty(E, num_mini_batch, mbs, dtype=torch.int32, device=perm.device)
    rc = _lib.load().mappo_recurrent_rows(_ptr(perm, torch.int64), int(E), int(chunks), int(L), int(T), int(R), int(num_mini_batch),
                                          _ptr(rows, torch.int32), _ptr(h0, torch.int32), _stream())
    _lib.check(rc, "mappo_recurrent_rows")
    return rows, h0


def copy_batch(pairs):
    """[(dst, src), ...] contiguous fp32 device tensors of equal numel per pair, copied in ONE launch (<= 16 pairs)."""
    n = len(pairs)
    dst = (C.c_void_p * n)(*[d.data_ptr() for d, _ in pairs])
    src = (C.c_void_p * n)(*[s.data_ptr() for _, s in pairs])
    cnt = (C.c_int64 * n)(*[d.numel() for d, _ in pairs])
    for d, s_ in pairs:
        assert d.is_cuda and s_.is_cuda and d.dtype == torch.float32 and s_.dtype == torch.float32 and d.is_contiguous() \
            and s_.is_contiguous() and d.numel() == s_.numel()
    rc = _lib.load().mappo_copy_batch(n, dst, src, cnt, _stream())
    _lib.check(rc, "mappo_copy_batch")


# ---- K2 -------------------------------------------------------------------------------------------
def gae_scan(rewards, value_preds, next_value, masks, bad_masks, returns, vn_state, gamma, gae_lambda,
             use_gae=True, use_proper_time_limits=False):
    """compute_returns (shared_buffer.py:168-224) in place on [T(+1), R] views of the buffer arrays."""
    T = rewards.shape[0]
    R = rewards.numel() // T
    lib = _lib.load()
    rc = lib.mappo_gae_scan(_ptr(rewards), _ptr(value_preds), _ptr(next_value), _ptr(masks),
                            _ptr(bad_masks, allow_none=True), _ptr(returns), _ptr(vn_state, allow_none=True),
                            T, R, float(gamma), float(gae_lambda), int(bool(use_gae)),
                            int(bool(use_proper_time_limits)), _stream())
    _lib.check(rc, "mappo_gae_scan")


# ---- K3 -------------------------------------------------------------------------------------------
def adv_moments(returns, value_preds, active_masks, vn_state, adv, moments, workspace=None):
    lib = _lib.load()
    n = adv.numel()
    if workspace is None:
        workspace = _ws(lib.mappo_adv_workspace_bytes(n), adv.device)
    rc = lib.mappo_adv_moments(_ptr(returns), _ptr(value_preds), _ptr(active_masks), _ptr(vn_state, allow_none=True),
                               _ptr(adv), _ptr(moments, torch.float64), _ptr(workspace, torch.uint8), n, _stream())
    _lib.check(rc, "mappo_adv_moments")


def adv_normalize(adv, moments):
    rc = _lib.load().mappo_adv_normalize(_ptr(adv), _ptr(moments, torch.float64), adv.numel(), _stream())
    _lib.check(rc, "mappo_adv_normalize")


# ---- K12 ------------------------------------------------------------------------------------------
def minibatch_moments(returns, active_masks, rows, B, mb_moments, workspace=None):
    lib = _lib.load()
    if workspace is None:
        workspace = _ws(lib.mappo_moments_workspace_bytes(B), returns.device)
    rc = lib.mappo_minibatch_moments(_ptr(returns), _ptr(active_masks), _ptr(rows, torch.int32, allow_none=True), int(B),
                                     _ptr(mb_moments, torch.float64), _ptr(workspace, torch.uint8), _stream())
    _lib.check(rc, "mappo_minibatch_moments")


def valuenorm_update(vn_state, mb_moments, beta=0.99999):
    rc = _lib.load().mappo_valuenorm_update(_ptr(vn_state), _ptr(mb_moments, torch.float64), float(beta), _stream())
    _lib.check(rc, "mappo_valuenorm_update")


def valuenorm_update_n(vn_state, mb_moments, beta, n, states_out):
    """n ValueNorm.update calls with the same batch moments in one launch; states_out [n, 3]."""
    rc = _lib.load().mappo_valuenorm_update_n(_ptr(vn_state), _ptr(mb_moments, torch.float64), float(beta), int(n), _ptr(states_out),
                                              _stream())
    _lib.check(rc, "mappo_valuenorm_update_n")


# ---- K5 -------------------------------------------------------------------------------------------
def ppo_cfg(args, accumulate_partials=False):
    return PpoCfg(float(args.clip_param), float(args.entropy_coef), float(args.value_loss_coef), float(args.huber_delta),
                  int(bool(args.use_huber_loss)), int(bool(args.use_clipped_value_loss)),
                  int(bool(args.use_policy_active_masks)), int(bool(args.use_value_active_masks)),
                  int(bool(args.use_valuenorm)), int(bool(accumulate_partials)))


def ppo_loss_fwd_bwd(logits, values, rows, avail, actions, old_logp, adv, active, v_old, returns, vn_state, mb_moments,
                     dlogits, dvalues, stats, cfg, workspace=None):
    lib = _lib.load()
    B, A = logits.shape
    if workspace is None:
        workspace = _ws(lib.mappo_ppo_loss_workspace_bytes(B), logits.device)
    rc = lib.mappo_ppo_loss_fwd_bwd(_ptr(logits), _ptr(values), _ptr(rows, torch.int32, allow_none=True),
                                    _ptr(avail, allow_none=True), _ptr(actions), _ptr(old_logp), _ptr(adv), _ptr(active),
                                    _ptr(v_old), _ptr(returns), _ptr(vn_state, allow_none=True),
                                    _ptr(mb_moments, torch.float64), _ptr(dlogits), _ptr(dvalues),
                                    _ptr(stats, torch.float64), _ptr(workspace, torch.uint8), C.byref(cfg), int(B), int(A),
                                    _stream())
    _lib.check(rc, "mappo_ppo_loss_fwd_bwd")


# ---- K7 / K8 --------------------------------------------------------------------------------------
def mlp_forward(params, desc, x, rows, B, out):
    rc = _lib.load().mappo_mlp_forward(_ptr(params), C.byref(desc), _ptr(x), _ptr(rows, torch.int32, allow_none=True),
                                       int(B), _ptr(out), _stream())
    _lib.check(rc, "mappo_mlp_forward")


def actor_act(params, desc, obs, avail, B, deterministic, seed, counter, actions, logp, counter_dev=None):
    rc = _lib.load().mappo_actor_act(_ptr(params), C.byref(desc), _ptr(obs), _ptr(avail, allow_none=True), int(B),
                                     int(bool(deterministic)), int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1),
                                     _ptr(counter_dev, torch.int64, allow_none=True), _ptr(actions), _ptr(logp), _stream())
    _lib.check(rc, "mappo_actor_act")


def rollout_step(actor_params, actor_desc, critic_params, critic_desc, obs, share_obs, M, B, avail, deterministic, seed, counter,
                 counter_dev, actions, logp, values, insert=None):
    """Fused rollout step.  obs / share_obs: (tensor, stride_n, stride_m) row sources (strides in elements; M == 0 means
    contiguous [B][D] and the strides are ignored).  insert: None or dict(obs_dst, share_dst, rewards=(tensor, sn, sm),
    dones=(tensor, sn, sm), rew_dst, mask_dst, centralized) — the env output `obs` comes from is copied into those slots."""
    ot, osn, osm = obs
    st, ssn, ssm = share_obs
    if insert is None:
        ins = (None, None, None, 0, 0, None, 0, 0, None, None, 0)
    else:
        rt, rsn, rsm = insert["rewards"]
        dt, dsn, dsm = insert["dones"]
        ins = (C.c_void_p(insert["obs_dst"].data_ptr()), C.c_void_p(insert["share_dst"].data_ptr()), C.c_void_p(rt.data_ptr()), int(rsn), int(rsm),
               C.c_void_p(dt.data_ptr()), int(dsn), int(dsm), C.c_void_p(insert["rew_dst"].data_ptr()), C.c_void_p(insert["mask_dst"].data_ptr()),
               int(bool(insert["centralized"])))
    rc = _lib.load().mappo_rollout_step(_ptr(actor_params), C.byref(actor_desc), _ptr(critic_params), C.byref(critic_desc),
                                        C.c_void_p(ot.data_ptr()), int(osn), int(osm), C.c_void_p(st.data_ptr()), int(ssn), int(ssm), int(M), int(B),
                                        _ptr(avail, allow_none=True), int(bool(deterministic)), int(seed) & (2 ** 64 - 1),
                                        int(counter) & (2 ** 64 - 1), _ptr(counter_dev, torch.int64, allow_none=True),
                                        _ptr(actions, allow_none=True), _ptr(logp, allow_none=True), _ptr(values), *ins, _stream())
    _lib.check(rc, "mappo_rollout_step")


# ---- MultiDiscrete action spaces: one Categorical head per sub-action (mappo_*_md) ---------------------------------
def _heads(head_dims):
    arr = (C.c_int32 * len(head_dims))(*[int(d) for d in head_dims])
    return arr, len(head_dims)


def actor_act_md(params, desc, obs, head_dims, B, deterministic, seed, counter, actions, logp, counter_dev=None, avail=None):
    """get_actions of a MultiDiscrete policy: actions / logp [B, K] (mappo_actor_act_md)."""
    arr, K = _heads(head_dims)
    rc = _lib.load().mappo_actor_act_md(_ptr(params), C.byref(desc), _ptr(obs), _ptr(avail, allow_none=True), arr, K, int(B),
                                        int(bool(deterministic)), int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1),
                                        _ptr(counter_dev, torch.int64, allow_none=True), _ptr(actions), _ptr(logp), _stream())
    _lib.check(rc, "mappo_actor_act_md")


def rollout_step_md(actor_params, actor_desc, critic_params, critic_desc, obs, share_obs, M, B, head_dims, deterministic, seed, counter,
                    counter_dev, actions, logp, values, insert=None, avail=None):
    """rollout_step for a MultiDiscrete policy (actions / logp [B, K]); arguments as rollout_step."""
    ot, osn, osm = obs
    st, ssn, ssm = share_obs
    arr, K = _heads(head_dims)
    if insert is None:
        ins = (None, None, None, 0, 0, None, 0, 0, None, None, 0)
    else:
        rt, rsn, rsm = insert["rewards"]
        dt, dsn, dsm = insert["dones"]
        ins = (C.c_void_p(insert["obs_dst"].data_ptr()), C.c_void_p(insert["share_dst"].data_ptr()), C.c_void_p(rt.data_ptr()), int(rsn), int(rsm),
               C.c_void_p(dt.data_ptr()), int(dsn), int(dsm), C.c_void_p(insert["rew_dst"].data_ptr()), C.c_void_p(insert["mask_dst"].data_ptr()),
               int(bool(insert["centralized"])))
    rc = _lib.load().mappo_rollout_step_md(_ptr(actor_params), C.byref(actor_desc), _ptr(critic_params), C.byref(critic_desc),
                                           C.c_void_p(ot.data_ptr()), int(osn), int(osm), C.c_void_p(st.data_ptr()), int(ssn), int(ssm), int(M),
                                           int(B), _ptr(avail, allow_none=True), arr, K, int(bool(deterministic)), int(seed) & (2 ** 64 - 1),
                                           int(counter) & (2 ** 64 - 1), _ptr(counter_dev, torch.int64, allow_none=True),
                                           _ptr(actions, allow_none=True), _ptr(logp, allow_none=True), _ptr(values), *ins, _stream())
    _lib.check(rc, "mappo_rollout_step_md")


def actor_update_md(params, desc, obs, rows, B, head_dims, actions, old_logp, adv, active, mb_moments, cfg, slabs, slab_stride,
                    slab_col0, partials, n_blocks=0, avail=None):
    """actor_update for a MultiDiscrete policy: actions / old_logp [., K] in buffer order (mappo_actor_update_md)."""
    arr, K = _heads(head_dims)
    rc = _lib.load().mappo_actor_update_md(_ptr(params), C.byref(desc), _ptr(obs), _ptr(rows, torch.int32, allow_none=True), int(B),
                                           _ptr(avail, allow_none=True), arr, K, _ptr(actions), _ptr(old_logp), _ptr(adv), _ptr(active),
                                           _ptr(mb_moments, torch.float64), C.byref(cfg), _ptr(slabs), int(slab_stride), int(slab_col0),
                                           _ptr(partials, torch.float64), None, int(n_blocks), _stream())
    _lib.check(rc, "mappo_actor_update_md")


def actor_critic_update_md(actor_params, actor_desc, obs, critic_params, critic_desc, share_obs, rows, B, head_dims, actions, old_logp,
                           adv, active, v_old, returns, vn_state, mb_moments, cfg, slabs, slab_stride, actor_col0, critic_col0,
                           actor_partials, critic_partials, avail=None):
    """actor_critic_update for a MultiDiscrete policy (mappo_actor_critic_update_md); slab / partial rows per network:
    dual_update_slabs(actor_desc, critic_desc, B)."""
    arr, K = _heads(head_dims)
    rc = _lib.load().mappo_actor_critic_update_md(_ptr(actor_params), C.byref(actor_desc), _ptr(obs), _ptr(critic_params),
                                                  C.byref(critic_desc), _ptr(share_obs), _ptr(rows, torch.int32, allow_none=True), int(B),
                                                  _ptr(avail, allow_none=True), arr, K, _ptr(actions), _ptr(old_logp), _ptr(adv),
                                                  _ptr(active), _ptr(v_old), _ptr(returns), _ptr(vn_state, allow_none=True),
                                                  _ptr(mb_moments, torch.float64), C.byref(cfg), _ptr(slabs), int(slab_stride),
                                                  int(actor_col0), int(critic_col0), _ptr(actor_partials, torch.float64),
                                                  _ptr(critic_partials, torch.float64), _stream())
    _lib.check(rc, "mappo_actor_critic_update_md")


def _strided(t, dtype):
    """Pointer of a (possibly strided) device view, for the entry points that take explicit strides."""
    if not t.is_cuda:
        raise _lib.MappoHipError("mappo_amd ops need tensors in HBM (cuda/hip device); got a CPU tensor — there is no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


def rollout_episode(actor_params, actor_desc, critic_params, critic_desc, obs, rewards, dones, deterministic, seed, counter, counter_dev,
                    obs_buf, share_buf, rew_buf, mask_buf, actions, logp, values, next_values, centralized):
    """A whole rollout episode in one launch (mappo_rollout_episode).  obs [T, N, M, D], rewards [T, N, M] (or [T, N, M, 1]),
    dones [T, N, M] bool: the env output of every step, any strides (d contiguous); the buffer arrays are the contiguous
    SharedReplayBuffer tensors (obs / share_obs / masks [T+1, ...], rewards / actions / action_log_probs [T, ...], value_preds
    [T+1, ...] of which slots 0..T-1 are written); next_values [N*M] receives the critic of step T."""
    T, N, M, D = obs.shape
    if obs.stride(3) != 1:
        raise ValueError("rollout_episode: obs rows must be contiguous in the feature dimension")
    if rewards.dim() == 4:
        rewards = rewards[..., 0]
    if tuple(rewards.shape) != (T, N, M) or tuple(dones.shape) != (T, N, M):
        raise ValueError(f"rollout_episode: rewards {tuple(rewards.shape)} / dones {tuple(dones.shape)} do not match obs {tuple(obs.shape)}")
    R = N * M
    rc = _lib.load().mappo_rollout_episode(_ptr(actor_params), C.byref(actor_desc), _ptr(critic_params), C.byref(critic_desc), int(T), int(N),
                                           int(M), _strided(obs, torch.float32), int(obs.stride(0)), int(obs.stride(1)), int(obs.stride(2)),
                                           _strided(rewards, torch.float32), int(rewards.stride(0)), int(rewards.stride(1)), int(rewards.stride(2)),
                                           _strided(dones, torch.bool), int(dones.stride(0)), int(dones.stride(1)), int(dones.stride(2)),
                                           int(bool(deterministic)), int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1),
                                           _ptr(counter_dev, torch.int64, allow_none=True), _ptr(obs_buf), _ptr(share_buf), _ptr(rew_buf),
                                           _ptr(mask_buf), _ptr(actions), _ptr(logp), _ptr(values), _ptr(next_values),
                                           int(bool(centralized)), _stream())
    _lib.check(rc, "mappo_rollout_episode")


# dtypes of the GPU-resident MPE envs' state tensors, in the order every entry point of a scenario takes them.  These rows guard
# the ABI (include/mappo_hip.h); the envs' `state` descriptions (envs/mpe_*.py) state the same dtypes again to allocate with, and
# a disagreement shows here as _ptr's TypeError at the first call
_F64, _I32, _I64 = torch.float64, torch.int32, torch.int64
_STATE_BODIES = (_F64, _F64, _F64, _I32, _I64)                  # agent_pos, agent_vel, landmark_pos, tstep, episode: spread, tag, world_comm
_STATE_GOAL = (_F64, _F64, _F64, _I32, _I32, _I64)              # ... landmark_pos, goal, tstep, episode: reference, adversary, push
_STATE_COMM = (_F64, _F64, _F64, _I32, _I32, _I32, _I64)        # listener_pos, listener_vel, landmark_pos, goal, symbol, tstep, episode
_STATE_CRYPTO = (_I32, _I32, _I32, _I32, _I64)                  # goal, key, comm, tstep, episode


def rollout_episode_spread(actor_params, actor_desc, critic_params, critic_desc, T, N, M, L, env_episode_length, env_seed, agent_pos,
                           agent_vel, landmark_pos, tstep, episode, deterministic, seed, counter, counter_dev, obs_buf, share_buf,
                           rew_buf, mask_buf, actions, logp, values, next_values, centralized):
    """A whole rollout episode on the GPU-resident simple_spread env in one launch, env steps included
    (mappo_rollout_episode_spread): the five env state tensors (SimpleSpreadVecEnv) are read, stepped T times on the sampled
    actions and stored back; the buffer arrays are the contiguous SharedReplayBuffer tensors, as for rollout_episode."""
    _env_call("mappo_rollout_episode_spread", _ptr(actor_params), C.byref(actor_desc), _ptr(critic_params), C.byref(critic_desc), int(T),
              int(N), int(M), int(L), int(env_episode_length), _u64(env_seed),
              *_ptrs((agent_pos, agent_vel, landmark_pos, tstep, episode), _STATE_BODIES), int(bool(deterministic)), _u64(seed),
              _u64(counter), _ptr(counter_dev, _I64, allow_none=True),
              *map(_ptr, (obs_buf, share_buf, rew_buf, mask_buf, actions, logp, values, next_values)), int(bool(centralized)))


def rollout_episode_spread_recurrent(actor_params, actor_desc, critic_params, critic_desc, T, N, M, L, env_episode_length, env_seed,
                                     agent_pos, agent_vel, landmark_pos, tstep, episode, deterministic, seed, counter, counter_dev,
                                     obs_buf, share_buf, rew_buf, mask_buf, actions, logp, values, rnn_states, rnn_states_critic,
                                     centralized):
    """The one-launch simple_spread episode of a recurrent shared policy (mappo_rollout_episode_spread_recurrent): as
    rollout_episode_spread, with the buffer's two rnn-state arrays [T+1, N, M, 1, 64] read at slot 0 and written at slots 1..T,
    and without the bootstrap value."""
    _env_call("mappo_rollout_episode_spread_recurrent", _ptr(actor_params), C.byref(actor_desc), _ptr(critic_params),
              C.byref(critic_desc), int(T), int(N), int(M), int(L), int(env_episode_length), _u64(env_seed),
              *_ptrs((agent_pos, agent_vel, landmark_pos, tstep, episode), _STATE_BODIES), int(bool(deterministic)), _u64(seed),
              _u64(counter), _ptr(counter_dev, _I64, allow_none=True),
              *map(_ptr, (obs_buf, share_buf, rew_buf, mask_buf, actions, logp, values, rnn_states, rnn_states_critic)),
              int(bool(centralized)))


def eval_episode_spread(actor_params, actor_desc, T, N, M, L, env_episode_length, env_seed, agent_pos, agent_vel, landmark_pos, tstep,
                        episode, deterministic, seed, counter, counter_dev, returns, actions=None):
    """A whole evaluation episode on the GPU-resident simple_spread env in one launch (mappo_eval_episode_spread): the actor acts
    and the env steps T times on the five state tensors, which are advanced in place; returns [N, M] receives each row's sum of
    the step rewards (fp32, in step order), actions [T, N*M] (optional) the chosen actions.  Nothing else is written."""
    _env_call("mappo_eval_episode_spread", _ptr(actor_params), C.byref(actor_desc), int(T), int(N), int(M), int(L),
              int(env_episode_length), _u64(env_seed), *_ptrs((agent_pos, agent_vel, landmark_pos, tstep, episode), _STATE_BODIES),
              int(bool(deterministic)), _u64(seed), _u64(counter), _ptr(counter_dev, _I64, allow_none=True), _ptr(returns),
              _ptr(actions, allow_none=True))


def rollout_episode_smac_recurrent(actor_params, actor_desc, critic_params, critic_desc, env_obs, env_share_obs, env_avail, env_rewards,
                                   env_dones, env_bad, deterministic, seed, counter, counter_dev, obs_buf, share_buf, avail_buf, rew_buf,
                                   mask_buf, bad_mask_buf, active_mask_buf, rnn_states, rnn_states_critic, actions, logp, values, centralized):
    """The one-launch episode of a recurrent shared policy on SMAC-shaped env output (mappo_rollout_episode_smac_recurrent).  env_*:
    the env output of all T steps, contiguous — obs [T, N, M, D], share_obs [T, N, M, S] (None when not centralized), avail
    [T, N, M, A] or None, rewards [T, N], dones [T, N, M] bool, bad [N, M] bool or None; the buffer arrays are the contiguous
    SharedReplayBuffer tensors (available_actions None together with env_avail).  A limit the kernel refuses (a wide observation,
    layer_N 2, a feed-forward descriptor, more than 16 agents, ...) raises ValueError with the library's message."""
    if env_obs.dim() != 4 or tuple(env_dones.shape) != tuple(env_obs.shape[:3]) or tuple(env_rewards.shape) != tuple(env_obs.shape[:2]):
        raise ValueError(f"rollout_episode_smac_recurrent: env output shapes obs {tuple(env_obs.shape)} / rewards {tuple(env_rewards.shape)} / "
                         f"dones {tuple(env_dones.shape)} are not [T, N, M, D] / [T, N] / [T, N, M]")
    T, N, M, _ = env_obs.shape
    n = lambda t, dtype=torch.float32: _ptr(t, dtype, allow_none=True)
    rc = _lib.load().mappo_rollout_episode_smac_recurrent(
        _ptr(actor_params), C.byref(actor_desc), _ptr(critic_params), C.byref(critic_desc), int(T), int(N), int(M), _ptr(env_obs),
        n(env_share_obs), n(env_avail), _ptr(env_rewards), _ptr(env_dones, torch.bool), n(env_bad, torch.bool), int(bool(deterministic)),
        _u64(seed), _u64(counter), n(counter_dev, _I64), _ptr(obs_buf), _ptr(share_buf), n(avail_buf), _ptr(rew_buf), _ptr(mask_buf),
        _ptr(bad_mask_buf), _ptr(active_mask_buf), _ptr(rnn_states), _ptr(rnn_states_critic), _ptr(actions), _ptr(logp), _ptr(values),
        int(bool(centralized)), _stream())
    if rc == -1:                                       # MAPPO_EINVAL: refused on the host, nothing was launched
        raise ValueError(_lib.load().mappo_last_error().decode("utf-8", "replace"))
    _lib.check(rc, "mappo_rollout_episode_smac_recurrent")


def rollout_episode_reference(actor_params, actor_desc, critic_params, critic_desc, head_dims, T, N, env_episode_length, env_seed,
                              agent_pos, agent_vel, landmark_pos, goal, tstep, episode, deterministic, seed, counter, counter_dev, obs_buf,
                              share_buf, rew_buf, mask_buf, actions, logp, values, next_values, centralized):
    """A whole rollout episode on the GPU-resident simple_reference env in one launch, env steps included
    (mappo_rollout_episode_reference): the six env state tensors (SimpleReferenceVecEnv) are read, stepped T times on the sampled
    head indices and stored back; the buffer arrays are the contiguous SharedReplayBuffer tensors (actions / action_log_probs
    [T, N, 2, 2]).  head_dims must be (5, 10)."""
    arr, K = _heads(head_dims)
    _env_call("mappo_rollout_episode_reference", _ptr(actor_params), C.byref(actor_desc), _ptr(critic_params), C.byref(critic_desc), arr, K,
              int(T), int(N), int(env_episode_length), _u64(env_seed),
              *_ptrs((agent_pos, agent_vel, landmark_pos, goal, tstep, episode), _STATE_GOAL), int(bool(deterministic)), _u64(seed),
              _u64(counter), _ptr(counter_dev, _I64, allow_none=True),
              *map(_ptr, (obs_buf, share_buf, rew_buf, mask_buf, actions, logp, values, next_values)), int(bool(centralized)))


# ---- one rollout episode of the SEPARATED runner in one launch, env steps included (csrc/rollout_separated.h) ------------------------
def comm_agent(actor_params, actor_desc, critic_params, critic_desc, seed, counter_dev, obs_buf, share_buf, rew_buf, mask_buf, actions, logp, values,
               next_values):
    """One agent of a separated one-launch episode (mappo_comm_agent; rollout_episode_comm and the five below it): its networks, its
    sampling seed and counter word (int64 [1] device tensor or None) and the contiguous arrays of its SeparatedReplayBuffer."""
    ag = _lib.CommAgent()
    ag.actor_params, ag.critic_params = _ptr(actor_params).value, _ptr(critic_params).value
    ag.actor_desc, ag.critic_desc = actor_desc, critic_desc
    ag.seed = _u64(seed)
    cd = _ptr(counter_dev, _I64, allow_none=True)
    ag.counter_dev = cd.value if cd is not None else None
    for name, t in (("obs_buf", obs_buf), ("share_buf", share_buf), ("rew_buf", rew_buf), ("mask_buf", mask_buf), ("actions", actions),
                    ("logp", logp), ("values", values), ("next_values", next_values)):
        setattr(ag, name, _ptr(t).value)
    return ag


def rollout_episode_comm(speaker, listener, T, N, env_episode_length, env_seed, listener_pos, listener_vel, landmark_pos, goal, symbol,
                         tstep, episode, deterministic, counter, centralized):
    """The episode on the GPU-resident simple_speaker_listener env (mappo_rollout_episode_comm).  speaker / listener: comm_agent(...)
    of agent 0 / 1; the seven env state tensors (SimpleSpeakerListenerVecEnv) are read, stepped T times on the sampled indices and
    stored back."""
    _env_call("mappo_rollout_episode_comm", C.byref(speaker), C.byref(listener), int(T), int(N), int(env_episode_length), _u64(env_seed),
              *_ptrs((listener_pos, listener_vel, landmark_pos, goal, symbol, tstep, episode), _STATE_COMM), int(bool(deterministic)),
              _u64(counter), int(bool(centralized)))


def _episode_agents(who, scenario, M, agents):
    """The M comm_agent(...) of a separated one-launch episode as the contiguous array its entry point reads."""
    if len(agents) != M:
        raise ValueError(f"{who}: {scenario} is built for num_agents = {M} (got {len(agents)} agents)")
    return (_lib.CommAgent * M)(*agents)


def rollout_episode_adversary(agents, T, N, env_episode_length, env_seed, agent_pos, agent_vel, landmark_pos, goal, tstep, episode,
                              deterministic, counter, centralized):
    """The episode on the GPU-resident simple_adversary env (mappo_rollout_episode_adversary).  agents: the three comm_agent(...) of
    agents 0 (adversary), 1, 2 (good); the six env state tensors (SimpleAdversaryVecEnv) are read, stepped T times on the sampled
    indices and stored back."""
    arr = _episode_agents("rollout_episode_adversary", "simple_adversary", 3, agents)
    _env_call("mappo_rollout_episode_adversary", arr, *_ptrs((agent_pos, agent_vel, landmark_pos, goal, tstep, episode), _STATE_GOAL),
              int(T), int(N), int(env_episode_length), _u64(env_seed), int(bool(deterministic)), _u64(counter), int(bool(centralized)))


def rollout_episode_tag(agents, T, N, env_episode_length, env_seed, agent_pos, agent_vel, landmark_pos, tstep, episode, deterministic,
                        counter, centralized):
    """The episode on the GPU-resident simple_tag env (mappo_rollout_episode_tag).  agents: the four comm_agent(...) of agents 0 .. 2
    (adversaries) and 3 (good); the five env state tensors (SimpleTagVecEnv) are read, stepped T times on the sampled indices and
    stored back."""
    arr = _episode_agents("rollout_episode_tag", "simple_tag", 4, agents)
    _env_call("mappo_rollout_episode_tag", arr, *_ptrs((agent_pos, agent_vel, landmark_pos, tstep, episode), _STATE_BODIES), int(T), int(N),
              int(env_episode_length), _u64(env_seed), int(bool(deterministic)), _u64(counter), int(bool(centralized)))


def rollout_episode_world_comm(agents, T, N, env_episode_length, env_seed, agent_pos, agent_vel, landmark_pos, tstep, episode, deterministic,
                               counter, centralized):
    """The episode on the GPU-resident simple_world_comm env (mappo_rollout_episode_world_comm) — the six ACTORS only: values /
    next_values are not written, the caller runs each critic afterwards on share_obs.  agents: the six comm_agent(...) of agent 0 (the
    leader, whose actions / logp are [T, N, 2]), 1 .. 3 (adversaries) and 4, 5 (good); the five env state tensors
    (SimpleWorldCommVecEnv) are read, stepped T times on the sampled indices and stored back."""
    arr = _episode_agents("rollout_episode_world_comm", "simple_world_comm", 6, agents)
    _env_call("mappo_rollout_episode_world_comm", arr, *_ptrs((agent_pos, agent_vel, landmark_pos, tstep, episode), _STATE_BODIES), int(T),
              int(N), int(env_episode_length), _u64(env_seed), int(bool(deterministic)), _u64(counter), int(bool(centralized)))


def rollout_episode_push(agents, T, N, env_episode_length, env_seed, agent_pos, agent_vel, landmark_pos, goal, tstep, episode,
                         deterministic, counter, centralized):
    """The episode on the GPU-resident simple_push env (mappo_rollout_episode_push).  agents: the two comm_agent(...) of agents 0
    (adversary) and 1 (good); the six env state tensors (SimplePushVecEnv) are read, stepped T times on the sampled indices and stored
    back."""
    arr = _episode_agents("rollout_episode_push", "simple_push", 2, agents)
    _env_call("mappo_rollout_episode_push", arr, *_ptrs((agent_pos, agent_vel, landmark_pos, goal, tstep, episode), _STATE_GOAL), int(T),
              int(N), int(env_episode_length), _u64(env_seed), int(bool(deterministic)), _u64(counter), int(bool(centralized)))


def rollout_episode_crypto(agents, T, N, env_episode_length, env_seed, goal, key, comm, tstep, episode, deterministic, counter,
                           centralized, num_landmarks=2):
    """The episode on the GPU-resident simple_crypto env (mappo_rollout_episode_crypto).  agents: the three comm_agent(...) of agents 0
    (Eve), 1 (Bob) and 2 (Alice); the five env state tensors (SimpleCryptoVecEnv) are read, stepped T times on the sampled symbols and
    stored back."""
    arr = _episode_agents("rollout_episode_crypto", "simple_crypto", 3, agents)
    _crypto_shape("rollout_episode_crypto", 3, num_landmarks)
    _env_call("mappo_rollout_episode_crypto", arr, *_ptrs((goal, key, comm, tstep, episode), _STATE_CRYPTO), int(T), int(N),
              int(num_landmarks), int(env_episode_length), _u64(env_seed), int(bool(deterministic)), _u64(counter), int(bool(centralized)))


def mlp_backward_slabs(B):
    return int(_lib.load().mappo_mlp_backward_slabs(int(B)))


PRODUCER_MLP_BACKWARD, PRODUCER_ACTOR_UPDATE, PRODUCER_CRITIC_UPDATE, PRODUCER_TRUNK_BACKWARD = 0, 1, 2, 3


def wide_layout(desc, producer):
    """Layout id the `producer` entry point leaves in a wide workspace for `desc` (a pure function: mappo_wide_layout)."""
    v = int(_lib.load().mappo_wide_layout(C.byref(desc), int(producer)))
    if v < 0:
        _lib.check(v, "mappo_wide_layout")
    return v


def _wide(desc, x, rows, B, slabs, slab_stride, slab_col0, params, wide_ws, producer):
    """Second launch of a wide-input (in_dim > 64) backward: W1 + feature-norm gradient columns."""
    if wide_ws is not None:
        rc = _lib.load().mappo_wide_l1_backward(_ptr(params), C.byref(desc), _ptr(x), _ptr(rows, torch.int32, allow_none=True), int(B),
                                                _ptr(wide_ws), _ptr(slabs), int(slab_stride), int(slab_col0),
                                                wide_layout(desc, producer), _stream())
        _lib.check(rc, "mappo_wide_l1_backward")


_wide_ws_cache = {}


def wide_workspace(desc, B, device):
    """Scratch of the wide-input path (None for in_dim <= 64), cached per (B, device, stream): two networks' backward
    passes may run on two streams at the same time (recurrent training) and must not share it."""
    if desc.in_dim <= 64:
        return None
    key = (int(B), str(device), int(torch.cuda.current_stream().cuda_stream))
    ws = _wide_ws_cache.get(key)
    if ws is None:
        ws = torch.empty(int(_lib.load().mappo_wide_workspace_floats(int(B))), dtype=torch.float32, device=device)
        _wide_ws_cache[key] = ws
    return ws


def wide_l1_slabs(B):
    return int(_lib.load().mappo_wide_l1_slabs(int(B)))


def mlp_backward(params, desc, x, rows, B, dout, slabs, slab_stride, slab_col0):
    ws = wide_workspace(desc, B, x.device)
    rc = _lib.load().mappo_mlp_backward(_ptr(params), C.byref(desc), _ptr(x), _ptr(rows, torch.int32, allow_none=True),
                                        int(B), _ptr(dout), _ptr(slabs), int(slab_stride), int(slab_col0),
                                        _ptr(ws, allow_none=True), _stream())
    _lib.check(rc, "mappo_mlp_backward")
    _wide(desc, x, rows, B, slabs, slab_stride, slab_col0, params, ws, PRODUCER_MLP_BACKWARD)


# ---- fused update kernels ------------------------------------------------------------------------
def update_partials(device):
    return torch.zeros(int(_lib.load().mappo_update_partials_bytes()) // 8, dtype=torch.float64, device=device)


def actor_update(params, desc, obs, rows, B, avail, actions, old_logp, adv, active, mb_moments, cfg, slabs, slab_stride,
                 slab_col0, partials, n_blocks=0):
    ws = wide_workspace(desc, B, obs.device)
    rc = _lib.load().mappo_actor_update(_ptr(params), C.byref(desc), _ptr(obs), _ptr(rows, torch.int32, allow_none=True), int(B),
                                        _ptr(avail, allow_none=True), _ptr(actions), _ptr(old_logp), _ptr(adv), _ptr(active),
                                        _ptr(mb_moments, torch.float64), C.byref(cfg), _ptr(slabs), int(slab_stride),
                                        int(slab_col0), _ptr(partials, torch.float64), _ptr(ws, allow_none=True), int(n_blocks),
                                        _stream())
    _lib.check(rc, "mappo_actor_update")
    _wide(desc, obs, rows, B, slabs, slab_stride, slab_col0, params, ws, PRODUCER_ACTOR_UPDATE)


def critic_update(params, desc, share_obs, rows, B, v_old, returns, active, vn_state, mb_moments, cfg, slabs, slab_stride,
                  slab_col0, partials, n_blocks=0):
    ws = wide_workspace(desc, B, share_obs.device)
    rc = _lib.load().mappo_critic_update(_ptr(params), C.byref(desc), _ptr(share_obs), _ptr(rows, torch.int32, allow_none=True),
                                         int(B), _ptr(v_old), _ptr(returns), _ptr(active), _ptr(vn_state, allow_none=True),
                                         _ptr(mb_moments, torch.float64), C.byref(cfg), _ptr(slabs), int(slab_stride),
                                         int(slab_col0), _ptr(partials, torch.float64), _ptr(ws, allow_none=True), int(n_blocks),
                                         _stream())
    _lib.check(rc, "mappo_critic_update")
    _wide(desc, share_obs, rows, B, slabs, slab_stride, slab_col0, params, ws, PRODUCER_CRITIC_UPDATE)


def dual_update_slabs(actor_desc, critic_desc, B):
    return int(_lib.load().mappo_dual_update_slabs(C.byref(actor_desc), C.byref(critic_desc), int(B)))


def actor_critic_update(actor_params, actor_desc, obs, critic_params, critic_desc, share_obs, rows, B, avail, actions, old_logp, adv,
                        active, v_old, returns, vn_state, mb_moments, cfg, slabs, slab_stride, actor_col0, critic_col0,
                        actor_partials, critic_partials):
    """mappo_actor_update + mappo_critic_update in one launch (both in_dim <= 64): each network on half the CUs, writing
    dual_update_slabs(actor_desc, critic_desc, B) slab rows / partial rows."""
    rc = _lib.load().mappo_actor_critic_update(_ptr(actor_params), C.byref(actor_desc), _ptr(obs), _ptr(critic_params), C.byref(critic_desc),
                                               _ptr(share_obs), _ptr(rows, torch.int32, allow_none=True), int(B),
                                               _ptr(avail, allow_none=True), _ptr(actions), _ptr(old_logp), _ptr(adv), _ptr(active),
                                               _ptr(v_old), _ptr(returns), _ptr(vn_state, allow_none=True),
                                               _ptr(mb_moments, torch.float64), C.byref(cfg), _ptr(slabs), int(slab_stride),
                                               int(actor_col0), int(critic_col0), _ptr(actor_partials, torch.float64),
                                               _ptr(critic_partials, torch.float64), _stream())
    _lib.check(rc, "mappo_actor_critic_update")


def update_job(actor_params, actor_desc, obs, critic_params, critic_desc, share_obs, rows, B, avail, actions, old_logp, adv, active, v_old,
               returns, vn_state, mb_moments, cfg, slabs, slab_stride, actor_col0, critic_col0, actor_partials, critic_partials):
    """The arguments of actor_critic_update as one job of actor_critic_update_group (the tensors must outlive the launch)."""
    v = lambda p: p.value if p is not None else None
    o = lambda t: v(_ptr(t, allow_none=True))
    j = _lib.UpdateJob()
    j.actor_params, j.obs, j.critic_params, j.share_obs = v(_ptr(actor_params)), v(_ptr(obs)), v(_ptr(critic_params)), v(_ptr(share_obs))
    C.memmove(C.byref(j.actor_desc), C.byref(actor_desc), C.sizeof(NetDesc))
    C.memmove(C.byref(j.critic_desc), C.byref(critic_desc), C.sizeof(NetDesc))
    C.memmove(C.byref(j.cfg), C.byref(cfg), C.sizeof(PpoCfg))
    j.rows, j.B, j.avail = v(_ptr(rows, torch.int32, allow_none=True)), int(B), o(avail)
    j.actions, j.old_logp, j.adv, j.active = v(_ptr(actions)), v(_ptr(old_logp)), v(_ptr(adv)), v(_ptr(active))
    j.v_old, j.returns, j.vn_state, j.mb_moments = v(_ptr(v_old)), v(_ptr(returns)), o(vn_state), v(_ptr(mb_moments, torch.float64))
    j.slabs, j.slab_stride, j.actor_col0, j.critic_col0 = v(_ptr(slabs)), int(slab_stride), int(actor_col0), int(critic_col0)
    j.actor_partials, j.critic_partials = v(_ptr(actor_partials, torch.float64)), v(_ptr(critic_partials, torch.float64))
    return j


def update_group_accepts(actor_desc, critic_desc):
    """Whether actor_critic_update_group takes a job of these two networks (host-only: no device needed)."""
    return bool(_lib.load().mappo_update_group_accepts(C.byref(actor_desc), C.byref(critic_desc)))


def actor_critic_update_group(jobs):
    """len(jobs) (1..8) actor_critic_update calls in ONE launch (mappo_actor_critic_update_group): every job's slab rows and loss
    partials are bit for bit the single call's.  Narrow feed-forward Discrete jobs of one (layer_N, activation, feature norm) only."""
    arr = (_lib.UpdateJob * len(jobs))(*jobs) if jobs else None
    rc = _lib.load().mappo_actor_critic_update_group(arr, len(jobs), _stream())
    _lib.check(rc, "mappo_actor_critic_update_group")


def update_stats(actor_partials, n_actor, critic_partials, n_critic, mb_moments, cfg, stats, acc=None):
    rc = _lib.load().mappo_update_stats(_ptr(actor_partials, torch.float64, allow_none=True), int(n_actor),
                                        _ptr(critic_partials, torch.float64), int(n_critic), _ptr(mb_moments, torch.float64),
                                        C.byref(cfg), _ptr(stats, torch.float64), _ptr(acc, torch.float64, allow_none=True), _stream())
    _lib.check(rc, "mappo_update_stats")


def _copy_lists(pairs):
    n = len(pairs)
    for d, s_ in pairs:
        assert d.is_cuda and s_.is_cuda and d.dtype == torch.float32 and s_.dtype == torch.float32 and d.is_contiguous() \
            and s_.is_contiguous() and d.numel() == s_.numel()
    return (n, (C.c_void_p * n)(*[d.data_ptr() for d, _ in pairs]), (C.c_void_p * n)(*[s.data_ptr() for _, s in pairs]),
            (C.c_int64 * n)(*[d.numel() for d, _ in pairs]))


# ---- once-per-train() glue of a whole-buffer update ---------------------------------------------------
def train_prologue_workspace(n, device):
    """(workspace, ticket) of train_prologue: allocate once, the ticket zeroed; every call leaves it zero again."""
    return _ws(_lib.load().mappo_train_prologue_workspace_bytes(int(n)), device), torch.zeros(1, dtype=torch.int32, device=device)


def train_prologue(returns, value_preds, active_masks, vn_state, adv, adv_moments, mb_moments, beta, n_epochs, states_out, zero,
                   workspace, ticket):
    """adv_moments + minibatch_moments(rows=None) + valuenorm_update_n (vn_state not None) + zero.zero_() in ONE launch, bit-identical
    to them; adv_normalize follows as its own launch.  zero: contiguous float64 tensor or None."""
    rc = _lib.load().mappo_train_prologue(_ptr(returns), _ptr(value_preds), _ptr(active_masks), _ptr(vn_state, allow_none=True), _ptr(adv),
                                          _ptr(adv_moments, torch.float64), _ptr(mb_moments, torch.float64), float(beta), int(n_epochs),
                                          _ptr(states_out, allow_none=True), _ptr(zero, torch.float64, allow_none=True),
                                          zero.numel() if zero is not None else 0, _ptr(workspace, torch.uint8),
                                          _ptr(ticket, torch.int32), adv.numel(), _stream())
    _lib.check(rc, "mappo_train_prologue")


def train_epilogue(actor_partials, n_actor, critic_partials, n_critic, mb_moments, cfg, stats, acc, pairs):
    """update_stats(...) + copy_batch(pairs) in ONE launch, bit-identical to them."""
    n, dst, src, cnt = _copy_lists(pairs)
    rc = _lib.load().mappo_train_epilogue(_ptr(actor_partials, torch.float64, allow_none=True), int(n_actor),
                                          _ptr(critic_partials, torch.float64), int(n_critic), _ptr(mb_moments, torch.float64),
                                          C.byref(cfg), _ptr(stats, torch.float64), _ptr(acc, torch.float64, allow_none=True),
                                          n, dst, src, cnt, _stream())
    _lib.check(rc, "mappo_train_epilogue")


# ---- K9: recurrent layer -------------------------------------------------------------------------
def mlp_features(params, desc, x, rows, B, featT):
    rc = _lib.load().mappo_mlp_features(_ptr(params), C.byref(desc), _ptr(x), _ptr(rows, torch.int32, allow_none=True), int(B),
                                        _ptr(featT), _stream())
    _lib.check(rc, "mappo_mlp_features")


def gru_forward(params, desc, featT, h0, h0_rows, masks, rows, L, Nc, h_last=None, head_mode=0, out=None,
                avail=None, deterministic=False, seed=0, counter=0, counter_dev=None, actions=None, logp=None):
    rc = _lib.load().mappo_gru_forward(_ptr(params), C.byref(desc), _ptr(featT), _ptr(h0),
                                       _ptr(h0_rows, torch.int32, allow_none=True),
                                       _ptr(masks), _ptr(rows, torch.int32, allow_none=True), int(L), int(Nc),
                                       _ptr(h_last, allow_none=True), int(head_mode),
                                       _ptr(out, allow_none=True), _ptr(avail, allow_none=True), int(bool(deterministic)),
                                       int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1),
                                       _ptr(counter_dev, torch.int64, allow_none=True), _ptr(actions, allow_none=True),
                                       _ptr(logp, allow_none=True), _stream())
    _lib.check(rc, "mappo_gru_forward")


def gru_step_dual(actor_params, actor_desc, actor_featT, actor_h0, actor_h_last, critic_params, critic_desc, critic_featT, critic_h0,
                  critic_h_last, masks, Nc, avail, deterministic, seed, counter, counter_dev, actions, logp, values):
    """One rollout step of a recurrent actor and critic in ONE launch (mappo_gru_step_dual)."""
    rc = _lib.load().mappo_gru_step_dual(_ptr(actor_params), C.byref(actor_desc), _ptr(actor_featT), _ptr(actor_h0), _ptr(actor_h_last),
                                         _ptr(critic_params), C.byref(critic_desc), _ptr(critic_featT), _ptr(critic_h0),
                                         _ptr(critic_h_last), _ptr(masks), int(Nc), _ptr(avail, allow_none=True), int(bool(deterministic)),
                                         int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1),
                                         _ptr(counter_dev, torch.int64, allow_none=True), _ptr(actions), _ptr(logp), _ptr(values), _stream())
    _lib.check(rc, "mappo_gru_step_dual")


def recurrent_step_dual(actor_params, actor_desc, actor_obs, actor_h0, actor_h_last, critic_params, critic_desc, critic_obs, critic_h0,
                  critic_h_last, masks, Nc, avail, deterministic, seed, counter, counter_dev, actions, logp, values):
    """One rollout step of a recurrent actor and critic in ONE launch (mappo_recurrent_step_dual)."""
    rc = _lib.load().mappo_recurrent_step_dual(_ptr(actor_params), C.byref(actor_desc), _ptr(actor_obs), _ptr(actor_h0), _ptr(actor_h_last),
                                         _ptr(critic_params), C.byref(critic_desc), _ptr(critic_obs), _ptr(critic_h0),
                                         _ptr(critic_h_last), _ptr(masks), int(Nc), _ptr(avail, allow_none=True), int(bool(deterministic)),
                                         int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1),
                                         _ptr(counter_dev, torch.int64, allow_none=True), _ptr(actions), _ptr(logp), _ptr(values), _stream())
    _lib.check(rc, "mappo_recurrent_step_dual")


def mlp_features_dual(params_a, desc_a, x_a, featT_a, params_c, desc_c, x_c, featT_c, B):
    """Trunk features of two networks on the same B rows in one launch (in_dim <= 64, same layer_N / activation)."""
    rc = _lib.load().mappo_mlp_features_dual(_ptr(params_a), C.byref(desc_a), _ptr(x_a), _ptr(featT_a), _ptr(params_c), C.byref(desc_c),
                                             _ptr(x_c), _ptr(featT_c), int(B), _stream())
    _lib.check(rc, "mappo_mlp_features_dual")


def trunk_backward(params, desc, x, rows, B, dxT, slabs, slab_stride, slab_col0):
    ws = wide_workspace(desc, B, x.device)
    rc = _lib.load().mappo_trunk_backward(_ptr(params), C.byref(desc), _ptr(x), _ptr(rows, torch.int32, allow_none=True), int(B),
                                          _ptr(dxT), _ptr(slabs), int(slab_stride), int(slab_col0), _ptr(ws, allow_none=True), _stream())
    _lib.check(rc, "mappo_trunk_backward")
    _wide(desc, x, rows, B, slabs, slab_stride, slab_col0, params, ws, PRODUCER_TRUNK_BACKWARD)


# ---- K9 training pass on 16-sequence tiles (gru_train16.hip) ---------------------------------------
def gru16_scratch_floats(L, Nc):
    return int(_lib.load().mappo_gru16_scratch_floats(int(L), int(Nc)))


def gru16_blocked_floats(L, Nc):
    return int(_lib.load().mappo_gru16_blocked_floats(int(L), int(Nc)))


def gru16_slabs(L, Nc):
    return int(_lib.load().mappo_gru16_slabs(int(L), int(Nc)))


def mlp_features_seq(params, desc, x, rows, L, Nc, out_blocked):
    rc = _lib.load().mappo_mlp_features_seq(_ptr(params), C.byref(desc), _ptr(x), _ptr(rows, torch.int32, allow_none=True), int(L), int(Nc),
                                            _ptr(out_blocked), _stream())
    _lib.check(rc, "mappo_mlp_features_seq")


def gru16_forward_loss(params, desc, x, x_blocked, h0, h0_rows, masks, rows, L, Nc, head, avail, actions, old_logp, adv, active, v_old,
                       returns, vn_state, mb_moments, cfg, scratch, slabs, slab_stride, slab_col0, partials):
    o = lambda t: _ptr(t, allow_none=True)
    rc = _lib.load().mappo_gru16_forward_loss(_ptr(params), C.byref(desc), _ptr(x), int(bool(x_blocked)), _ptr(h0),
                                              _ptr(h0_rows, torch.int32, allow_none=True), _ptr(masks),
                                              _ptr(rows, torch.int32, allow_none=True), int(L), int(Nc), int(head), o(avail), o(actions),
                                              o(old_logp), o(adv), _ptr(active), o(v_old), o(returns), o(vn_state),
                                              _ptr(mb_moments, torch.float64), C.byref(cfg), _ptr(scratch), _ptr(slabs), int(slab_stride),
                                              int(slab_col0), _ptr(partials, torch.float64), _stream())
    _lib.check(rc, "mappo_gru16_forward_loss")


def gru16_backward(params, desc, masks, rows, L, Nc, scratch, dxT=None):
    rc = _lib.load().mappo_gru16_backward(_ptr(params), C.byref(desc), _ptr(masks), _ptr(rows, torch.int32, allow_none=True), int(L), int(Nc),
                                          _ptr(scratch), _ptr(dxT, allow_none=True), _stream())
    _lib.check(rc, "mappo_gru16_backward")


def gru16_wgrad(desc, x, x_blocked, scratch, L, Nc, slabs, slab_stride, slab_col0):
    rc = _lib.load().mappo_gru16_wgrad(C.byref(desc), _ptr(x), int(bool(x_blocked)), _ptr(scratch), int(L), int(Nc), _ptr(slabs),
                                       int(slab_stride), int(slab_col0), _stream())
    _lib.check(rc, "mappo_gru16_wgrad")


def trunk_backward_seq(params, desc, x, rows, L, Nc, dx_blocked, slabs, slab_stride, slab_col0):
    ws = wide_workspace(desc, L * Nc, x.device)
    rc = _lib.load().mappo_trunk_backward_seq(_ptr(params), C.byref(desc), _ptr(x), _ptr(rows, torch.int32, allow_none=True), int(L), int(Nc),
                                              _ptr(dx_blocked), _ptr(slabs), int(slab_stride), int(slab_col0), _ptr(ws, allow_none=True),
                                              _stream())
    _lib.check(rc, "mappo_trunk_backward_seq")
    _wide(desc, x, rows, L * Nc, slabs, slab_stride, slab_col0, params, ws, PRODUCER_TRUNK_BACKWARD)


# ---- K10 / K11 ------------------------------------------------------------------------------------
def slab_reduce(slabs, n_slabs, slab_stride, P, grad):
    rc = _lib.load().mappo_slab_reduce(_ptr(slabs), int(n_slabs), int(slab_stride), int(P), _ptr(grad), _stream())
    _lib.check(rc, "mappo_slab_reduce")


def optim_workspace(P, device):
    return _ws(_lib.load().mappo_optim_workspace_bytes(int(P)), device)


def clip_adam(params, grad, exp_avg, exp_avg_sq, seg_bounds, opt_hyper, opt_step, grad_norms, workspace, norm_acc=None):
    n_seg = len(seg_bounds) - 1
    arr = (C.c_int64 * (n_seg + 1))(*[int(b) for b in seg_bounds])
    rc = _lib.load().mappo_clip_adam(_ptr(params), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), arr, n_seg,
                                     _ptr(opt_hyper), _ptr(opt_step, torch.int32), _ptr(grad_norms),
                                     _ptr(norm_acc, torch.float64, allow_none=True), _ptr(workspace, torch.uint8), _stream())
    _lib.check(rc, "mappo_clip_adam")


def reduce_clip_adam(slabs, n_slabs, slab_stride, params, grad, exp_avg, exp_avg_sq, seg_bounds, opt_hyper, opt_step, grad_norms,
                     workspace, norm_acc=None):
    """slab_reduce + clip_adam in two launches (single-process training)."""
    n_seg = len(seg_bounds) - 1
    arr = (C.c_int64 * (n_seg + 1))(*[int(b) for b in seg_bounds])
    rc = _lib.load().mappo_reduce_clip_adam(_ptr(slabs), int(n_slabs), int(slab_stride), _ptr(params), _ptr(grad), _ptr(exp_avg),
                                            _ptr(exp_avg_sq), arr, n_seg, _ptr(opt_hyper), _ptr(opt_step, torch.int32), _ptr(grad_norms),
                                            _ptr(norm_acc, torch.float64, allow_none=True), _ptr(workspace, torch.uint8), _stream())
    _lib.check(rc, "mappo_reduce_clip_adam")


def optim_job(slabs, n_slabs, slab_stride, params, grad, exp_avg, exp_avg_sq, seg_bounds, opt_hyper, opt_step, grad_norms, workspace,
              norm_acc=None):
    """The arguments of reduce_clip_adam as one job of reduce_clip_adam_group."""
    v = lambda p: p.value if p is not None else None
    j = _lib.OptimJob()
    j.slabs, j.n_slabs, j.slab_stride = v(_ptr(slabs)), int(n_slabs), int(slab_stride)
    j.params, j.grad, j.exp_avg, j.exp_avg_sq = v(_ptr(params)), v(_ptr(grad)), v(_ptr(exp_avg)), v(_ptr(exp_avg_sq))
    n_seg = len(seg_bounds) - 1
    if not 1 <= n_seg <= 4:
        raise ValueError(f"optim_job: {n_seg} segments (1..4)")
    for s, b in enumerate(seg_bounds):
        j.seg_bounds[s] = int(b)
    j.n_seg = n_seg
    j.opt_hyper, j.opt_step, j.grad_norms = v(_ptr(opt_hyper)), v(_ptr(opt_step, torch.int32)), v(_ptr(grad_norms))
    j.norm_acc, j.workspace = v(_ptr(norm_acc, torch.float64, allow_none=True)), v(_ptr(workspace, torch.uint8))
    return j


def reduce_clip_adam_group(jobs):
    """len(jobs) (1..8) reduce_clip_adam calls in the same two launches (mappo_reduce_clip_adam_group), bit-identical per job."""
    arr = (_lib.OptimJob * len(jobs))(*jobs) if jobs else None
    rc = _lib.load().mappo_reduce_clip_adam_group(arr, len(jobs), _stream())
    _lib.check(rc, "mappo_reduce_clip_adam_group")


def selftest_mfma(A, Bm, D):
    rc = _lib.load().mappo_selftest_mfma(_ptr(A), _ptr(Bm), _ptr(D), _stream())
    _lib.check(rc, "mappo_selftest_mfma")


# ---- measurement hook -----------------------------------------------------------------------------
PROF_IDS = dict(gae=0, ppo_loss=1, mlp_fwd=2, mlp_bwd=3, slab_reduce=4, adam=5, act=6, wide_l1=7)


def profile_arm(kernel, start_event, stop_event):
    """Bracket the next launch of `kernel`'s dominant HIP kernel with two torch.cuda.Event(enable_timing=True)
    (recorded by the C side on the stream that launch uses).  One-shot."""
    for ev in (start_event, stop_event):
        if ev.cuda_event == 0:                 # torch creates the hipEvent lazily on first record
            ev.record()
    rc = _lib.load().mappo_profile_arm(PROF_IDS[kernel], C.c_void_p(start_event.cuda_event), C.c_void_p(stop_event.cuda_event))
    _lib.check(rc, "mappo_profile_arm")


# ---- GPU-vectorised MPE envs: reset (state..., obs..., N, [shape...], seed) and step (state..., actions, mode, obs..., rewards, dones, N,
# [shape...], episode_length, seed), one launch each ----
# simple_spread (csrc/mpe_env.hip)
def mpe_spread_reset(agent_pos, agent_vel, landmark_pos, tstep, episode, obs, N, M, L, seed):
    _env_call("mappo_mpe_spread_reset", *_ptrs((agent_pos, agent_vel, landmark_pos, tstep, episode), _STATE_BODIES), _ptr(obs), int(N), int(M),
              int(L), _u64(seed))


def mpe_spread_step(agent_pos, agent_vel, landmark_pos, tstep, episode, actions, action_mode, obs, rewards, dones, N, M, L,
                    episode_length, seed):
    _env_call("mappo_mpe_spread_step", *_ptrs((agent_pos, agent_vel, landmark_pos, tstep, episode), _STATE_BODIES), _ptr(actions),
              int(action_mode), _ptr(obs), _ptr(rewards), _ptr(dones, torch.uint8), int(N), int(M), int(L), int(episode_length), _u64(seed))


# simple_reference (csrc/mpe_ref_env.hip): 2 agents, 3 landmarks, MultiDiscrete (5, 10)
def mpe_reference_reset(agent_pos, agent_vel, landmark_pos, goal, tstep, episode, obs, N, seed):
    _env_call("mappo_mpe_reference_reset", *_ptrs((agent_pos, agent_vel, landmark_pos, goal, tstep, episode), _STATE_GOAL), _ptr(obs), int(N),
              _u64(seed))


def mpe_reference_step(agent_pos, agent_vel, landmark_pos, goal, tstep, episode, actions, action_mode, obs, rewards, dones, N,
                       episode_length, seed):
    """action_mode 0: actions [N, 2, 15] (the heads' one-hots side by side) | 1: [N, 2, 2] fp32 head indices."""
    _env_call("mappo_mpe_reference_step", *_ptrs((agent_pos, agent_vel, landmark_pos, goal, tstep, episode), _STATE_GOAL), _ptr(actions),
              int(action_mode), _ptr(obs), _ptr(rewards), _ptr(dones, torch.uint8), int(N), int(episode_length), _u64(seed))


# simple_speaker_listener (csrc/mpe_comm_env.hip): speaker Discrete(3), listener Discrete(5)
def mpe_comm_reset(listener_pos, listener_vel, landmark_pos, goal, symbol, tstep, episode, obs_speaker, obs_listener, N, seed):
    _env_call("mappo_mpe_comm_reset", *_ptrs((listener_pos, listener_vel, landmark_pos, goal, symbol, tstep, episode), _STATE_COMM),
              _ptr(obs_speaker), _ptr(obs_listener), int(N), _u64(seed))


def mpe_comm_step(listener_pos, listener_vel, landmark_pos, goal, symbol, tstep, episode, actions_speaker, actions_listener, action_mode,
                  obs_speaker, obs_listener, rewards, dones, N, episode_length, seed):
    """action_mode 0: one-hots, actions_speaker [N, 3] and actions_listener [N, 5] | 1: actions_speaker = fp32 indices [N, 2]
    (symbol, move), actions_listener None."""
    _env_call("mappo_mpe_comm_step", *_ptrs((listener_pos, listener_vel, landmark_pos, goal, symbol, tstep, episode), _STATE_COMM),
              _ptr(actions_speaker), _ptr(actions_listener, allow_none=True), int(action_mode), _ptr(obs_speaker), _ptr(obs_listener),
              _ptr(rewards), _ptr(dones, torch.uint8), int(N), int(episode_length), _u64(seed))


# The scenarios below pay every agent its OWN reward and share their kernels (csrc/mpe_ragged_env.hip over each scenario's
# mpe_<scenario>_core.h): rewards [N, M], one per agent.
# simple_adversary: adversary + two good agents, Discrete(5) each
def mpe_adversary_reset(agent_pos, agent_vel, landmark_pos, goal, tstep, episode, obs_adversary, obs_good1, obs_good2, N, seed, num_agents=3):
    _env_call("mappo_mpe_adversary_reset", *_ptrs((agent_pos, agent_vel, landmark_pos, goal, tstep, episode), _STATE_GOAL),
              *map(_ptr, (obs_adversary, obs_good1, obs_good2)), int(N), int(num_agents), _u64(seed))


def mpe_adversary_step(agent_pos, agent_vel, landmark_pos, goal, tstep, episode, actions, action_mode, obs_adversary, obs_good1, obs_good2,
                       rewards, dones, N, episode_length, seed, num_agents=3):
    """action_mode 0: one-hots [N, 3, 5] | 1: fp32 indices [N, 3]."""
    _env_call("mappo_mpe_adversary_step", *_ptrs((agent_pos, agent_vel, landmark_pos, goal, tstep, episode), _STATE_GOAL), _ptr(actions),
              int(action_mode), *map(_ptr, (obs_adversary, obs_good1, obs_good2, rewards)), _ptr(dones, torch.uint8), int(N), int(num_agents),
              int(episode_length), _u64(seed))


# simple_tag: three adversaries + one good agent, Discrete(5) each
def _tag_agents(who, num_agents):
    if int(num_agents) != 4:
        raise ValueError(f"{who}: simple_tag is built for num_agents = 4: 3 adversaries, 1 good agent, 2 landmarks (got {num_agents})")


def mpe_tag_reset(agent_pos, agent_vel, landmark_pos, tstep, episode, obs_adv0, obs_adv1, obs_adv2, obs_good, N, seed, num_agents=4):
    _tag_agents("mpe_tag_reset", num_agents)
    _env_call("mappo_mpe_tag_reset", *_ptrs((agent_pos, agent_vel, landmark_pos, tstep, episode), _STATE_BODIES),
              *map(_ptr, (obs_adv0, obs_adv1, obs_adv2, obs_good)), int(N), int(num_agents), _u64(seed))


def mpe_tag_step(agent_pos, agent_vel, landmark_pos, tstep, episode, actions, action_mode, obs_adv0, obs_adv1, obs_adv2, obs_good, rewards,
                 dones, N, episode_length, seed, num_agents=4):
    """action_mode 0: one-hots [N, 4, 5] | 1: fp32 indices [N, 4]."""
    _tag_agents("mpe_tag_step", num_agents)
    _env_call("mappo_mpe_tag_step", *_ptrs((agent_pos, agent_vel, landmark_pos, tstep, episode), _STATE_BODIES), _ptr(actions), int(action_mode),
              *map(_ptr, (obs_adv0, obs_adv1, obs_adv2, obs_good, rewards)), _ptr(dones, torch.uint8), int(N), int(num_agents),
              int(episode_length), _u64(seed))


# simple_push: one adversary + one good agent that collide, Discrete(5) each
def _push_agents(who, num_agents):
    if int(num_agents) != 2:
        raise ValueError(f"{who}: simple_push is built for num_agents = 2: 1 adversary, 1 good agent, 2 landmarks (got {num_agents})")


def mpe_push_reset(agent_pos, agent_vel, landmark_pos, goal, tstep, episode, obs_adversary, obs_good, N, seed, num_agents=2):
    _push_agents("mpe_push_reset", num_agents)
    _env_call("mappo_mpe_push_reset", *_ptrs((agent_pos, agent_vel, landmark_pos, goal, tstep, episode), _STATE_GOAL), _ptr(obs_adversary),
              _ptr(obs_good), int(N), int(num_agents), _u64(seed))


def mpe_push_step(agent_pos, agent_vel, landmark_pos, goal, tstep, episode, actions, action_mode, obs_adversary, obs_good, rewards, dones, N,
                  episode_length, seed, num_agents=2):
    """action_mode 0: one-hots [N, 2, 5] | 1: fp32 indices [N, 2]."""
    _push_agents("mpe_push_step", num_agents)
    _env_call("mappo_mpe_push_step", *_ptrs((agent_pos, agent_vel, landmark_pos, goal, tstep, episode), _STATE_GOAL), _ptr(actions),
              int(action_mode), _ptr(obs_adversary), _ptr(obs_good), _ptr(rewards), _ptr(dones, torch.uint8), int(N), int(num_agents),
              int(episode_length), _u64(seed))


# simple_crypto: Eve, Bob and Alice only speak, Discrete(4) each
def _crypto_shape(who, num_agents, num_landmarks):
    if int(num_agents) != 3:
        raise ValueError(f"{who}: simple_crypto is built for num_agents = 3: adversary Eve, listener Bob, speaker Alice (got {num_agents})")
    if not 2 <= int(num_landmarks) <= 4:
        raise ValueError(f"{who}: simple_crypto takes num_landmarks = 2, 3 or 4, a landmark's colour being a one-hot of dim_c = 4 "
                         f"(got {num_landmarks})")


def mpe_crypto_reset(goal, key, comm, tstep, episode, obs_eve, obs_bob, obs_alice, N, seed, num_agents=3, num_landmarks=2):
    _crypto_shape("mpe_crypto_reset", num_agents, num_landmarks)
    _env_call("mappo_mpe_crypto_reset", *_ptrs((goal, key, comm, tstep, episode), _STATE_CRYPTO), *map(_ptr, (obs_eve, obs_bob, obs_alice)),
              int(N), int(num_agents), int(num_landmarks), _u64(seed))


def mpe_crypto_step(goal, key, comm, tstep, episode, actions, action_mode, obs_eve, obs_bob, obs_alice, rewards, dones, N, episode_length,
                    seed, num_agents=3, num_landmarks=2):
    """action_mode 0: one-hots [N, 3, 4] | 1: fp32 indices [N, 3]."""
    _crypto_shape("mpe_crypto_step", num_agents, num_landmarks)
    _env_call("mappo_mpe_crypto_step", *_ptrs((goal, key, comm, tstep, episode), _STATE_CRYPTO), _ptr(actions), int(action_mode),
              *map(_ptr, (obs_eve, obs_bob, obs_alice, rewards)), _ptr(dones, torch.uint8), int(N), int(num_agents), int(num_landmarks),
              int(episode_length), _u64(seed))


# simple_world_comm (its own kernels, csrc/mpe_world_comm_env.hip): four adversaries, the first a MultiDiscrete (5, 4) leader, + two
# good agents, Discrete(5) each
def _world_comm_shape(who, num_agents, num_adversaries, num_good_agents, num_landmarks):
    if (int(num_agents), int(num_adversaries), int(num_good_agents), int(num_landmarks)) != (6, 4, 2, 1):
        raise ValueError(f"{who}: simple_world_comm is built for num_agents = 6: 4 adversaries (the first their leader), 2 good agents, "
                         f"1 landmark (got num_agents {num_agents}, num_adversaries {num_adversaries}, num_good_agents {num_good_agents}, "
                         f"num_landmarks {num_landmarks})")


def _ptr_array(tensors, n, what, allow_none=False):
    """A host array of n device pointers (fp32 tensors; None -> NULL where allowed)."""
    if len(tensors) != n:
        raise ValueError(f"{what}: {len(tensors)} tensors, needs {n}")
    ptrs = [_ptr(t, allow_none=allow_none) for t in tensors]
    return (C.c_void_p * n)(*[None if q is None else q.value for q in ptrs])


def mpe_world_comm_reset(agent_pos, agent_vel, landmark_pos, tstep, episode, obs, N, seed, num_agents=6, num_adversaries=4,
                         num_good_agents=2, num_landmarks=1):
    """obs: the six per-agent output tensors, [N, 34] x 4 then [N, 28] x 2."""
    _world_comm_shape("mpe_world_comm_reset", num_agents, num_adversaries, num_good_agents, num_landmarks)
    _env_call("mappo_mpe_world_comm_reset", *_ptrs((agent_pos, agent_vel, landmark_pos, tstep, episode), _STATE_BODIES),
              _ptr_array(list(obs), 6, "mpe_world_comm_reset: obs"), int(N), int(num_agents), int(num_landmarks), _u64(seed))


def mpe_world_comm_step(agent_pos, agent_vel, landmark_pos, tstep, episode, actions, action_mode, obs, rewards, dones, N, episode_length, seed,
                        num_agents=6, num_adversaries=4, num_good_agents=2, num_landmarks=1):
    """action_mode 0: actions = the six one-hot tensors, [N, 9] of the leader (move | word) and [N, 5] x 5 | 1: actions = one tensor of
    fp32 indices [N, 7]: leader move, leader word, agents 1..5.  obs as in mpe_world_comm_reset."""
    _world_comm_shape("mpe_world_comm_step", num_agents, num_adversaries, num_good_agents, num_landmarks)
    acts = list(actions) if int(action_mode) == 0 else [actions] + [None] * 5
    if acts[0] is None:
        raise ValueError("tensor required")
    _env_call("mappo_mpe_world_comm_step", *_ptrs((agent_pos, agent_vel, landmark_pos, tstep, episode), _STATE_BODIES),
              _ptr_array(acts, 6, "mpe_world_comm_step: actions", allow_none=int(action_mode) != 0), int(action_mode),
              _ptr_array(list(obs), 6, "mpe_world_comm_step: obs"), _ptr(rewards), _ptr(dones, torch.uint8), int(N), int(num_agents),
              int(num_landmarks), int(episode_length), _u64(seed))


def synth_smac_pool(obs, share_obs, avail, rewards, dead, dones, p_death, p_term, seed, counter):
    """P steps of the synthetic SMAC-shaped env in one launch: pools obs [P, N, M, D], share_obs, avail, rewards [P, N], dones [P, N, M]."""
    P, N, M, D = obs.shape
    assert counter.numel() == 34
    rc = _lib.load().mappo_synth_smac_pool(_ptr(obs), _ptr(share_obs), _ptr(avail), _ptr(rewards), _ptr(dead, torch.bool), _ptr(dones, torch.bool),
                                           int(P), int(N), int(M), int(D), int(share_obs.shape[3]), int(avail.shape[3]), float(p_death),
                                           float(p_term), int(seed), _ptr(counter, torch.int64), _stream())
    _lib.check(rc, "mappo_synth_smac_pool")


def synth_smac_step(obs, share_obs, avail, rewards, dead, dones, p_death, p_term, seed, counter):
    """One step of the synthetic SMAC-shaped env (bench utility, csrc/synth_env.hip); `counter`: int64 [34] device tensor
    {Philox counter, 33 tickets (0)}: the launch advances the counter itself."""
    assert counter.numel() == 34
    N, M, D = obs.shape
    rc = _lib.load().mappo_synth_smac_step(_ptr(obs), _ptr(share_obs), _ptr(avail), _ptr(rewards), _ptr(dead, torch.bool), _ptr(dones, torch.bool),
                                           int(N), int(M), int(D), int(share_obs.shape[2]), int(avail.shape[2]), float(p_death), float(p_term),
                                           int(seed), _ptr(counter, torch.int64), _stream())
    _lib.check(rc, "mappo_synth_smac_step")
