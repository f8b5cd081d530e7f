"""CPU: the oracle (oracle/mappo_oracle.py) against the golden vectors produced by the reference."""
import numpy as np
import pytest
import torch

from conftest import golden, sub
from oracle import mappo_oracle as O

RTOL = 1e-5   # north_star: 1e-5 relative on fp32 returns / losses


def close(a, b, rtol=RTOL, atol=1e-6):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=rtol, atol=atol)


def args_from(**kw):
    return O.default_args(**kw)


def load_net(net, npz, prefix):
    sd = {k: torch.from_numpy(np.array(v)) for k, v in sub(npz, prefix).items()}
    net.load_state_dict(sd, strict=True)
    return net


def test_valuenorm():
    g = golden("valuenorm")
    vn = O.ValueNormRef()
    for i in range(4):
        vn.update(g[f"x{i}"])
        np.testing.assert_array_equal(vn.state(), g[f"state{i}"])
        close(vn.normalize(g[f"x{i}"]).numpy(), g[f"norm{i}"], 1e-6)
        close(vn.denormalize(g[f"x{i}"]), g[f"denorm{i}"], 1e-6)


def test_compute_returns_all_branches():
    g = golden("gae")
    for c in range(int(g["n_cases"])):
        d = sub(g, f"c{c}")
        use_gae, ptl, use_vn = [bool(x) for x in d["flags"]]
        vn = None
        if use_vn:
            vn = O.ValueNormRef(); vn.load_state(d["vn_state"])
        vp = d["value_preds"].copy()
        ret = O.compute_returns_ref(d["rewards"], vp, d["masks"], d["bad_masks"], d["next_value"],
                                    float(d["hyper"][0]), float(d["hyper"][1]), use_gae, ptl,
                                    vn.denormalize if vn else None)
        close(ret, d["returns"], 1e-6)
        np.testing.assert_array_equal(vp, d["value_preds_after"])


def test_advantage_normalisation():
    g = golden("advnorm")
    for c in range(int(g["n_cases"])):
        d = sub(g, f"c{c}")
        vn = None
        if bool(d["use_vn"]):
            vn = O.ValueNormRef(); vn.load_state(d["vn_state"])
        adv, mean, std = O.normalized_advantages_ref(d["returns"], d["value_preds"], d["active_masks"],
                                                     vn.denormalize if vn else None)
        close(adv, d["adv"], 1e-6)
        close(mean, d["mean"]); close(std, d["std"])


TUPLE = ("share_obs", "obs", "rnn_states", "rnn_states_critic", "actions", "value_preds", "returns",
         "masks", "active_masks", "old_action_log_probs", "adv_targ", "available_actions")


def _buffer_from(d, T, N, M, hidden):
    a = args_from(episode_length=T, n_rollout_threads=N, hidden_size=hidden)
    buf = O.BufferRef(a, M, d["buf/obs"].shape[-1], d["buf/share_obs"].shape[-1], d["buf/available_actions"].shape[-1])
    for k in ("share_obs", "obs", "rnn_states", "rnn_states_critic", "value_preds", "returns", "available_actions",
              "actions", "action_log_probs", "rewards", "masks", "bad_masks", "active_masks"):
        getattr(buf, k)[...] = d["buf/" + k]
    return buf


def test_generators_bit_exact():
    g = golden("generators")
    for c in range(int(g["n_cases"])):
        d = sub(g, f"c{c}")
        kind, T, N, M, nmb, L, seed = [int(x) for x in d["spec"]]
        buf = _buffer_from(d, T, N, M, d["buf/rnn_states"].shape[-1])
        R = N * M
        torch.manual_seed(seed)                      # same torch => same permutation stream as the reference
        if kind == 0:
            rand = torch.randperm(T * R).numpy()
            batches = [(rows, None) for rows in O.feed_forward_rows(T, R, nmb, rand)]
        elif kind == 1:
            rand = torch.randperm((T * R) // L).numpy()
            batches = O.recurrent_rows(T, R, nmb, L, rand)
        else:
            rand = torch.randperm(R).numpy()
            batches = O.naive_recurrent_rows(T, R, nmb, rand)
        np.testing.assert_array_equal(rand, d["rand"])          # indices: bit-exact
        assert len(batches) == int(d["n_batches"])
        for bi, (rows, h0) in enumerate(batches):
            sample = buf.sample(rows, d["adv"], h0)
            for nm, arr in zip(TUPLE, sample):
                np.testing.assert_array_equal(arr, d[f"b{bi}/{nm}"], err_msg=f"case {c} batch {bi} {nm}")


def test_insert_after_update():
    g = golden("insert")
    T, N, M = 4, 2, 3
    a = args_from(episode_length=T, n_rollout_threads=N, hidden_size=8)
    buf = O.BufferRef(a, M, 6, 18, 5)
    names = ("share_obs", "obs", "rnn_states", "rnn_states_critic", "value_preds", "returns", "available_actions",
             "actions", "action_log_probs", "rewards", "masks", "bad_masks", "active_masks")
    for s in range(int(g["n_inserts"])):
        d = sub(g, f"in{s}")
        buf.insert(d["share_obs"], d["obs"], d["rnn_a"], d["rnn_c"], d["actions"], d["logp"], d["values"],
                   d["rewards"], d["masks"], d["bad"], d["active"], d["avail"])
        assert buf.step == int(g[f"step_after{s}"])
        if s == T - 1:
            for n in names:
                np.testing.assert_array_equal(getattr(buf, n), g["full/" + n])
            buf.after_update()
            for n in names:
                np.testing.assert_array_equal(getattr(buf, n), g["after_update/" + n])
    for n in names:
        np.testing.assert_array_equal(getattr(buf, n), g["final/" + n])


def test_insert_ref_matches_golden_slots():
    """tests/insert_ref.py, the NumPy reference of test_gpu_insert_matrix.py, against the buffer the reference filled: every
    insert of golden/insert.npz (the step wraps after T) lands in the slot the reference wrote, with the reference's values.
    The fixture's masks are drawn per agent, so they pin insert_mpe_ref's mask (dones := masks == 0) and state reset; its
    share_obs, available_actions and bad_masks pin insert_smac_ref's copies and bad mask."""
    from insert_ref import episode_insert_ref, insert_mpe_ref, insert_smac_ref
    g = golden("insert")
    T, N, M = 4, 2, 3
    assert int(g["n_inserts"]) == T + 2
    steps = []
    for s in range(T + 2):
        d = sub(g, f"in{s}")
        step, snap = s % T, ("full/" if s < T else "final/")
        dones = d["masks"][..., 0] == 0
        rnn = (d["rnn_a"].reshape(N * M, 1, 8), d["rnn_c"].reshape(N * M, 1, 8))
        obs, share, rew, mask, ha, hc = insert_mpe_ref(d["obs"], d["rewards"], dones, False, rnn)
        np.testing.assert_array_equal(obs, g[snap + "obs"][step + 1])
        np.testing.assert_array_equal(share, g[snap + "obs"][step + 1])
        np.testing.assert_array_equal(rew, g[snap + "rewards"][step])
        np.testing.assert_array_equal(mask, g[snap + "masks"][step + 1])
        for got, name in ((ha, "rnn_states"), (hc, "rnn_states_critic")):
            want = g[snap + name][step + 1].reshape(N * M, 1, 8)
            keep = ~dones.reshape(N * M)
            np.testing.assert_array_equal(got[keep], want[keep])
            assert (got[~keep] == 0).all() and (want[~keep] != 0).all()
        cen = insert_mpe_ref(d["obs"], d["rewards"][..., 0], dones, True)
        assert cen[1].shape == (N, M, M * 6)
        for m in range(M):
            np.testing.assert_array_equal(cen[1][:, m], g[snap + "obs"][step + 1].reshape(N, M * 6))
        for a, b in zip(cen[:1] + cen[2:], (obs, rew, mask)):
            np.testing.assert_array_equal(a, b)
        out = insert_smac_ref(d["obs"], d["share_obs"], d["avail"], d["rewards"], np.zeros((N, M), dtype=bool), d["bad"][..., 0] == 0, rnn)
        names = ("obs", "share_obs", "available_actions", "rewards", "masks", "bad_masks", "active_masks", "rnn_states", "rnn_states_critic")
        for got, name in zip(out, names):
            lo = step if name == "rewards" else step + 1
            want = np.ones((N, M, 1), np.float32) if name in ("masks", "active_masks") else g[snap + name][lo]
            np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=name)
        if s < T:
            steps.append((d["obs"], d["rewards"], dones))
    ep = episode_insert_ref(*(np.stack(x) for x in zip(*steps)), False)
    for got, name, lo in zip(ep, ("obs", "obs", "rewards", "masks"), (1, 1, 0, 1)):
        np.testing.assert_array_equal(got, g["full/" + name][lo:lo + T])


def test_forward_paths():
    g = golden("forward")
    t = torch.from_numpy
    for c in range(int(g["n_cases"])):
        d = sub(g, f"c{c}")
        relu, rec, D, S, A, B, H = [int(x) for x in d["spec"]]
        a = args_from(use_ReLU=bool(relu), use_recurrent_policy=bool(rec), hidden_size=H)
        actor = load_net(O.ActorRef(a, D, A), g, f"c{c}/actor")
        critic = load_net(O.CriticRef(a, S), g, f"c{c}/critic")
        with torch.no_grad():
            for tag in ("avail", "noavail"):
                av = t(d["avail"]) if tag == "avail" else None
                act, lp, ra = actor(t(d["obs"]), t(d["rnn_a"]), t(d["masks"]), av, deterministic=True)
                v, rc = critic(t(d["share_obs"]), t(d["rnn_c"]), t(d["masks"]))
                np.testing.assert_array_equal(act.numpy(), d[f"{tag}/actions"])
                close(lp.numpy(), d[f"{tag}/logp"]); close(v.numpy(), d[f"{tag}/values"])
                close(v.numpy(), d[f"{tag}/get_values"])
                if rec:
                    close(ra.numpy(), d[f"{tag}/rnn_a"]); close(rc.numpy(), d[f"{tag}/rnn_c"])
                elp, ent, _ = actor.evaluate_actions(t(d["obs"]), t(d["rnn_a"]), t(d[f"{tag}/actions"].astype(np.float32)),
                                                     t(d["masks"]), av, t(d[f"{tag}/active"]))
                close(elp.numpy(), d[f"{tag}/eval_logp"]); close(ent.item(), d[f"{tag}/eval_entropy"])
            if rec:
                elp, ent, _ = actor.evaluate_actions(t(d["seq/obs"]), t(d["seq/h0a"]), t(d["seq/actions"]), t(d["seq/masks"]),
                                                     t(d["seq/avail"]), t(d["seq/active"]))
                v, _ = critic(t(d["seq/share_obs"]), t(d["seq/h0c"]), t(d["seq/masks"]))
                close(elp.numpy(), d["seq/logp"]); close(v.numpy(), d["seq/values"]); close(ent.item(), d["seq/entropy"])


def _policy_from(g, c, prefix0=("actor0", "critic0")):
    d = sub(g, f"c{c}")
    T, N, M, D, S, A, H = [int(x) for x in d["dims"][:7]]
    return d, (T, N, M, D, S, A, H)


def test_ppo_update_all_variants():
    g = golden("ppo_update")
    for c in range(int(g["n_cases"])):
        d, (T, N, M, D, S, A, H) = _policy_from(g, c)
        fl = dict(zip([str(x) for x in d["flag_names"]], [bool(x) for x in d["flags"]]))
        hy = d["hyper"]
        a = args_from(episode_length=T, n_rollout_threads=N, hidden_size=H, clip_param=float(hy[0]),
                      entropy_coef=float(hy[1]), value_loss_coef=float(hy[2]), huber_delta=float(hy[3]),
                      max_grad_norm=float(hy[4]), lr=float(hy[5]), critic_lr=float(hy[6]), opti_eps=float(hy[7]),
                      weight_decay=float(hy[8]), data_chunk_length=int(hy[9]),
                      **{k: v for k, v in fl.items() if k not in ("update_actor", "two_steps")})
        pol = O.PolicyRef(a, D, S, A)
        load_net(pol.actor, g, f"c{c}/actor0"); load_net(pol.critic, g, f"c{c}/critic0")
        vn = None
        if a.use_valuenorm:
            vn = O.ValueNormRef(); vn.load_state(d["vn0"])
        sample = tuple(d[f"sample/{nm}"] for nm in TUPLE)
        for rep in range(2 if fl["two_steps"] else 1):
            vl, cn, pl, ent, an, imp = O.ppo_update_ref(a, pol, vn, sample, fl["update_actor"])
            close([vl, cn, pl, ent, an, float(imp.mean())], d[f"r{rep}/stats"], 2e-5)
            close(imp.numpy(), d[f"r{rep}/imp"])
            for tag, net in (("actor", pol.actor), ("critic", pol.critic)):
                ref_sd = sub(g, f"c{c}/r{rep}/{tag}")
                # post-Adam parameters: the first Adam steps move a weight by lr*g/(|g|+eps); where |g| ~ eps an
                # fp32 re-association of g (per-step GRU here vs torch's fused GRU in the reference) shifts the step
                # by up to ~0.3 % of lr, hence the absolute floor of 3e-6 (lr = 7e-4).
                for k, v in net.state_dict().items():
                    close(v.numpy(), ref_sd[k], 1e-5, 3e-6)
                for n_, p_ in net.named_parameters():
                    key = f"r{rep}/{tag}_grad/{n_}"
                    if key in d:
                        close(p_.grad.numpy(), d[key], 1e-4, 1e-7)
                    else:
                        assert p_.grad is None
            if vn is not None:
                close(vn.state(), d[f"r{rep}/vn"], 1e-6)
        # analytic fused-loss gradient (what the HIP kernel implements) vs autograd on the same sample
        _check_analytic_loss(a, g, c, d, sample)


def _check_analytic_loss(a, g, c, d, sample):
    """ppo_loss_fwd_bwd_ref (float64 closed form) == torch autograd w.r.t. logits / values."""
    D, S, A = int(d["dims"][3]), int(d["dims"][4]), int(d["dims"][5])
    pol = O.PolicyRef(a, D, S, A)
    load_net(pol.actor, g, f"c{c}/actor0"); load_net(pol.critic, g, f"c{c}/critic0")
    t = lambda x: torch.as_tensor(x, dtype=torch.float32)
    (share_obs, obs, rnn_a, rnn_c, actions, v_old, ret, masks, active, old_logp, adv, avail) = [t(x) for x in sample]
    feats, _ = pol.actor.features(obs, rnn_a, masks)
    z_raw = pol.actor.act.action_out.linear(feats).detach().requires_grad_(True)
    z = z_raw.masked_fill(avail == 0, -1e10)
    logp, ent, _ = pol.actor.act.logp_entropy(z, actions)
    values = pol.critic(share_obs, rnn_c, masks)[0].detach().requires_grad_(True)
    vn_mean, vn_var = 0.0, 1.0
    if a.use_valuenorm:
        vn = O.ValueNormRef(); vn.load_state(d["vn0"]); vn.update(ret)
        m, v = vn.mean_var(); vn_mean, vn_var = float(m), float(v)
        tgt = vn.normalize(ret)
    else:
        tgt = ret
    imp = torch.exp(logp - old_logp)
    s1, s2 = imp * adv, torch.clamp(imp, 1 - a.clip_param, 1 + a.clip_param) * adv
    surr = torch.min(s1, s2)
    if a.use_policy_active_masks:
        pl = (-surr * active).sum() / active.sum(); e = (ent * active.squeeze(-1)).sum() / active.sum()
    else:
        pl = -surr.mean(); e = ent.mean()
    (pl - a.entropy_coef * e).backward()
    vclip = v_old + (values - v_old).clamp(-a.clip_param, a.clip_param)
    lo = O.huber_ref(tgt - values, a.huber_delta) if a.use_huber_loss else (tgt - values) ** 2 / 2
    lc = O.huber_ref(tgt - vclip, a.huber_delta) if a.use_huber_loss else (tgt - vclip) ** 2 / 2
    l = torch.max(lo, lc) if a.use_clipped_value_loss else lo
    vl = (l * active).sum() / active.sum() if a.use_value_active_masks else l.mean()
    (vl * a.value_loss_coef).backward()
    out = O.ppo_loss_fwd_bwd_ref(z_raw.detach().numpy(), avail.numpy(), actions.numpy(), old_logp.numpy(), adv.numpy(),
                                 active.numpy(), values.detach().numpy(), v_old.numpy(), ret.numpy(), vn_mean, vn_var,
                                 a.clip_param, a.entropy_coef, a.value_loss_coef, a.huber_delta, a.use_huber_loss,
                                 a.use_clipped_value_loss, a.use_policy_active_masks, a.use_value_active_masks,
                                 a.use_valuenorm)
    close(out["policy_loss"], pl.item(), 1e-5); close(out["dist_entropy"], e.item(), 1e-5)
    close(out["value_loss"], vl.item(), 1e-5)
    close(out["dlogits"], z_raw.grad.numpy(), 1e-4, 1e-8)
    close(out["dvalues"], values.grad.numpy().reshape(-1), 1e-4, 1e-8)


def test_train_end_to_end():
    g = golden("train")
    for c in range(int(g["n_cases"])):
        d = sub(g, f"c{c}")
        T, N, M, D, S, A, H, nmb, rec, epochs, L = [int(x) for x in d["dims"]]
        a = args_from(episode_length=T, n_rollout_threads=N, hidden_size=H, lr=7e-4, critic_lr=7e-4, ppo_epoch=epochs,
                      num_mini_batch=nmb, use_recurrent_policy=bool(rec), data_chunk_length=L)
        pol = O.PolicyRef(a, D, S, A)
        load_net(pol.actor, g, f"c{c}/actor0"); load_net(pol.critic, g, f"c{c}/critic0")
        buf = _buffer_from(d, T, N, M, H)
        vn = O.ValueNormRef()
        info = O.train_ref(a, pol, vn, buf, perms=list(d["perms"]))
        ref = dict(zip([str(k) for k in d["info_keys"]], d["info"]))
        for k, v in info.items():
            close(v, ref[k], 1e-4)
        for tag, net in (("actor1", pol.actor), ("critic1", pol.critic)):
            ref_sd = sub(g, f"c{c}/{tag}")
            for k, v in net.state_dict().items():
                close(v.numpy(), ref_sd[k], 1e-4, 1e-6)
        close(vn.state(), d["vn1"], 1e-6)


def test_clip_adam_closed_form_matches_torch():
    rng = np.random.default_rng(0)
    P = 257
    p0 = rng.standard_normal(P).astype(np.float32)
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([param], lr=7e-4, eps=1e-5)
    p, m, v = p0.astype(np.float64), np.zeros(P), np.zeros(P)
    for step in range(3):
        gr = (rng.standard_normal(P) * (5.0 if step == 1 else 0.1)).astype(np.float32)
        param.grad = torch.from_numpy(gr.copy())
        n_t = float(torch.nn.utils.clip_grad_norm_([param], 10.0))
        opt.step()
        p, m, v, n = O.clip_adam_ref(p, gr, m, v, step, 7e-4, 10.0)
        close(n, n_t, 1e-6); close(p, param.detach().numpy(), 1e-6, 1e-7)


def test_separated_buffer_train_matches_reference():
    """share_policy=False (golden/separated.npz from onpolicy/utils/separated_buffer.py + r_mappo.py): the reference's separated
    buffer is the oracle's shared buffer with ONE agent — returns and a whole train() agree with the reference's outputs."""
    g = golden("separated")
    T, N, D, S, A, epochs, nmb = [int(x) for x in g["tr/dims"]]
    a = args_from(episode_length=T, n_rollout_threads=N, lr=7e-4, critic_lr=7e-4, ppo_epoch=epochs, num_mini_batch=nmb)
    pol = O.PolicyRef(a, D, S, A)
    load_net(pol.actor, g, "tr/actor0"); load_net(pol.critic, g, "tr/critic0")
    d = sub(g, "tr/buf")
    buf = O.BufferRef(a, 1, D, S, A)
    for name in ("share_obs", "obs", "rnn_states", "rnn_states_critic", "value_preds", "returns", "available_actions", "actions",
                 "action_log_probs", "rewards", "masks", "bad_masks", "active_masks"):
        getattr(buf, name)[...] = np.expand_dims(d[name], 2)
    want = buf.returns.copy()
    buf.returns[...] = 0
    vn = O.ValueNormRef()
    buf.compute_returns(g["tr/next_value"][:, None, :], vn)
    close(buf.returns[:T], want[:T], 1e-5, 1e-6)
    buf.returns[...] = want
    info = O.train_ref(a, pol, vn, buf, perms=list(g["tr/perms"]))
    ref = dict(zip([str(k) for k in g["tr/info_keys"]], g["tr/info"]))
    for k, v in info.items():
        close(v, ref[k], 1e-4)
    for tag, net in (("actor1", pol.actor), ("critic1", pol.critic)):
        ref_sd = sub(g, f"tr/{tag}")
        for k, v in net.state_dict().items():
            close(v.numpy(), ref_sd[k], 1e-4, 1e-6)
    close(vn.state(), g["tr/vn1"], 1e-6)
