"""CPU: the host side of the one-launch SMAC-shaped recurrent episode (mappo_rollout_episode_smac_recurrent, opt-in
MAPPO_SMAC_REC_EPISODE=1) — the entry point refuses every limit by name before any launch, the ops wrapper turns a refusal into
ValueError, SyntheticSMACEnv.episode_block needs a device env, the runner does not take the path without the flag — and, through
the host mirror of the synthetic env (tests/synth_ref.py), the env seeds of the GPU cases (tests/smac_episode_cases.py) reach every
mask branch of the kernel within their T steps."""
import ctypes

import pytest
import torch

import smac_episode_cases as SC


def _call(lib, a, c, T=6, N=7, M=3, centralized=1, ptr=ctypes.c_void_p(16), null_at=None, avail=True, avail_buf=True):
    """ptr: a non-null pointer that is never dereferenced — validation fails first."""
    p = [ptr] * 19
    if null_at is not None:
        p[null_at] = None
    rc = lib.mappo_rollout_episode_smac_recurrent(
        p[0], ctypes.byref(a) if a is not None else None, p[1], ctypes.byref(c) if c is not None else None, T, N, M,
        p[2], p[3], ptr if avail else None, p[4], p[5], None, 0, 1, 0, None,
        p[6], p[7], ptr if avail_buf else None, p[8], p[9], p[10], p[11], p[12], p[13], p[14], p[15], p[16], centralized, None)
    return rc, lib.mappo_last_error().decode()


def test_rollout_episode_smac_recurrent_rejects_every_limit_by_name():
    from mappo_amd import _lib
    lib = _lib.load()
    ND = _lib.NetDesc                                        # (in_dim, hidden, out_dim, layer_N, use_relu, use_feature_norm, recurrent)
    actor, critic = ND(30, 64, 9, 1, 1, 1, 1), ND(48, 64, 1, 1, 1, 1, 1)
    cases = [
        (dict(a=None, c=critic), "null pointer"),
        (dict(a=actor, c=None), "null pointer"),
        (dict(a=actor, c=critic, ptr=None, avail=False, avail_buf=False), "null pointer"),
        (dict(a=ND(30, 64, 9, 1, 1, 1, 0), c=critic), "recurrent"),
        (dict(a=actor, c=ND(48, 64, 1, 1, 1, 1, 0)), "recurrent"),
        (dict(a=ND(65, 64, 9, 1, 1, 1, 1), c=critic), "narrow"),
        (dict(a=actor, c=ND(65, 64, 1, 1, 1, 1, 1)), "narrow"),
        (dict(a=ND(30, 64, 9, 2, 1, 1, 1), c=ND(48, 64, 1, 2, 1, 1, 1)), "layer_N <= 1"),
        (dict(a=actor, c=ND(48, 64, 1, 0, 1, 1, 1)), "share layer_N"),
        (dict(a=actor, c=ND(48, 64, 1, 1, 0, 1, 1)), "activation"),
        (dict(a=ND(30, 64, _lib.MAX_ACTIONS + 1, 1, 1, 1, 1), c=critic), f"out_dim {_lib.MAX_ACTIONS + 1}"),
        (dict(a=actor, c=ND(48, 64, 2, 1, 1, 1, 1)), "critic out_dim"),
        (dict(a=actor, c=critic, M=0), "out of range"),
        (dict(a=actor, c=critic, M=17), "out of range"),
        (dict(a=actor, c=critic, T=0), "bad shape"),
        (dict(a=actor, c=critic, centralized=0), "not centralized"),
        (dict(a=actor, c=critic, avail=False), "go together"),
        (dict(a=actor, c=critic, avail_buf=False), "go together"),
    ]
    cases += [(dict(a=actor, c=critic, null_at=i), "null pointer") for i in range(17) if i != 3]
    for kw, msg in cases:
        rc, err = _call(lib, **kw)
        assert rc == -1, (kw, rc)
        assert "rollout_episode_smac_recurrent" in err and msg in err, (kw, err)
    # env_share_obs is required only by a centralized critic
    rc, err = _call(lib, a=actor, c=critic, null_at=3)
    assert rc == -1 and "null pointer" in err
    # the widest accepted shapes pass the validation ... which only a GPU can follow with a launch: not called here


def test_wrapper_and_signature_exist():
    from mappo_amd import _lib, ops
    assert len(_lib.SIGNATURES["mappo_rollout_episode_smac_recurrent"][1]) == 31
    assert callable(ops.rollout_episode_smac_recurrent)


def test_ops_wrapper_raises_value_error_with_the_library_message(monkeypatch):
    """A limit the kernel refuses reaches Python as ValueError carrying the C message (pointers faked: nothing is launched)."""
    from mappo_amd import ops
    monkeypatch.setattr(ops, "_ptr", lambda t, dtype=torch.float32, allow_none=False: None if t is None else ctypes.c_void_p(16))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    T, N, M, D, S, A = 2, 3, 3, 30, 48, 9
    z = lambda *s, **k: torch.zeros(*s, **k)
    args = lambda a, c: (z(1), a, z(1), c, z(T, N, M, D), z(T, N, M, S), z(T, N, M, A), z(T, N), z(T, N, M, dtype=torch.bool), None, False, 1, 0,
                         None) + (z(1),) * 12 + (True,)
    with pytest.raises(ValueError, match="rollout_episode_smac_recurrent.*layer_N <= 1"):
        ops.rollout_episode_smac_recurrent(*args(ops.net_desc(D, A, 2, recurrent=True), ops.net_desc(S, 1, 2, recurrent=True)))
    with pytest.raises(ValueError, match="needs recurrent network descriptors"):
        ops.rollout_episode_smac_recurrent(*args(ops.net_desc(D, A), ops.net_desc(S, 1)))
    with pytest.raises(ValueError, match=r"\[T, N, M, D\]"):
        bad = list(args(ops.net_desc(D, A, 1, recurrent=True), ops.net_desc(S, 1, 1, recurrent=True)))
        bad[7] = z(T, N, M)
        ops.rollout_episode_smac_recurrent(*bad)


def test_episode_block_needs_a_device_env_and_the_runner_needs_the_flag(monkeypatch):
    from mappo_amd.envs.synthetic import SyntheticSMACEnv
    from mappo_amd.runner.shared.smac_runner import SMACRunner
    env = SyntheticSMACEnv.__new__(SyntheticSMACEnv)        # (the constructor seeds the device generator: no device here)
    env.N, env.M, env.D, env.S, env.A, env.pool_steps, env._t, env.device = 4, 3, 30, 48, 9, 6, 0, torch.device("cpu")
    with pytest.raises(RuntimeError, match="episode_block: needs a device env"):
        env.episode_block()
    env.device, env.pool_steps = torch.device("cuda"), 0
    with pytest.raises(RuntimeError, match="pool_steps > 0"):
        env.episode_block()
    env.pool_steps, env._t = 6, 3
    with pytest.raises(AssertionError, match="pool boundary"):
        env.episode_block()
    r = SMACRunner.__new__(SMACRunner)                       # the flag is looked at before anything else of the runner
    monkeypatch.delenv("MAPPO_SMAC_REC_EPISODE", raising=False)
    assert r._episode_launch_ok() is False
    monkeypatch.setenv("MAPPO_SMAC_REC_EPISODE", "0")
    assert r._episode_launch_ok() is False


@pytest.mark.parametrize("case", SC.CASES + [c[:10] + (False, c[10]) for c in SC.F64_CASES])
def test_env_seeds_reach_every_mask_branch(case):
    """Per GPU case: within the T steps of its first rollout the env output holds at least one env termination, one row that is
    dead in a live env (M >= 2), one env whose agents are all done without a termination (where reachable: see
    smac_episode_cases.required) and one unavailable action on a row whose env is live."""
    M, N, T, D, S, A = case[:6]
    cov = SC.coverage(M, N, T, D, S, A, case[11])
    for k in SC.required(M, T):
        assert cov[k] > 0, (case, cov)


@pytest.mark.parametrize("case", SC.F64_CASES)
def test_float64_reference_alone_stays_inside_the_skip_cap(case):
    """The GPU float64 test may skip a sampled action where the uniform lies within 1e-5 of a float64 CDF edge, at most 1 % of the
    (step, row) pairs.  On the same host-built weights and slot-0 rows, the env mirror's output and the host Philox draw, the
    float64 reference alone puts at most that many pairs so near an edge — so the cap is met by the choice of seeds, not by chance
    on the GPU."""
    M, N, T, D, S, A, relu, layer_N, fnorm, centralized, seed, _ = case
    assert SC.reference_skips(M, N, T, D, S, A, relu, layer_N, fnorm, centralized, seed) <= 0.01 * T * N * M
