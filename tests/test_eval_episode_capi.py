"""CPU: mappo_eval_episode_spread (csrc/eval_spread.h) is exported and bound, validates its arguments on the host before any launch —
error code and a message that names the limit — and the float64 reference the GPU test compares against (eval_spread_ref.py) keeps
its undecided-argmax share within the cap for the committed seeds.  No GPU needed."""
import ctypes

import pytest

import eval_spread_ref as ER


def test_symbol_wrapper_and_policy_method_exist():
    from mappo_amd import _lib, ops
    from mappo_amd.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    assert hasattr(_lib.load(), "mappo_eval_episode_spread")
    assert len(_lib.SIGNATURES["mappo_eval_episode_spread"][1]) == 20
    assert callable(ops.eval_episode_spread) and callable(R_MAPPOPolicy.eval_episode_env_fused)


def test_eval_episode_spread_rejects_bad_arguments():
    from mappo_amd import _lib
    lib = _lib.load()
    ND = _lib.NetDesc                                        # (in_dim, hidden, out_dim, layer_N, use_relu, use_feature_norm, recurrent)
    actor = ND(18, 64, 5, 1, 1, 1, 0)
    one = ctypes.c_void_p(16)                                # a non-null pointer that is never dereferenced: validation fails first

    def call(a, T=25, N=8, M=3, L=3, env_T=25, ptr=one, null_at=None, actions=None):
        p = [ptr] * 7                                        # params, pos, vel, lpos, tstep, episode, returns
        if null_at is not None:
            p[null_at] = None
        rc = lib.mappo_eval_episode_spread(p[0], ctypes.byref(a) if a is not None else None, T, N, M, L, env_T, 1, p[1], p[2], p[3],
                                           p[4], p[5], 1, 1, 0, None, p[6], actions, None)
        return rc, lib.mappo_last_error().decode()

    cases = [
        (dict(a=None), "null desc"),
        (dict(a=ND(18, 64, 5, 1, 1, 1, 1)), "recurrent"),
        (dict(a=ND(65, 64, 5, 1, 1, 1, 0)), "narrow"),
        (dict(a=ND(18, 64, 5, 2, 1, 1, 0)), "layer_N <= 1"),
        (dict(a=ND(18, 64, 6, 1, 1, 1, 0)), "5 actions"),
        (dict(a=ND(20, 64, 5, 1, 1, 1, 0)), "observation features"),
        (dict(a=ND(64, 64, 5, 1, 1, 1, 0), M=8, L=8), "observation features"),      # M = L = 8 has 48
        (dict(a=actor, T=0), "bad shape"),
        (dict(a=actor, N=0), "bad shape"),
        (dict(a=actor, env_T=0), "bad shape"),
        (dict(a=actor, M=0), "out of range"),
        (dict(a=actor, M=9), "out of range"),
        (dict(a=actor, L=0), "out of range"),
        (dict(a=actor, L=9), "out of range"),
        (dict(a=actor, ptr=None), "null pointer"),
    ] + [(dict(a=actor, null_at=k), "null pointer") for k in range(7)]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc == -1, (kw, rc)
        assert "eval_episode_spread" in err and msg in err, (kw, err)


@pytest.mark.parametrize("case", ER.F64_CASES, ids=[f"N{c[0]}-M{c[1]}-T{c[3]}" for c in ER.F64_CASES])
def test_float64_reference_keeps_the_undecided_share_within_the_cap(case):
    """From the float64 reference alone: envs with a top-two logit gap below MARGIN at any step are at most NEAR_CAP of the case,
    the episode uses more than one action, and the env's episodes end inside it where the case says so."""
    N, M, L, T, env_T = case[:5]
    ref = ER.reference_episode(case)
    print(f"\nnear {int(ref['near'].sum())} of {N} envs, smallest top-two gap {ref['min_gap']:.3e} (margin {ER.MARGIN:.1e})")
    assert ref["near"].mean() <= ER.NEAR_CAP, f"{int(ref['near'].sum())} of {N} envs have a gap below {ER.MARGIN}"
    assert len(set(ref["actions"].reshape(-1).tolist())) > 1
    assert ref["episode"].tolist() == [T // env_T] * N and ref["tstep"].tolist() == [T % env_T] * N
