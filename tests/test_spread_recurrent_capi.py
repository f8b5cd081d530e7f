"""CPU: mappo_rollout_episode_spread_recurrent validates its arguments on the host before any launch — error code and a message
that names the limit; no GPU needed."""
import ctypes


def test_rollout_episode_spread_recurrent_rejects_bad_arguments():
    from mappo_amd import _lib
    lib = _lib.load()
    ND = _lib.NetDesc                                        # (in_dim, hidden, out_dim, layer_N, use_relu, use_feature_norm, recurrent)
    actor, critic = ND(18, 64, 5, 1, 1, 1, 1), ND(54, 64, 1, 1, 1, 1, 1)
    one = ctypes.c_void_p(16)                                # a non-null pointer that is never dereferenced: validation fails first

    def call(a, c, T=8, N=8, M=3, L=3, env_T=25, centralized=1, ptr=one, null_at=None):
        p = [ptr] * 16
        if null_at is not None:
            p[null_at] = None
        rc = lib.mappo_rollout_episode_spread_recurrent(p[0], ctypes.byref(a) if a is not None else None, p[1],
                                                        ctypes.byref(c) if c is not None else None, T, N, M, L, env_T, 1, p[2], p[3], p[4],
                                                        p[5], p[6], 0, 1, 0, None, p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14],
                                                        p[15], centralized, None)
        return rc, lib.mappo_last_error().decode()

    cases = [
        (dict(a=None, c=critic), "null pointer"),
        (dict(a=actor, c=critic, ptr=None), "null pointer"),
        (dict(a=actor, c=critic, null_at=14), "null pointer"),                     # rnn_states
        (dict(a=actor, c=critic, null_at=15), "null pointer"),                     # rnn_states_critic
        (dict(a=ND(18, 64, 5, 1, 1, 1, 0), c=critic), "recurrent"),
        (dict(a=actor, c=ND(54, 64, 1, 1, 1, 1, 0)), "recurrent"),
        (dict(a=ND(65, 64, 5, 1, 1, 1, 1), c=ND(65, 64, 1, 1, 1, 1, 1), centralized=0), "narrow"),
        (dict(a=ND(18, 64, 5, 2, 1, 1, 1), c=ND(54, 64, 1, 2, 1, 1, 1)), "layer_N <= 1"),
        (dict(a=actor, c=ND(54, 64, 1, 0, 1, 1, 1)), "share layer_N"),
        (dict(a=actor, c=ND(54, 64, 1, 1, 0, 1, 1)), "activation"),
        (dict(a=ND(18, 64, 6, 1, 1, 1, 1), c=critic), "5 actions"),
        (dict(a=actor, c=ND(54, 64, 5, 1, 1, 1, 1)), "critic out_dim"),
        (dict(a=actor, c=critic, M=0), "out of range"),
        (dict(a=actor, c=critic, M=9), "out of range"),
        (dict(a=actor, c=critic, L=9), "out of range"),
        (dict(a=actor, c=critic, T=0), "bad shape"),
        (dict(a=ND(20, 64, 5, 1, 1, 1, 1), c=critic), "observation features"),
        (dict(a=actor, c=ND(18, 64, 1, 1, 1, 1, 1)), "centralized"),
        (dict(a=actor, c=critic, centralized=0), "in_dim"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc == -1, (kw, rc)
        assert "rollout_episode_spread_recurrent" in err and msg in err, (kw, err)


def test_wrapper_and_signature_exist():
    from mappo_amd import _lib, ops
    assert "mappo_rollout_episode_spread_recurrent" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mappo_rollout_episode_spread_recurrent"][1]) == 30
    assert callable(ops.rollout_episode_spread_recurrent)
