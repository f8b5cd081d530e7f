"""simple_spread beyond 3 agents and 3 landmarks, without a GPU: tests/golden/mpe_spread_shapes.npz holds episodes stepped by the
reference's own environment at seven shapes (tests/golden/generate_golden_mpe_spread_shapes.py).  oracle/mpe_oracle.py, which the
GPU tests hold the kernels against, must reproduce them to the 1e-12 of test_mpe_reference.py; the fixture must cover what it
claims, read from the file; and the host restatement of the reset draws must give every coordinate Philox words of its own."""
import numpy as np
import pytest

import mpe_spread_np as MS
from conftest import golden, sub

ATOL = 1e-12                                   # test_mpe_reference.py's: the margin is for another libm's logaddexp
PLAIN, CROWDED, SCRIPTED, SOFT = 0, 1, 2, 3


@pytest.fixture(scope="module")
def fx():
    g = golden("mpe_spread_shapes")
    return {s: sub(g, "%dx%d" % s) for s in MS.shapes(g)}


def _pair_dists(pos):
    """[E, M (M - 1) / 2] distances between the agents of pos [E, M, 2]."""
    M = pos.shape[1]
    return np.stack([np.linalg.norm(pos[:, a] - pos[:, b], axis=-1) for a in range(M) for b in range(a + 1, M)], axis=1)


def test_fixture_covers_the_shapes_it_is_for(fx):
    """Everything below is computed from the arrays' own shapes and values."""
    shapes = [(f["pos0"].shape[1], f["lpos"].shape[1]) for f in fx.values()]
    assert shapes == list(fx)                                                     # the group names say what the arrays hold
    Ms, Ls = [m for m, _ in shapes], [l for _, l in shapes]
    assert 1 in Ms and 1 in Ls and max(Ms) == 8 and max(Ls) == 8
    assert any(m < l for m, l in shapes) and any(m > l for m, l in shapes) and any(m == l for m, l in shapes)
    assert {16 // m for m in Ms} >= {16, 8, 4, 3, 2}                              # every tile size of the one-launch episode
    assert set(shapes) >= {(1, 1), (1, 3), (2, 5), (5, 2), (4, 3), (7, 1), (8, 8)}
    for (M, L), f in fx.items():
        E, T, D = f["obs"].shape[0], 6, 4 + 2 * L + 4 * (M - 1)
        assert f["obs"].shape == (E, T, M, D) and f["obs0"].shape == (E, M, D) and f["obs"].dtype == np.float64
        assert f["actions_env"].shape == (E, T, M, 5) and f["actions"].shape == (E, T, M) and f["rewards"].shape == (E, T, M)
        assert f["pos"].shape == f["vel"].shape == (E, T, M, 2) and f["lpos"].shape == (E, L, 2)
        np.testing.assert_array_equal(f["pos"][:, -1], f["pos1"])
        np.testing.assert_array_equal(f["vel"][:, -1], f["vel1"])
        assert not f["dones"][:, :-1].any() and f["dones"][:, -1].all()
        kind = f["kind"]
        # one soft episode: probability rows that are no one-hots, exactly representable in fp32 (the kernel's action input)
        soft = np.flatnonzero(kind == SOFT)
        assert len(soft) == 1
        p = f["actions_env"][soft[0]]
        assert (p > 0).all() and (p < 1).all() and np.abs(p.sum(-1) - 1).max() < 1e-6 and (f["actions"][soft[0]] == -1).all()
        np.testing.assert_array_equal(p, p.astype(np.float32).astype(np.float64))
        hard = kind != SOFT
        np.testing.assert_array_equal(f["actions_env"][hard], np.eye(5)[f["actions"][hard]])
        assert set(np.unique(f["actions"][hard])) == {0, 1, 2, 3, 4}
        if M == 1:
            continue
        d0 = _pair_dists(f["pos0"])
        assert d0.min() > 0.0                                                     # no two agents on one point: 0 / 0 in the reference
        assert (kind == CROWDED).sum() >= 1 and (d0[kind == CROWDED][:, :M - 1] < 0.3).all()      # every agent touches agent 0
        assert (d0[kind == PLAIN] > 0.3).any()                                    # and pairs out of contact
        ds = d0[kind == SCRIPTED].reshape(-1)
        for want in (0.3 - 1e-4, 0.3 + 1e-4, 1e-6, 50.0):
            assert (np.abs(ds - want) <= 1e-9 * max(1.0, want)).any(), (M, L, want)
        # deep overlap pushes two agents apart faster than any action can (5 * 0.1 per step)
        assert np.abs(f["vel"][kind == SCRIPTED][:, 0]).max() > 1.0


def test_oracle_equals_the_reference_at_every_shape(fx):
    """obs0, and every step's observations, rewards, dones and float64 state, of every episode — crowded, scripted contacts and
    probability actions included."""
    from oracle import mpe_oracle as R
    worst_all = 0.0
    for (M, L), f in fx.items():
        T = f["obs"].shape[1]
        env = R.SimpleSpreadRef(f["pos0"], f["vel0"], f["lpos"], T)
        o0 = env.obs()
        assert o0.shape == f["obs0"].shape
        worst = np.abs(o0 - f["obs0"]).max()
        np.testing.assert_allclose(o0, f["obs0"], rtol=0, atol=ATOL, err_msg=f"{M}x{L} obs0")
        for t in range(T):
            def keep(n):                       # the reference env does not reset itself: keep the stepped state
                return env.pos[n], env.vel[n], env.lpos[n]
            obs, rew, dones = env.step(f["actions_env"][:, t], keep)
            worst = max(worst, np.abs(obs - f["obs"][:, t]).max(), np.abs(rew[..., 0] - f["rewards"][:, t]).max(),
                        np.abs(env.pos - f["pos"][:, t]).max(), np.abs(env.vel - f["vel"][:, t]).max())
            np.testing.assert_allclose(obs, f["obs"][:, t], rtol=0, atol=ATOL, err_msg=f"{M}x{L} obs, step {t}")
            np.testing.assert_allclose(rew[..., 0], f["rewards"][:, t], rtol=0, atol=ATOL, err_msg=f"{M}x{L} rewards, step {t}")
            np.testing.assert_allclose(env.pos, f["pos"][:, t], rtol=0, atol=ATOL, err_msg=f"{M}x{L} pos, step {t}")
            np.testing.assert_allclose(env.vel, f["vel"][:, t], rtol=0, atol=ATOL, err_msg=f"{M}x{L} vel, step {t}")
            np.testing.assert_array_equal(dones, f["dones"][:, t])
        print(f"simple_spread {M} x {L}: oracle vs reference, max |diff| {worst:.2e}")
        worst_all = max(worst_all, worst)
    print(f"simple_spread, all shapes: oracle vs reference, max |diff| {worst_all:.2e} (bound {ATOL:.0e})")


def test_reset_draws_use_distinct_philox_words():
    """M = L = 8 fills an environment's 32 uniform numbers: the 2 (M + L) numbers of an environment and of its neighbour, and the
    Philox word indices they read, are pairwise distinct — and so are the values drawn."""
    a, l = MS.uniform_indices(2, 8, 8)
    u = np.concatenate([a.reshape(-1), l.reshape(-1)])
    assert len(u) == 2 * 2 * (8 + 8) and len(np.unique(u)) == len(u)
    hi, lo = MS.philox_indices(u)
    words = np.concatenate([hi, lo])
    assert len(np.unique(words)) == 2 * len(u)
    assert sorted(u.tolist()) == list(range(2 * MS.DRAWS))                        # dense: the two environments tile 0 .. 63
    pos, lpos = MS.reset_draws(3, 1, 2, 8, 8)
    vals = np.concatenate([pos.reshape(-1), lpos.reshape(-1) / 0.8])
    assert len(np.unique(vals)) == len(vals)
    # smaller shapes use a subset of the same numbers: the layout does not move with M or L
    for M, L in ((1, 1), (5, 2), (3, 3)):
        p, q = MS.reset_draws(3, 1, 2, M, L)
        np.testing.assert_array_equal(p, pos[:, :M])
        np.testing.assert_array_equal(q, lpos[:, :L])


def test_reset_draws_take_seed_and_episode_as_64_bit_numbers():
    base = MS.reset_draws(3, 6, 4, 3, 3)
    for seed, ep in ((2 ** 32 + 3, 6), (3, 2 ** 32 + 6)):
        other = MS.reset_draws(seed, ep, 4, 3, 3)
        assert not np.array_equal(base[0], other[0]) and not np.array_equal(base[1], other[1])
    pos, lpos = MS.reset_draws(2 ** 32 + 3, 2 ** 32 + 6, 257, 8, 8)
    assert pos.min() >= -1.0 and pos.max() <= 1.0 and np.abs(lpos).max() <= 0.8
    assert abs(pos.mean()) < 0.05 and abs(pos.var() - 1 / 3) < 0.03
