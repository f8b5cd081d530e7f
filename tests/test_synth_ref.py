"""The host mirror of the synthetic SMAC env kernels (tests/synth_ref.py), on the CPU: the five kinds of draw of a step never share a
Philox word at any shape the GPU tests run, the state-machine case exercises every transition, and the pool mirror is P steps of
the step mirror."""
import itertools

import numpy as np
import pytest

import synth_ref as SR

SHAPES = sorted(set(SR.STEP_SHAPES.values()) | {s for s, _ in SR.POOL_SHAPES.values()}
                | {tuple(SR.STATE_CASE[k] for k in "NMDSA"), (37, 4, 30, 48, 9)})


def test_case_list_has_the_workgroup_counts_it_names():
    for name, shape in SR.STEP_SHAPES.items():
        assert SR.workgroups(shape) == SR.WORKGROUPS[name], name
    for name, (shape, P) in SR.POOL_SHAPES.items():
        assert SR.workgroups(shape, P) == SR.WORKGROUPS[name], name
    assert {1, 31, 32, 33, 65} <= {SR.WORKGROUPS[k] for k in SR.STEP_SHAPES}
    assert SR.WORKGROUPS["over_cap"] > 4096 and SR.WORKGROUPS["over_cap_p3"] > 8192
    for P in (1, 7):
        assert {1, 31, 32, 33, 65} <= {SR.WORKGROUPS[k] for k, (_, p) in SR.POOL_SHAPES.items() if p == P}
    assert sum((D + S + A) % 256 != 0 and 256 % (D + S + A) != 0 for _, _, D, S, A in SHAPES) >= len(SHAPES) - 2


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_kinds_of_draw_share_no_philox_word(shape):
    N, M, D, S, A = shape
    w = SR.stream_words(*shape)
    assert tuple(w) == SR.KINDS
    want = dict(normal=2 * N * M * (D + S), avail=N * M * (A - 1), death=N * M, termination=N, reward=2 * N)
    for k, v in w.items():
        assert v.size == want[k] and np.unique(v).size == v.size and v.min(initial=0) >= 0, k
    for a, b in itertools.combinations(SR.KINDS, 2):
        assert np.intersect1d(w[a], w[b]).size == 0, (a, b)
    # and the mirror draws what stream_words says: the words behind obs / share / avail / the state draws / the rewards of step() are
    # those of the kernel's layout (element e: words 2e, 2e + 1; then the agents, the envs, the rewards)
    W, total = D + S + A, N * M * (D + S + A)
    assert w["normal"].max() < 2 * total and w["avail"].max(initial=0) < 2 * total
    assert w["death"][0] == 2 * total and w["termination"][0] == 2 * (total + N * M) and w["reward"].min() == 2 * (total + N * M + N)


def test_mirror_values_at_the_smallest_shape():
    """N = M = D = S = A = 1 by hand: three elements, then one agent, one env, one reward."""
    seed, ctr = 5, 9
    o = SR.step(seed, ctr, 1, 1, 1, 1, 1, 0.5, 0.5, np.zeros((1, 1), bool))
    u = lambda w: float(SR.uniform(seed, ctr, np.array([w]))[0])
    z = lambda a, b: np.sqrt(-2 * np.log(a)) * np.cos(2 * np.pi * b)
    assert 0.0 < u(0) <= 1.0
    assert float(o["obs"][0, 0, 0]) == z(u(0), u(1)) and float(o["share"][0, 0, 0]) == z(u(2), u(3))
    assert float(o["avail"][0, 0, 0]) == 1.0                                     # action 0: always available, no draw
    assert bool(o["died"][0, 0]) == (u(6) <= 0.5) and bool(o["term"][0]) == (u(8) <= 0.5)
    assert float(o["rewards"][0]) == z(u(10), u(11))
    assert o["counter"] == ctr + 1
    b = float(o["obs_bound"][0, 0, 0])
    moves = [abs(z(u(0), u(1) + SR.H) - z(u(0), u(1))), abs(z(u(0), u(1) - SR.H) - z(u(0), u(1)))]
    moves += [abs(z(u(0) + d, u(1)) - z(u(0), u(1))) for d in (SR.H, -SR.H) if 0.0 < u(0) + d <= 1.0]
    assert b > 0.0 and abs(b - max(moves)) <= 1e-6 * b            # (the mirror factors r and cos out of the differences: 1e-16 on 1e-7)


def test_bound_at_the_ends_of_u1():
    """u1 = 2^-24 (the largest normal, 5.77) and u1 = 1 (a zero) only move inwards; both bounds are finite and non-zero."""
    u1, u2 = np.array([SR.H, 1.0]), np.array([0.125, 0.125])
    z, b = SR.normal(u1, u2), SR.normal_bound(u1, u2)
    assert np.isfinite(z).all() and np.isfinite(b).all() and (b > 0).all()
    assert abs(z[0] - np.sqrt(2 * 24 * np.log(2)) * np.cos(np.pi / 4)) < 1e-12 and z[1] == 0.0
    assert abs(b[1] - np.sqrt(-2 * np.log1p(-SR.H)) * np.cos(np.pi / 4)) < 1e-12


def test_state_case_exercises_every_transition():
    c = SR.STATE_CASE
    cov = SR.coverage(c["seed"], 1, c["N"], c["M"], c["D"], c["S"], c["A"], c["p_death"], c["p_term"], SR.state_case_dead0(), c["steps"])
    print(cov)
    assert set(cov) == {"alive_to_dead", "dead_stays_dead", "dead_to_alive_by_termination", "termination_with_nobody_dead",
                        "termination_and_death_same_step"}
    assert all(v > 0 for v in cov.values()), cov
    assert 0 < int(SR.state_case_dead0().sum()) < c["N"] * c["M"]


@pytest.mark.parametrize("P", [1, 5, 7])
def test_pool_mirror_is_P_steps_of_the_step_mirror(P):
    seed, N, M, D, S, A = 2 ** 40 + 3, 6, 3, 4, 5, 3
    dead0 = np.arange(N * M).reshape(N, M) % 4 == 1
    steps, ctr = SR.run(seed, 17, N, M, D, S, A, 0.3, 0.2, dead0, P)
    q = SR.pool(seed, 17, N, M, D, S, A, 0.3, 0.2, dead0, P)
    assert q["counter"] == ctr == 17 + P
    for k in ("obs", "share", "avail", "rewards", "dones", "obs_bound", "share_bound", "rewards_bound"):
        assert q[k].shape[0] == P
        for p in range(P):
            np.testing.assert_array_equal(q[k][p], steps[p][k], err_msg=f"{k}, step {p}")
    np.testing.assert_array_equal(q["dead_out"], steps[-1]["dead_out"])
    assert any(not np.array_equal(steps[0]["obs"], s["obs"]) for s in steps[1:]) or P == 1


def test_largest_case_holds_an_avail_draw_on_the_threshold():
    """The first launch of the over_cap cases draws 0.7f itself for one avail element (and the mirror calls it available)."""
    shape = SR.STEP_SHAPES["over_cap"]
    N, M, D, S, A = shape
    W = D + S + A
    e = np.arange(N * M * W, dtype=np.int64)
    e = e[e % W > D + S]
    u = SR.uniform(SR.SEEDS["over_cap"], 1, 2 * e)
    hit = u == float(np.float32(0.7))
    assert hit.sum() >= 1
    avail = SR.draws(SR.SEEDS["over_cap"], 1, *shape)["avail"].reshape(-1, A)[:, 1:].reshape(-1)
    assert (avail[hit] == 1.0).all() and np.array_equal(avail == 1.0, u <= float(np.float32(0.7)))
