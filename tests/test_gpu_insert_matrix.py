"""Edge shapes of the rollout insert and row-index kernels (csrc/insert.hip, csrc/insert_core.h) and of the fused forms of their
bodies, against references that share no code with them: tests/insert_ref.py (NumPy, written from the reference's Python and pinned
by tests/test_oracle_golden.py) and oracle.mappo_oracle.recurrent_rows (pinned by golden/generators.npz).

Every comparison is bit for bit on the int32 view of the arrays, so -0.0 and NaN payloads count: these kernels copy, write 0 / 1 or
multiply by exactly 0 or 1.  The one exception follows from IEEE 754, not from the kernels: inf * 0 is an invalid operation whose
result is "a quiet NaN" whose sign and payload the standard leaves open (x86 hosts produce the negative one), so where a state is
+-inf and its row is reset the result must be a NaN and its bits are free.  NaN * 0 propagates the operand, and is compared bit for bit.

Every destination is a slice of a larger allocation filled with the words FILL (a quiet NaN with a payload no source holds; for
int32 outputs the same word as a sentinel).  After the launch the G words on either side must still be FILL, and the slice must
equal the reference everywhere, so every element inside was written.  Every strided source is a view into a larger random pool:
a mis-strided read picks up a wrong value instead of faulting, and the pools must be unchanged afterwards.

What runs, per entry point (cap = the largest grid x workgroup size, beyond which the grid-stride loop takes a second pass):

mappo_insert_mpe (cap 2048 x 256 = 524 288 share elements): (N, M, D) = (1, 1, 1), (1, 3, 18), (37, 1, 7), (5, 8, 64) centralized and
  not; (700, 5, 31) centralized = 542 500 and (2100, 5, 51) not centralized = 535 500 elements cross the cap with a ragged second
  pass.  Each under the three source layouts of COMBOS: obs as an interior slice with a 4-byte-aligned base and padding between
  agents and between threads ("pad"), or permuted so that stride_n < stride_m ("perm"); rewards with strides (0, 0), (1, 0), (M, 1);
  dones contiguous or transposed (stride_n 1, stride_m N).  Sources hold -0.0 and NaNs with a payload.
mappo_insert_mpe_rnn: the same layouts at (1, 1, 1) H 4, (1, 3, 18) centralized H 128, (37, 1, 7) centralized H 64 (the state loop
  sizes the grid: 16 float4 per row against 7 elements), (5, 8, 64) centralized H 4 (the copy loop does) and (4100, 8, 4) H 64 =
  524 800 float4 items, one workgroup over the cap.  States hold -0.0, +-inf, NaN and negative values in rows with and without done.
mappo_insert_smac (grid from N M max(D, S), cap 524 288): the eight present / absent combinations of avail, bad_transition and the
  state pair at (N, M, D, S, A, H) = (9, 3, 30, 48, 9, 64); (1, 1, 1, 1, 1, 4); (37, 5, 7, 5, 40, 64) where A alone outgrows the
  grid (1 536 threads for 7 400 availability words); (500, 8, 100, 140, 9, 64) = 560 000 share elements over the cap.  dones contain
  envs with every, some and no agent done; contiguous and transposed dones, full and broadcast rewards.
mappo_rollout_step / _md with obs_dst (insert_mpe_body as a workgroup role; narrow: ceil(elements / 2048) <= 256 insert workgroups
  of 64 .. 256 threads): (1, 1, 4), (37, 3, 18), (700, 5, 12) centralized = 210 000 elements on 103 workgroups (8 passes), a wide
  pair D = 130 (there the insert is the stand-alone kernel), MultiDiscrete heads (3, 3), and the values-only form.
mappo_recurrent_rollout_step (insert_smac_body as a role, <= 64 insert workgroups): (D, S, A) = (30, 48, 9) narrow and (176, 322, 18)
  wide at (N, M) = (1, 1) and (37, 3), avail and bad_transition both present and both absent.
mappo_rollout_episode (insert_mpe_episode_run<16, uint32_t> in the register body, <4, uint32_t> in the LDS body):
  (T, N, M, D) = (1, 1, 1, 4), (3, 7, 3, 18), (25, 2, 3, 18), (2, 300, 3, 18), centralized and not, layer_N 0 and 1, both bodies.  No
  element total is a multiple of U x waves x 64, so the predicated last pass always runs; sources are strided in t, n and m.
  NOT covered: the int64_t instantiation of the index split, which needs more than 2^32 elements (16 GiB of share_obs) and is out
  of reach of a test that takes seconds.
mappo_recurrent_rows (cap 4096 x 256 = 1 048 576 entries): (T, N, M, L, nmb, E) = (5, 1, 1, 1, 1, 1), (10, 3, 2, 10, 2, 2) with L = T,
  (7, 5, 2, 3, 23, 1) with mbs = 1, (25, 4, 3, 10, 4, 2) with 30 chunks of which 2 are left over, (400, 100, 3, 10, 2, 9) = 1 080 000
  entries over the cap.  Its two bad-argument paths run on the host: tests/test_capi_symbols.py.
mappo_copy_batch is covered by tests/test_gpu_train_glue.py and is not repeated here.

test_case_lists_cross_the_caps needs no GPU: it mirrors the launch geometry in Python and asserts the claims above."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from insert_ref import episode_insert_ref, insert_mpe_ref, insert_smac_ref
from oracle import mappo_oracle as O

gpu = pytest.mark.gpu
F32 = np.float32
T_, F_ = True, False
G = 64                                    # guard words on either side of a destination (a multiple of 4: the slices stay 16-byte aligned)
FILL = 0x7FC0BEEF                         # "never written": a quiet NaN with this payload, or this int32
PAYLOAD_NAN = 0x7FC01234                  # a NaN the sources hold: a copy must keep its payload
SLACK = 1024                              # pool elements past the last one a view reaches


@pytest.fixture(scope="module")
def ops(gpu_device):
    from mappo_amd import ops as _ops
    return _ops


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---- destinations with guards ---------------------------------------------------------------------------------------------
class Slots:
    def __init__(self):
        self.pools = {}

    def new(self, name, *shape, dtype=torch.float32):
        n = int(np.prod(shape))
        pool = torch.full((n + 2 * G,), FILL, dtype=torch.int32, device="cuda")
        self.pools[name] = (pool, n)
        return pool[G:G + n].view(dtype).view(*shape)

    def check(self, name, want=None, free_nan=None):
        """Guards untouched; with `want`: the slice equals it bit for bit (free_nan: where any NaN will do, see the module docstring)."""
        pool, n = self.pools[name]
        bits = pool.cpu().numpy()
        assert (bits[:G] == FILL).all(), f"{name}: wrote in front of the destination"
        assert (bits[G + n:] == FILL).all(), f"{name}: wrote past the destination"
        if want is None:
            return
        want = np.ascontiguousarray(want).reshape(-1)
        assert want.size == n and want.dtype.itemsize == 4, (name, want.shape, want.dtype, n)
        got, wb = bits[G:G + n], want.view(np.int32)
        bad = got != wb
        if free_nan is not None:
            bad &= ~(free_nan.reshape(-1) & np.isnan(got.view(F32)))
        if bad.any():
            i = np.flatnonzero(bad)
            unwritten = int((got[i] == FILL).sum())
            raise AssertionError(f"{name}: {i.size} of {n} words differ ({unwritten} never written); first at {i[:8].tolist()}: "
                                 f"got {got.view(want.dtype)[i[:8]].tolist()} want {want[i[:8]].tolist()}")


# ---- strided sources inside random pools -----------------------------------------------------------------------------------
class Src:
    """A view of `shape` / `strides` (elements) at element `off` of a random pool: .ref the logical values (contiguous NumPy), .t
    the device view.  kind: "f32" (normal values, a few -0.0 and, with nans, payload NaNs), "bool" (bytes 0 / 1)."""
    def __init__(self, rng, shape, strides, off, kind="f32", nans=False, edit=None):
        span = off + sum((s - 1) * st for s, st in zip(shape, strides)) + 1
        size = span + SLACK
        if kind == "bool":
            pool = (rng.random(size) < 0.5)
        else:
            pool = rng.standard_normal(size).astype(F32)
            pool[rng.integers(0, size, size // 40 + 1)] = -0.0
            if nans:
                pool.view(np.int32)[rng.integers(0, size, size // 40 + 1)] = PAYLOAD_NAN
        view = np.lib.stride_tricks.as_strided(pool[off:], shape, [st * pool.itemsize for st in strides])
        if edit is not None:
            edit(view)
        self.pool, self.ref = pool, np.ascontiguousarray(view)
        self.tpool = torch.from_numpy(pool).cuda()
        self.t = torch.as_strided(self.tpool, shape, strides, off)

    def unchanged(self):
        a, b = self.tpool.cpu().numpy(), self.pool
        return np.array_equal(a.view(np.uint8), b.view(np.uint8))


COMBOS = [("pad", "00", "contig"), ("perm", "10", "T"), ("pad", "M1", "T")]      # (obs, rewards, dones) layouts
COMBO_IDS = ["-".join(c) for c in COMBOS]


def _obs_layout(pat, N, M, D):
    if pat == "pad":                                       # padding between agents and between threads, base 12 bytes into the pool
        sm = D + 3
        return (M * sm + 5, sm), 3
    sn = D + 1                                             # "perm": agent-major storage, stride_n < stride_m
    return (sn, N * sn + 2), 1


def _rew_layout(pat, N, M):
    return {"00": ((0, 0), 5), "10": ((1, 0), 2), "M1": ((M, 1), 7)}[pat]


def _done_layout(pat, N, M):
    return {"contig": ((M, 1), 3), "T": ((1, N), 1)}[pat]


def _mpe_sources(rng, N, M, D, combo, nans, done_edit=None):
    (osn, osm), ooff = _obs_layout(combo[0], N, M, D)
    rst, roff = _rew_layout(combo[1], N, M)
    dst, doff = _done_layout(combo[2], N, M)
    obs = Src(rng, (N, M, D), (osn, osm, 1), ooff, nans=nans)
    rew = Src(rng, (N, M), rst, roff, nans=nans)
    done = Src(rng, (N, M), dst, doff, kind="bool", edit=done_edit)
    assert obs.t.stride() == (osn, osm, 1) and rew.t.stride() == rst and done.t.stride() == dst
    if combo[0] == "pad":
        assert obs.t.data_ptr() % 16 != 0 and osm > D
    else:
        assert osn < osm
    return obs, rew, done


def _states(rng, R, H, keep_rows):
    """[R, 1, H] states with -0.0, +-inf, NaN and negative values: sprinkled at random, and four of them at the head of the first
    row that is reset and of the first that is kept.  Returns (Src, mask of the elements whose product with keep is an invalid
    operation)."""
    specials = np.array([-0.0, np.inf, -np.inf, np.nan, -1.5], dtype=F32)
    reset, kept = np.flatnonzero(keep_rows == 0), np.flatnonzero(keep_rows == 1)
    assert R < 8 or (reset.size and kept.size)

    def edit(v):
        flat = v.reshape(-1)
        idx = rng.permutation(flat.size)[:flat.size // 5]
        flat[idx] = specials[np.arange(idx.size) % specials.size]
        for rows in (reset, kept):
            if rows.size:
                v[rows[0], 0, :4] = specials[[0, 1, 3, 4]]
    s = Src(rng, (R, 1, H), (H, H, 1), 8, edit=edit)
    assert s.t.is_contiguous() and s.t.data_ptr() % 16 == 0
    for rows in (reset, kept):
        if rows.size:
            sub = s.ref[rows]
            assert np.isinf(sub).any() and np.isnan(sub).any() and (np.signbit(sub) & (sub == 0)).any()
    return s, np.isinf(s.ref) & (keep_rows == 0).reshape(R, 1, 1)


def _force_both(view):
    """dones with the first row set and the last clear (where there are two)."""
    if view.size >= 2:
        view[(0,) * view.ndim] = True
        view[(-1,) * view.ndim] = False


# ---- Python mirror of the launch geometry (no GPU) ------------------------------------------------------------------------------
CAP_INSERT, CAP_ROWS, NUM_CU = 2048 * 256, 4096 * 256, 256


def _passes(total, cap):
    return -(-total // min(cap, -(-total // 256) * 256))


MPE_CASES = [(1, 1, 1, F_), (1, 1, 1, T_), (1, 3, 18, F_), (1, 3, 18, T_), (37, 1, 7, F_), (37, 1, 7, T_), (5, 8, 64, F_), (5, 8, 64, T_),
             (700, 5, 31, T_), (2100, 5, 51, F_)]
RNN_CASES = [(1, 1, 1, F_, 4), (1, 3, 18, T_, 128), (37, 1, 7, T_, 64), (5, 8, 64, T_, 4), (4100, 8, 4, F_, 64)]
SMAC_BASE = (9, 3, 30, 48, 9, 64)
SMAC_CASES = [SMAC_BASE + (a, b, r, i % 3) for i, (a, b, r) in enumerate((a, b, r) for a in (T_, F_) for b in (T_, F_) for r in (T_, F_))] + [
    (1, 1, 1, 1, 1, 4, T_, T_, T_, 0), (1, 1, 1, 1, 1, 4, F_, F_, F_, 1),
    (37, 5, 7, 5, 40, 64, T_, T_, T_, 1), (37, 5, 7, 5, 40, 64, T_, F_, F_, 2),
    (500, 8, 100, 140, 9, 64, T_, T_, T_, 2), (500, 8, 100, 140, 9, 64, F_, F_, F_, 1)]
SMAC_PATS = [("M1", "contig"), ("00", "T"), ("10", "T")]                          # (rewards, dones) layouts
STEP_CASES = [  # (N, M, D, centralized, combo, kind)
    (1, 1, 4, F_, 0, "plain"), (1, 1, 4, T_, 1, "plain"), (37, 3, 18, T_, 0, "plain"), (37, 3, 18, F_, 1, "plain"), (37, 3, 18, T_, 2, "plain"),
    (700, 5, 12, T_, 0, "plain"), (700, 5, 12, T_, 1, "plain"), (37, 3, 130, F_, 0, "plain"), (5, 3, 130, T_, 1, "plain"),
    (37, 3, 18, T_, 1, "md"), (37, 3, 18, F_, 2, "md"), (37, 3, 18, F_, 2, "values"), (700, 5, 12, T_, 2, "values")]
REC_CASES = [(D, S, A, N, M, both) for (D, S, A) in ((30, 48, 9), (176, 322, 18)) for (N, M) in ((1, 1), (37, 3)) for both in (T_, F_)]
EPISODE_SHAPES = [(1, 1, 1, 4), (3, 7, 3, 18), (25, 2, 3, 18), (2, 300, 3, 18)]
ROWS_CASES = [(5, 1, 1, 1, 1, 1), (10, 3, 2, 10, 2, 2), (7, 5, 2, 3, 23, 1), (25, 4, 3, 10, 4, 2), (400, 100, 3, 10, 2, 9)]


def _episode_waves(T, N, M, lds):
    """Waves that share the episode insert (mappo_rollout_episode's geometry at its defaults)."""
    tiles = (N * M + 15) // 16
    ia, ic = T * tiles, (T + 1) * tiles
    if lds:
        return min(NUM_CU, -(-ia // 16) + -(-ic // 16)) * 16
    n_net, best, wa = 4 * NUM_CU, None, 1
    for a in range(1, n_net):
        l = max(-(-ia // a) * 150, -(-ic // (n_net - a)) * 134)
        if best is None or l < best:
            best, wa = l, a
    return min(wa, ia) + min(n_net - wa, ic)


def test_case_lists_cross_the_caps():
    mpe = {(N, M, D, c): N * M * (M * D if c else D) for N, M, D, c in MPE_CASES}
    assert mpe[(700, 5, 31, T_)] == 542500 and mpe[(2100, 5, 51, F_)] == 535500
    assert sorted(_passes(v, CAP_INSERT) for v in mpe.values())[-3:] == [1, 2, 2]
    assert all(v % CAP_INSERT for v in mpe.values())                                   # ragged second pass
    grid_by = {(N, M, D, c, H): ("state" if N * M * (H // 4) > N * M * (M * D if c else D) else "copy") for N, M, D, c, H in RNN_CASES}
    assert grid_by[(37, 1, 7, T_, 64)] == "state" and grid_by[(5, 8, 64, T_, 4)] == "copy" and grid_by[(4100, 8, 4, F_, 64)] == "state"
    assert 4100 * 8 * 16 == 524800 > CAP_INSERT and {c[4] for c in RNN_CASES} == {4, 64, 128}
    assert {c[6:9] for c in SMAC_CASES if c[:6] == SMAC_BASE} == {(a, b, r) for a in (T_, F_) for b in (T_, F_) for r in (T_, F_)}
    N, M, D, S, A, H = 37, 5, 7, 5, 40, 64
    assert A > max(D, S) and N * M * A > -(-N * M * max(D, S) // 256) * 256             # the availability copy needs the stride loop
    assert 500 * 8 * 140 == 560000 > CAP_INSERT
    assert {p for c in SMAC_CASES for p in SMAC_PATS[c[9]]} == {"M1", "00", "10", "contig", "T"}
    big = 700 * 5 * 60
    assert -(-big // 2048) == 103 <= NUM_CU and _passes(big, 103 * 256) == 8
    assert {k for *_, k in STEP_CASES} == {"plain", "md", "values"} and any(c[2] > 64 for c in STEP_CASES)
    for T, N, M, D in EPISODE_SHAPES:
        for cen in (T_, F_):
            total = T * N * M * (M * D if cen else D)
            assert total < 2 ** 32
            for lds, U in ((T_, 4), (F_, 16)):
                assert total % (U * _episode_waves(T, N, M, lds) * 64), (T, N, M, D, cen, lds)
    rows = {c: c[5] * c[4] * ((c[0] * c[1] * c[2] // c[3]) // c[4]) * c[3] for c in ROWS_CASES}
    assert rows[(400, 100, 3, 10, 2, 9)] == 1080000 > CAP_ROWS and max(v for c, v in rows.items() if c[0] != 400) < CAP_ROWS
    assert (25 * 4 * 3 // 10) % 4 == 2 and (7 * 5 * 2 // 3) // 23 == 1


# ---- 1. mappo_insert_mpe -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("N,M,D,cen", MPE_CASES)
def test_insert_mpe_matrix(ops, N, M, D, cen, combo):
    rng = _rng("mpe", N, M, D, cen, combo)
    obs, rew, done = _mpe_sources(rng, N, M, D, combo, nans=True, done_edit=_force_both)
    S = M * D if cen else D
    sl = Slots()
    od, sd, rd, md = sl.new("obs", N, M, D), sl.new("share_obs", N, M, S), sl.new("rewards", N, M, 1), sl.new("masks", N, M, 1)
    ops.insert_mpe(obs.t, rew.t, done.t, od, sd, rd, md, cen)
    torch.cuda.synchronize()
    for name, want in zip(("obs", "share_obs", "rewards", "masks"), insert_mpe_ref(obs.ref, rew.ref, done.ref, cen)):
        sl.check(name, want)
    assert obs.unchanged() and rew.unchanged() and done.unchanged()


# ---- 2. mappo_insert_mpe_rnn -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("N,M,D,cen,H", RNN_CASES)
def test_insert_mpe_rnn_matrix(ops, N, M, D, cen, H, combo):
    rng = _rng("rnn", N, M, D, cen, H, combo)
    obs, rew, done = _mpe_sources(rng, N, M, D, combo, nans=True, done_edit=_force_both)
    keep = 1 - done.ref.reshape(N * M).astype(np.int64)
    ha, free_a = _states(rng, N * M, H, keep)
    hc, free_c = _states(rng, N * M, H, keep)
    S = M * D if cen else D
    sl = Slots()
    od, sd, rd, md = sl.new("obs", N, M, D), sl.new("share_obs", N, M, S), sl.new("rewards", N, M, 1), sl.new("masks", N, M, 1)
    da, dc = sl.new("rnn_states", N, M, 1, H), sl.new("rnn_states_critic", N, M, 1, H)
    ops.insert_mpe_rnn(obs.t, rew.t, done.t, od, sd, rd, md, cen, ha.t, hc.t, da, dc)
    torch.cuda.synchronize()
    want = insert_mpe_ref(obs.ref, rew.ref, done.ref, cen, rnn=(ha.ref, hc.ref))
    for name, w, free in zip(("obs", "share_obs", "rewards", "masks", "rnn_states", "rnn_states_critic"), want, (None,) * 4 + (free_a, free_c)):
        sl.check(name, w, free)
    assert obs.unchanged() and rew.unchanged() and done.unchanged() and ha.unchanged() and hc.unchanged()


# ---- 3. mappo_insert_smac --------------------------------------------------------------------------------------------------
def _smac_dones(N, M):
    """edit(view): env n gets every agent done (n % 3 == 0), none (1) or some (2: the first done, the last not)."""
    def edit(v):
        for n in range(N):
            if n % 3 == 0:
                v[n, :] = True
            elif n % 3 == 1:
                v[n, :] = False
            else:
                v[n, 0], v[n, -1] = True, False
    return edit


def _smac_sources(rng, N, M, D, S, A, H, with_avail, with_bad, with_rnn, pat, nans):
    rpat, dpat = SMAC_PATS[pat]
    rst, roff = _rew_layout(rpat, N, M)
    dst, doff = _done_layout(dpat, N, M)
    contig = lambda *s: tuple(int(np.prod(s[i + 1:])) for i in range(len(s)))
    obs = Src(rng, (N, M, D), contig(N, M, D), 3, nans=nans)
    share = Src(rng, (N, M, S), contig(N, M, S), 1, nans=nans)
    avail = Src(rng, (N, M, A), contig(N, M, A), 5, kind="bool") if with_avail else None
    rew = Src(rng, (N, M), rst, roff, nans=nans)
    done = Src(rng, (N, M), dst, doff, kind="bool", edit=_smac_dones(N, M) if M >= 2 else None)
    bad = Src(rng, (N, M), (M, 1), 3, kind="bool") if with_bad else None
    if N >= 3 and M >= 2:
        n_done = done.ref.sum(axis=1)
        assert (n_done == M).any() and (n_done == 0).any() and ((n_done > 0) & (n_done < M)).any()
    return obs, share, avail, rew, done, bad


def _avail_f32(avail):
    """Availability as the float32 0 / 1 words the kernels copy, on a pool of its own (action 0 always available)."""
    if avail is None:
        return None, None
    ref = avail.ref.astype(F32)
    ref[..., 0] = 1.0
    pool = torch.full((ref.size + 5 + SLACK,), 0.5, device="cuda")
    pool[5:5 + ref.size] = torch.from_numpy(ref.reshape(-1)).cuda()
    return ref, pool[5:5 + ref.size].view(*ref.shape)


SLOT_NAMES = ("obs", "share_obs", "available_actions", "rewards", "masks", "bad_masks", "active_masks", "rnn_states", "rnn_states_critic")


def _smac_slots(sl, N, M, D, S, A, H, with_avail, with_rnn):
    shapes = dict(obs=(N, M, D), share_obs=(N, M, S), available_actions=(N, M, A), rewards=(N, M, 1), masks=(N, M, 1), bad_masks=(N, M, 1),
                  active_masks=(N, M, 1), rnn_states=(N, M, 1, H), rnn_states_critic=(N, M, 1, H))
    absent = (() if with_avail else ("available_actions",)) + (() if with_rnn else ("rnn_states", "rnn_states_critic"))
    return {k: (None if k in absent else sl.new(k, *shapes[k])) for k in SLOT_NAMES}


@gpu
@pytest.mark.parametrize("N,M,D,S,A,H,with_avail,with_bad,with_rnn,pat", SMAC_CASES)
def test_insert_smac_matrix(ops, N, M, D, S, A, H, with_avail, with_bad, with_rnn, pat):
    rng = _rng("smac", N, M, D, S, A, H, with_avail, with_bad, with_rnn, pat)
    obs, share, avail, rew, done, bad = _smac_sources(rng, N, M, D, S, A, H, with_avail, with_bad, with_rnn, pat, nans=True)
    av_ref, av_t = _avail_f32(avail)
    keep = np.repeat(~done.ref.all(axis=1), M).astype(np.int64)
    ha = hc = free_a = free_c = None
    if with_rnn:
        ha, free_a = _states(rng, N * M, H, keep)
        hc, free_c = _states(rng, N * M, H, keep)
    sl = Slots()
    d = _smac_slots(sl, N, M, D, S, A, H, with_avail, with_rnn)
    ops.insert_smac(obs.t, share.t, av_t, rew.t, done.t, bad.t if bad else None, ha.t if ha else None, hc.t if hc else None, d["obs"],
                    d["share_obs"], d["available_actions"], d["rewards"], d["masks"], d["bad_masks"], d["active_masks"], d["rnn_states"],
                    d["rnn_states_critic"])
    torch.cuda.synchronize()
    want = insert_smac_ref(obs.ref, share.ref, av_ref, rew.ref, done.ref, bad.ref if bad else None, (ha.ref, hc.ref) if with_rnn else None)
    for name, w, free in zip(SLOT_NAMES, want, (None,) * 7 + (free_a, free_c)):
        assert (w is None) == (d[name] is None), name
        if w is not None:
            sl.check(name, w, free)
    assert all(s.unchanged() for s in (obs, share, rew, done, bad, ha, hc) if s is not None)


# ---- 4a. insert_mpe_body as a role of mappo_rollout_step / mappo_rollout_step_md ---------------------------------------------------
@gpu
@pytest.mark.parametrize("N,M,D,cen,combo,kind", STEP_CASES)
def test_rollout_step_insert_role(ops, N, M, D, cen, combo, kind):
    """Only the slot arrays and the guards: the networks (tiny random ones) are test_gpu_rollout_matrix.py's business.  A centralized
    critic reads M D consecutive words from each thread's first row, which with padded or permuted agents is not the share row, but
    stays inside the pool."""
    rng = _rng("step", N, M, D, cen, combo, kind)
    obs, rew, done = _mpe_sources(rng, N, M, D, COMBOS[combo], nans=False, done_edit=_force_both)
    B, S = N * M, (M * D if cen else D)
    heads = (3, 3)
    A = sum(heads) if kind == "md" else 5
    da, dc = ops.net_desc(D, A), ops.net_desc(S, 1)
    tg = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
    pa = torch.randn(ops.net_param_count(da), device="cuda", generator=tg) * 0.1
    pc = torch.randn(ops.net_param_count(dc), device="cuda", generator=tg) * 0.1
    sl = Slots()
    ins = dict(obs_dst=sl.new("obs", N, M, D), share_dst=sl.new("share_obs", N, M, S), rewards=(rew.t, *rew.t.stride()),
               dones=(done.t, *done.t.stride()), rew_dst=sl.new("rewards", N, M, 1), mask_dst=sl.new("masks", N, M, 1), centralized=cen)
    K = len(heads) if kind == "md" else 1
    act, lp = (None, None) if kind == "values" else (sl.new("actions", B, K), sl.new("logp", B, K))
    val = sl.new("values", B)
    o = (obs.t, obs.t.stride(0), obs.t.stride(1))
    s = (obs.t, obs.t.stride(0), 0 if cen else obs.t.stride(1))
    if kind == "md":
        ops.rollout_step_md(pa, da, pc, dc, o, s, M, B, heads, False, 11, 3, None, act, lp, val, ins)
    else:
        ops.rollout_step(pa, da, pc, dc, o, s, M, B, None, False, 11, 3, None, act, lp, val, ins)
    torch.cuda.synchronize()
    for name, want in zip(("obs", "share_obs", "rewards", "masks"), insert_mpe_ref(obs.ref, rew.ref, done.ref, cen)):
        sl.check(name, want)
    for name in ("values",) + (() if kind == "values" else ("actions", "logp")):
        sl.check(name)
        pool, n = sl.pools[name]
        assert (pool[G:G + n] != FILL).all(), f"{name}: rows left unwritten"
    assert obs.unchanged() and rew.unchanged() and done.unchanged()


# ---- 4b. insert_smac_body as a role of mappo_recurrent_rollout_step -----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("D,S,A,N,M,both", REC_CASES)
def test_recurrent_rollout_step_insert_role(ops, D, S, A, N, M, both):
    rng = _rng("rec", D, S, A, N, M, both)
    pat = 1 if both else 2
    obs, share, avail, rew, done, bad = _smac_sources(rng, N, M, D, S, A, 64, both, both, True, pat, nans=False)
    av_ref, av_t = _avail_f32(avail)
    B = N * M
    keep = np.repeat(~done.ref.all(axis=1), M).astype(np.int64)

    def finite_states():
        def edit(v):
            v.reshape(-1)[::7] = -0.0
        return Src(rng, (B, 1, 64), (64, 64, 1), 8, edit=edit)
    ha, hc = finite_states(), finite_states()
    da, dc = ops.net_desc(D, A, recurrent=True), ops.net_desc(S, 1, recurrent=True)
    tg = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
    pa = torch.randn(ops.net_param_count(da), device="cuda", generator=tg) * 0.1
    pc = torch.randn(ops.net_param_count(dc), device="cuda", generator=tg) * 0.1
    sl = Slots()
    slot = _smac_slots(sl, N, M, D, S, A, 64, both, True)
    han, hcn = sl.new("actor_h_next", B, 1, 64), sl.new("critic_h_next", B, 1, 64)
    act, lp, val = sl.new("actions", B), sl.new("logp", B), sl.new("values", B)
    ops.recurrent_rollout_step(pa, da, pc, dc, obs.t, share.t, av_t, rew.t, done.t, bad.t if bad else None, ha.t, hc.t, han, hcn, False, 11, 3,
                               None, act, lp, val, {k: v for k, v in slot.items() if v is not None})
    torch.cuda.synchronize()
    want = insert_smac_ref(obs.ref, share.ref, av_ref, rew.ref, done.ref, bad.ref if bad else None, (ha.ref, hc.ref))
    for name, w in zip(SLOT_NAMES, want):
        assert (w is None) == (slot[name] is None), name
        if w is not None:
            sl.check(name, w)
    for name in ("actor_h_next", "critic_h_next", "actions", "logp", "values"):
        sl.check(name)
        pool, n = sl.pools[name]
        assert (pool[G:G + n] != FILL).all(), f"{name}: rows left unwritten"
    assert all(s.unchanged() for s in (obs, share, rew, done, bad, ha, hc) if s is not None)


# ---- 5. the whole-episode insert of mappo_rollout_episode ---------------------------------------------------------------------------
EPISODE_ENV = ("MAPPO_EPISODE_WAVES", "MAPPO_EPISODE_NET_WAVES", "MAPPO_EPISODE_INS_WAVES", "MAPPO_EPISODE_COST_A", "MAPPO_EPISODE_LDS",
               "MAPPO_EPISODE_LDS_WAVES", "MAPPO_EPISODE_LDS_ACTOR_WGS")


@gpu
@pytest.mark.parametrize("lds", [0, 1], ids=["registers", "lds"])
@pytest.mark.parametrize("layer_N", [0, 1])
@pytest.mark.parametrize("cen", [T_, F_], ids=["centralized", "local"])
@pytest.mark.parametrize("T,N,M,D", EPISODE_SHAPES)
def test_rollout_episode_insert(ops, monkeypatch, T, N, M, D, cen, layer_N, lds):
    from mappo_amd import _lib
    for k in EPISODE_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MAPPO_EPISODE_LDS", str(lds))
    assert _lib.load().mappo_rollout_episode_uses_lds(layer_N) == lds
    rng = _rng("episode", T, N, M, D, cen, layer_N, lds)
    B, S = N * M, (M * D if cen else D)
    # an interior slice of a [T][N][row + pad] block; a centralized critic reads the thread's agents side by side, so they are D apart
    sm = D if cen else D + 1
    sn = M * sm + 3
    env = Src(rng, (T, N, M, D), (N * sn + 7, sn, sm, 1), 3)
    rew = Src(rng, (T, N, M), (N + 2, 1, 0), 2)
    done = Src(rng, (T, N, M), (B + 5, M, 1), 3, kind="bool", edit=_force_both)
    assert done.t.stride(0) != B and env.t.data_ptr() % 16 != 0
    da, dc = ops.net_desc(D, 5, layer_N), ops.net_desc(S, 1, layer_N)
    tg = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
    pa = torch.randn(ops.net_param_count(da), device="cuda", generator=tg) * 0.1
    pc = torch.randn(ops.net_param_count(dc), device="cuda", generator=tg) * 0.1
    sl = Slots()
    obs_buf, share_buf, mask_buf = sl.new("obs", T + 1, B, D), sl.new("share_obs", T + 1, B, S), sl.new("masks", T + 1, B)
    rew_buf = sl.new("rewards", T, B)
    slot0 = [rng.standard_normal(s).astype(F32) for s in ((B, D), (B, S), (B,))]
    for buf, s0 in zip((obs_buf, share_buf, mask_buf), slot0):
        buf[0] = torch.from_numpy(s0).cuda()
    act, lp, val, nxt = sl.new("actions", T, B), sl.new("logp", T, B), sl.new("values", T, B), sl.new("next_values", B)
    ops.rollout_episode(pa, da, pc, dc, env.t, rew.t, done.t, False, 11, 3, None, obs_buf, share_buf, rew_buf, mask_buf, act, lp, val, nxt, cen)
    torch.cuda.synchronize()
    o, s, r, m = episode_insert_ref(env.ref, rew.ref, done.ref, cen)
    sl.check("obs", np.concatenate([slot0[0].reshape(-1), o.reshape(-1)]))            # slot 0 unchanged, slots 1 .. T the env output
    sl.check("share_obs", np.concatenate([slot0[1].reshape(-1), s.reshape(-1)]))
    sl.check("masks", np.concatenate([slot0[2].reshape(-1), m.reshape(-1)]))
    sl.check("rewards", r)
    for name in ("actions", "logp", "values", "next_values"):
        sl.check(name)
        pool, n = sl.pools[name]
        assert (pool[G:G + n] != FILL).all(), f"{name}: rows left unwritten"
    assert env.unchanged() and rew.unchanged() and done.unchanged()


# ---- 6. mappo_recurrent_rows -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("T,N,M,L,nmb,E", ROWS_CASES)
def test_recurrent_rows_matrix(ops, T, N, M, L, nmb, E):
    from mappo_amd import _lib
    rng = _rng("rows", T, N, M, L, nmb, E)
    R = N * M
    chunks = (T * R) // L
    mbs = chunks // nmb
    perm = np.stack([rng.permutation(chunks) for _ in range(E)]).astype(np.int64)
    tperm = torch.from_numpy(perm).cuda()
    sl = Slots()
    rows, h0 = sl.new("rows", E, nmb, L * mbs, dtype=torch.int32), sl.new("h0_rows", E, nmb, mbs, dtype=torch.int32)
    rc = _lib.load().mappo_recurrent_rows(C.c_void_p(tperm.data_ptr()), E, chunks, L, T, R, nmb, C.c_void_p(rows.data_ptr()),
                                          C.c_void_p(h0.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "mappo_recurrent_rows")
    torch.cuda.synchronize()
    want_rows, want_h0 = np.empty((E, nmb, L * mbs), np.int32), np.empty((E, nmb, mbs), np.int32)
    for e in range(E):
        want = O.recurrent_rows(T, R, nmb, L, perm[e])
        assert len(want) == nmb
        for k, (r, h) in enumerate(want):
            want_rows[e, k], want_h0[e, k] = r, h
    sl.check("rows", want_rows)
    sl.check("h0_rows", want_h0)
    got_rows, got_h0 = rows.cpu().numpy(), h0.cpu().numpy()
    for e in range(E):
        np.testing.assert_array_equal(got_h0[e], got_rows[e][..., :mbs])
        left = perm[e][nmb * mbs:]                                                   # chunks no minibatch takes: their rows appear nowhere
        q = (left[:, None] * L + np.arange(L)[None, :]).reshape(-1)
        assert not np.isin((q % T) * R + q // T, got_rows[e]).any()
        assert np.unique(got_rows[e]).size == got_rows[e].size
    if (T, nmb) == (25, 4):
        assert chunks - nmb * mbs == 2
    assert np.array_equal(tperm.cpu().numpy(), perm)
