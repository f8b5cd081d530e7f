"""Edge shapes of the small kernels every trainer iteration runs: returns (gae.hip), statistics (stats.hip / stats_core.h,
vn_stats in common.h), the stand-alone PPO loss (ppo_loss.hip) and slab reduction + clip + Adam (optim.hip), each against a
float64 reference of the same operation.

test_case_lists_cover_every_path needs no GPU: it mirrors the host geometry of the launches in Python and asserts that the case
lists below reach every path the kernels can take (empty scan segment, one full chunk, a one-step last chunk, grid caps, empty and
ragged slab quarters, > 256 norm partials, every segment count, every (rows, avail) pair).  Removing the case that covers a path
makes it fail.

Tolerances are stated where they are used; none is fitted to the kernels' output.  Measured on the MI355X: returns within 1.3 x err32
of float64 (4 x allowed), advantages within 0.75 of their 2-ulp bound, normalised advantages within 0.78 of their tolerance."""
import math

import numpy as np
import pytest
import torch

from oracle import mappo_oracle as O
from test_gpu_kernels import close, close_rel_max, dev

gpu = pytest.mark.gpu
F32, F64 = np.float32, np.float64
NAN = float("nan")


# ---- Python mirror of the host geometry ----------------------------------------------------------------------------
GAE_LMAX, GAE_SMAX, WAVE = 16, 16, 64
STAT_BLOCK, STAT_MAX_BLOCKS = 256, 1024
PL_BLOCK, PL_MAX_GRID, MAX_ACTIONS = 256, 2048, 32
SLAB_BLOCK, SLAB_Q, SLAB_BATCH, OPT_BLOCK = 128, 4, 16, 256


def gae_geometry(T):
    """(S, Lseg, chunk) of mappo_gae_scan."""
    S = max(1, min(GAE_SMAX, (T + 7) // 8))
    Lseg = min(GAE_LMAX, (T + S - 1) // S)
    return S, Lseg, S * Lseg


def gae_chunks(T):
    """Per chunk, last chunk first (the order the block walks them): the segment length of every wave."""
    S, Lseg, chunk = gae_geometry(T)
    out = []
    for base in range(((T - 1) // chunk) * chunk, -1, -chunk):
        out.append([max(0, min(T, base + s * Lseg + Lseg) - (base + s * Lseg)) for s in range(S)])
    return out


def gae_workgroups(R):
    return (R + WAVE - 1) // WAVE


def stat_blocks(n):
    return max(1, min(STAT_MAX_BLOCKS, (n + STAT_BLOCK * 4 - 1) // (STAT_BLOCK * 4)))


def stat_trips(n):
    """Trips of the busiest thread's grid-stride loop in the statistics kernels (4 by design below the grid cap)."""
    return -(-n // (stat_blocks(n) * STAT_BLOCK))


def pl_blocks(B):
    return max(1, min(PL_MAX_GRID, (B + PL_BLOCK - 1) // PL_BLOCK))


def pl_trips(B):
    return -(-((B + PL_BLOCK - 1) // PL_BLOCK) // pl_blocks(B))


def pl_av_lds(with_rows, with_avail):
    return with_avail and not with_rows


def pl_lds_bytes(A, with_rows, with_avail):
    return (2 if pl_av_lds(with_rows, with_avail) else 1) * PL_BLOCK * A * 4


def slab_quarters(n_slabs):
    return [(q * n_slabs // SLAB_Q, (q + 1) * n_slabs // SLAB_Q) for q in range(SLAB_Q)]


def seg_partials(sizes):
    return [s // SLAB_BLOCK for s in sizes]


# ---- the case lists ----------------------------------------------------------------------------------------------------
# (T, R): every T and every R in a sparse cross.  err32 = max |fp32 oracle - float64 oracle| on this file's data, the largest over the four
# branches and the four ValueNorm states (returns reach |17|); the test recomputes it per branch and state, where it goes down to 0 for
# the series whose returns are exact in fp32 (R = 1 without ValueNorm):
GAE_CASES = [
    (8, 1),      # err32 8.9e-07   one wave, full segment
    (8, 130),    #       1.6e-06
    (9, 64),     #       2.3e-06   two waves
    (9, 65),     #       2.2e-06
    (129, 1),    #       2.7e-07   Lseg = 9: wave 15 starts past T
    (129, 65),   #       4.0e-06
    (256, 64),   #       3.8e-06   exactly one full chunk
    (256, 130),  #       4.4e-06
    (257, 1),    #       1.8e-06   second chunk of one step
    (257, 65),   #       4.0e-06
    (513, 64),   #       4.2e-06   three chunks, the last of one step
    (513, 130),  #       5.2e-06
]
VN_STATES = ["running", "zero", "one_update", None]

ADV_N = [1, 255, 1024, 1025, 1024 * 1024 + 5]
ADV_VARIANTS = ["constant", "one_active", "offset_returns", "zero_state"]       # at n = 4099
MBM_B = [1, 1024 * 1024 + 5]
VN_UPDATE_N = [1, 10, 15]

LOSS_SHAPES = [(777, 5), (300, 32)]
LOSS_PAIRS = [(False, False), (False, True), (True, False), (True, True)]       # (with_rows, with_avail)
LOSS_STRIDE_B = PL_MAX_GRID * PL_BLOCK + 257
MISALIGNED = [("logits",), ("avail",), ("dlogits",), ("logits", "avail", "dlogits")]

ADAM_LAYOUTS = {1: [256], 2: [512, 256], 3: [256, 33024, 512], 4: [256, 512, 256, 768]}
ADAM_VARIANTS = ["plain", "weight_decay", "no_clip_seg2", "seg1_disabled", "zero_grad", "huge_grad", "step_100000"]
SLAB_N = [1, 2, 3, 4, 5, 63, 64, 67, 256]
SLAB_P = [1, 127, 129, 300]
RCA_N = [3, 67]


def test_case_lists_cover_every_path():
    """Every path named in this file's docstring is reached by at least one listed case (no GPU needed)."""
    chunks = {T: gae_chunks(T) for T, _ in GAE_CASES}
    geo = {T: gae_geometry(T) for T, _ in GAE_CASES}
    assert any(0 in c[-1] and len(c) == 1 for c in chunks.values()), "gae: an empty segment inside a single chunk"
    assert any(len(c) == 1 and all(l == geo[T][1] for l in c[0]) and geo[T][0] == GAE_SMAX and geo[T][1] == GAE_LMAX
               for T, c in chunks.items()), "gae: exactly one full chunk"
    assert any(len(c) >= 2 and sum(c[0]) == 1 for c in chunks.values()), "gae: a last chunk of a single step"
    assert any(len(c) >= 3 for c in chunks.values()), "gae: three chunks (the carry crosses two boundaries)"
    assert any(geo[T][0] == 1 and chunks[T] == [[geo[T][1]]] for T in chunks), "gae: one wave with a full segment"
    assert any(geo[T][0] == 2 for T in chunks), "gae: two waves"
    assert {gae_workgroups(R) for _, R in GAE_CASES} >= {1, 2, 3} and {1, 64, 65} <= {R for _, R in GAE_CASES}, "gae: R edges"
    assert {T for T, _ in GAE_CASES} == {8, 9, 129, 256, 257, 513} and {R for _, R in GAE_CASES} == {1, 64, 65, 130}
    assert {(T, gae_workgroups(R) > 1) for T, R in GAE_CASES} == {(T, many) for T in chunks for many in (False, True)}, \
        "gae: every segment geometry with one workgroup and with several (the last one ragged)"
    # statistics: one thread, one block ragged / full, two blocks, the grid cap (a fifth trip of the grid-stride loop)
    for lst, what in ((ADV_N, "adv_moments"), (MBM_B, "minibatch_moments")):
        assert any(n == 1 for n in lst), what + ": n = 1"
        assert any(stat_blocks(n) == STAT_MAX_BLOCKS and stat_trips(n) > 4 for n in lst), what + ": grid cap, extra trip"
    assert any(stat_blocks(n) == 1 and n > 1 and n % STAT_BLOCK for n in ADV_N) and any(n == STAT_BLOCK * 4 for n in ADV_N)
    assert any(stat_blocks(n) == 2 for n in ADV_N), "adv_moments: second block"
    assert set(ADV_VARIANTS) == {"constant", "one_active", "offset_returns", "zero_state"}
    assert set(VN_UPDATE_N) == {1, 10, 15}
    # loss
    assert {(r, a) for r, a in LOSS_PAIRS} == {(False, False), (False, True), (True, False), (True, True)}, "loss: (rows, avail) pairs"
    assert any(pl_lds_bytes(A, r, a) == 2 * PL_BLOCK * MAX_ACTIONS * 4 for _, A in LOSS_SHAPES for r, a in LOSS_PAIRS), "loss: 64 KiB launch"
    assert any(A <= 8 for _, A in LOSS_SHAPES) and any(A > 8 for _, A in LOSS_SHAPES), "loss: register and LDS softmax"
    assert all((B % PL_BLOCK) * A % 4 for B, A in LOSS_SHAPES[:1]), "loss: scalar tail of the 16-byte copy"
    assert pl_trips(LOSS_STRIDE_B) >= 2 and pl_blocks(LOSS_STRIDE_B) == PL_MAX_GRID, "loss: grid-stride second trip"
    assert {m for ms in MISALIGNED for m in ms if len(ms) == 1} == {"logits", "avail", "dlogits"} and any(len(ms) == 3 for ms in MISALIGNED)
    # optimiser
    assert set(ADAM_LAYOUTS) == {1, 2, 3, 4} and all(len(v) == k for k, v in ADAM_LAYOUTS.items()), "adam: every n_seg"
    assert all(s % OPT_BLOCK == 0 for v in ADAM_LAYOUTS.values() for s in v)
    assert any(p > OPT_BLOCK for v in ADAM_LAYOUTS.values() for p in seg_partials(v)), "adam: a segment of more than 256 partials"
    assert max(seg_partials(ADAM_LAYOUTS[3])) > OPT_BLOCK and len(ADAM_LAYOUTS[3]) == 3
    assert set(ADAM_VARIANTS) == {"plain", "weight_decay", "no_clip_seg2", "seg1_disabled", "zero_grad", "huge_grad", "step_100000"}
    # slab reduction
    for lst, what in ((SLAB_N, "slab_reduce"), (RCA_N, "reduce_clip_adam")):
        q = {n: slab_quarters(n) for n in lst}
        assert any(any(hi == lo for lo, hi in v) for v in q.values()), what + ": an empty quarter"
        assert any(any(hi - lo > SLAB_BATCH and (hi - lo) % SLAB_BATCH for lo, hi in v) for v in q.values()), \
            what + ": a quarter with a full 16-row batch and a remainder"
    q = {n: slab_quarters(n) for n in SLAB_N}
    assert {sum(hi == lo for lo, hi in v) for v in q.values()} >= {1, 2, 3}, "slab_reduce: one, two and three empty quarters"
    assert any(all(hi - lo == 1 for lo, hi in v) for v in q.values()), "slab_reduce: one row per quarter"
    assert any({hi - lo for lo, hi in v} == {1, 2} for v in q.values()), "slab_reduce: quarters of one and of two rows"
    assert any(any(hi - lo == SLAB_BATCH - 1 for lo, hi in v) for v in q.values()), "slab_reduce: a quarter one row short of a batch"
    assert any(all(hi - lo == SLAB_BATCH for lo, hi in v) for v in q.values()), "slab_reduce: exactly one batch per quarter"
    assert any(len({hi - lo for lo, hi in v}) > 1 and min(hi - lo for lo, hi in v) >= SLAB_BATCH for v in q.values()), \
        "slab_reduce: quarters of unequal length"
    assert any(all((hi - lo) % SLAB_BATCH == 0 and hi - lo > SLAB_BATCH for lo, hi in v) for v in q.values()), "slab_reduce: several full batches"
    assert 1 in SLAB_P and any(1 < P < SLAB_BLOCK for P in SLAB_P) and any(P % SLAB_BLOCK == 1 and P > SLAB_BLOCK for P in SLAB_P)
    assert any(-(-P // SLAB_BLOCK) >= 3 and P % SLAB_BLOCK for P in SLAB_P), "slab_reduce: three workgroups, the last ragged"


@pytest.fixture(scope="module")
def ops(gpu_device):
    from mappo_amd import ops as _ops
    return _ops


# ---- ValueNorm states ------------------------------------------------------------------------------------------------
def vn_state(name):
    """fp32 [3] state: a running state, the all-zero state of iteration 0 (both clamps of vn_stats apply: sd = 0.1), the state after
    exactly one update (debiasing term ~ 1e-5, at its clamp), or None (no ValueNorm)."""
    if name is None:
        return None
    if name == "running":
        return np.array([0.7, 3.1, 0.8], F32)
    if name == "zero":
        return np.zeros(3, F32)
    if name == "one_update":
        vn = O.ValueNormRef()
        vn.update(np.random.default_rng(77).standard_normal((64, 1)).astype(F32) * 2 + 1)
        return vn.state()
    if name == "dyadic":                      # mean 1, sd 2, every operation of vn_stats exact in fp32
        return np.array([0.5, 2.5, 0.5], F32)
    raise KeyError(name)


def vn_mean_sd(state, dtype):
    """vn_stats (common.h) evaluated in `dtype`: debiasing term clamped at 1e-5, variance at 1e-2."""
    if state is None:
        return dtype(0), dtype(1)
    s = np.asarray(state, F32).astype(dtype)
    d = np.maximum(s[2], dtype(1e-5))
    mean, msq = s[0] / d, s[1] / d
    var = np.maximum(msq - mean * mean, dtype(1e-2))
    return dtype(mean), dtype(np.sqrt(var))


def vn_denorm(state, dtype):
    if state is None:
        return None
    mean, sd = vn_mean_sd(state, dtype)
    return lambda x: np.asarray(x, dtype) * sd + mean


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.int32), np.ascontiguousarray(b, F32).view(np.int32))


def all_nan(t):
    return bool(torch.isnan(t).all().item())


# ---- 1. returns ----------------------------------------------------------------------------------------------------------
GAMMA, LAMBDA = float(F32(0.99)), float(F32(0.95))          # the values the kernel receives (its ABI takes floats)
GUARD = 64


def _gae_data(T, R):
    rng = np.random.default_rng(T * 1000 + R)
    rewards = rng.standard_normal((T, R)).astype(F32)
    vp = rng.standard_normal((T + 1, R)).astype(F32)
    masks = (rng.random((T + 1, R)) > 0.1).astype(F32)
    bad = (rng.random((T + 1, R)) > 0.1).astype(F32)
    nv = rng.standard_normal(R).astype(F32)
    # one series with masks all 0, one with masks all 1, one with bad_masks all 0 (R == 1: one of the three, chosen by T)
    kinds = [0, 1, 2] if R >= 3 else [T % 3]
    for r, k in zip(range(R), kinds):
        if k == 0:
            masks[:, r] = 0
        elif k == 1:
            masks[:, r] = 1
        else:
            bad[:, r] = 0
    return rewards, vp, masks, bad, nv


@gpu
@pytest.mark.parametrize("T,R", GAE_CASES)
def test_gae_edge_shapes(ops, T, R):
    """gae_scan at the T that change the segment geometry and the R around one workgroup, all four branches and four ValueNorm states,
    against compute_returns_ref in float64.  Tolerance: rtol 1e-5 + atol 4 * err32, err32 the error of the same oracle run in fp32
    (the kernel composes per-segment affine maps, so its products associate differently from the step-by-step scan).  `returns` is
    NaN before the launch: every row < T must be written, slot T only in the discounted branches, and nothing past either array."""
    rewards, vp, masks, bad, nv = _gae_data(T, R)
    n = (T + 1) * R
    d_rw, d_mk, d_bm, d_nv = dev(rewards), dev(masks), dev(bad), dev(nv)
    SENT = F32(123.25)
    for name in VN_STATES:
        st = vn_state(name)
        d_st = dev(st) if st is not None else None
        for use_gae in (True, False):
            for ptl in (False, True):
                what = f"T={T} R={R} vn={name} gae={use_gae} ptl={ptl}"
                ref = O.compute_returns_ref(rewards.astype(F64), vp.astype(F64), masks.astype(F64), bad.astype(F64), nv.astype(F64),
                                            GAMMA, LAMBDA, use_gae, ptl, vn_denorm(st, F64))
                ref32 = O.compute_returns_ref(rewards, vp.copy(), masks, bad, nv, F32(GAMMA), F32(LAMBDA), use_gae, ptl, vn_denorm(st, F32))
                assert ref.dtype == F64 and ref32.dtype == F32
                err32 = float(np.abs(ref32[:T].astype(F64) - ref[:T]).max())
                ret_buf = torch.full((n + GUARD,), NAN, device="cuda")
                vp_buf = torch.full((n + GUARD,), NAN, device="cuda")
                vp_in = vp.copy(); vp_in[T] = SENT
                vp_buf[:n] = dev(vp_in).view(-1)
                ops.gae_scan(d_rw, vp_buf[:n].view(T + 1, R), d_nv, d_mk, d_bm if ptl else None, ret_buf[:n].view(T + 1, R), d_st,
                             GAMMA, LAMBDA, use_gae, ptl)
                ret, vpo = ret_buf.cpu().numpy(), vp_buf.cpu().numpy()
                got = ret[:T * R].reshape(T, R).astype(F64)
                err = float(np.abs(got - ref[:T]).max())
                print(f"{what}: err32 {err32:.2e} kernel err {err:.2e}")
                np.testing.assert_allclose(got, ref[:T], rtol=1e-5, atol=4 * err32, err_msg=what)
                assert same_bits(vpo[:T * R], vp[:T].reshape(-1)), what + ": value_preds[:T] changed"
                if use_gae:
                    assert same_bits(vpo[T * R:n], nv), what + ": value_preds[T] != next_value"
                    assert np.isnan(ret[T * R:n]).all(), what + ": returns[T] written in a GAE branch"
                else:
                    assert same_bits(ret[T * R:n], nv), what + ": returns[T] != next_value"
                    assert (vpo[T * R:n] == SENT).all(), what + ": value_preds[T] written in a discounted branch"
                assert np.isnan(ret[n:]).all() and np.isnan(vpo[n:]).all(), what + ": wrote past the arrays"


# ---- 2. statistics -------------------------------------------------------------------------------------------------------
def _adv_case(n, variant, seed):
    rng = np.random.default_rng(seed)
    state = vn_state("zero" if variant == "zero_state" else "dyadic")
    ret = (rng.standard_normal(n) * 3 + 1.5).astype(F32)            # mean advantage ~ 0.5: the sum does not cancel
    vp = rng.standard_normal(n).astype(F32)
    active = (rng.random(n) > 0.3).astype(F32)
    if n == 1:
        active[:] = 1                                               # (all rows inactive: test_gpu_train_glue.py)
    if variant == "constant":
        vp[:] = 0.5; ret[:] = 4.25                                  # adv = 4.25 - (0.5 * 2 + 1) = 2.25 in every row, exactly
    elif variant == "one_active":
        active[:] = 0; active[n // 3] = 1
        vp[n // 3], ret[n // 3] = 0.5, 3.0                          # the one active row is exact (adv = 1): the mean carries no rounding
    elif variant == "offset_returns":
        ret = (1e4 + rng.standard_normal(n)).astype(F32)
    return state, ret, vp, active


def _check_adv(ops, n, variant, seed):
    state, ret, vp, active = _adv_case(n, variant, seed)
    what = f"n={n} {variant}"
    buf = torch.full((n + GUARD,), NAN, device="cuda")
    adv = buf[:n]
    mom = torch.full((3,), NAN, dtype=torch.float64, device="cuda")
    ops.adv_moments(dev(ret), dev(vp), dev(active), dev(state), adv, mom)
    a_k = adv.cpu().numpy()
    m = mom.cpu().numpy()
    # float64 reference from the fp32 inputs and the fp32 (mean, sd) of vn_stats (exact for both states used here)
    mean32, sd32 = vn_mean_sd(state, F32)
    dn = vp.astype(F64) * F64(sd32) + F64(mean32)
    a_ref = ret.astype(F64) - dn
    # 2 ulp (fp32) of the larger operand of the subtraction: one rounding of vp * sd + mean (contracted to an FMA or not
    # observable here), one of the subtraction
    bound = 2 * np.spacing(np.maximum(np.abs(ret), np.abs(dn).astype(F32)).astype(F32)).astype(F64)
    err = np.abs(a_k.astype(F64) - a_ref)
    print(f"{what}: worst adv error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), f"{what}: advantage off by {float((err / bound).max()):.2f} x its 2-ulp bound"
    on = active != 0
    a64 = a_k.astype(F64)
    sums = np.array([a64[on].sum(), (a64[on] ** 2).sum(), float(on.sum())])
    np.testing.assert_allclose(m, sums, rtol=1e-12, atol=0, err_msg=what + ": moments")
    ops.adv_normalize(adv, mom)
    out = buf.cpu().numpy()
    assert np.isnan(out[n:]).all(), what + ": wrote past adv"
    mean, std = a_ref[on].mean(), a_ref[on].std()
    ref = (a_ref - mean) / (std + 1e-5)
    tol = bound / (std + 1e-5) + 1e-6 * np.abs(ref)
    nerr = np.abs(out[:n].astype(F64) - ref)
    print(f"{what}: std {std:.3e} worst normalised error / tolerance {float((nerr / np.maximum(tol, 1e-300)).max()):.3f}")
    assert (nerr <= tol).all(), f"{what}: normalised advantage off by {float((nerr / np.maximum(tol, 1e-300)).max()):.2f} x tolerance"
    return std


@gpu
@pytest.mark.parametrize("n", ADV_N)
def test_adv_moments_sizes(ops, n):
    """adv_moments + adv_normalize from one thread to the grid cap (n > 1024 * 1024: a fifth trip per thread), ~30 % rows inactive."""
    _check_adv(ops, n, "plain", n)


@gpu
@pytest.mark.parametrize("variant", ADV_VARIANTS)
def test_adv_moments_degenerate(ops, variant):
    """n = 4099: constant advantages (E[a^2] - mean^2 cancels to ~0, the divisor is the 1e-5 floor), one active row (the same, with
    4098 other rows scaled by 1e5), returns of 1e4 + N(0, 1) (the variance is 1e-8 of E[a^2]), the all-zero ValueNorm state."""
    std = _check_adv(ops, 4099, variant, 4099)
    if variant in ("constant", "one_active"):
        assert std == 0.0


@gpu
@pytest.mark.parametrize("B", MBM_B + ["duplicates"])
def test_minibatch_moments_gathered(ops, B):
    """minibatch_moments through a row list (a permutation prefix of a larger buffer; at the small size also a list with duplicates)
    against float64 sums at 1e-12."""
    rng = np.random.default_rng(9)
    if B == "duplicates":
        N, rows = 8, np.array([3, 3, 0, 3, 0], np.int32)
    else:
        N = B + 1000
        rows = rng.permutation(N)[:B].astype(np.int32)
    ret = (rng.standard_normal(N) * 3 + 0.5).astype(F32)
    act = (rng.random(N) > 0.3).astype(F32)
    mom = torch.full((4,), NAN, dtype=torch.float64, device="cuda")
    ops.minibatch_moments(dev(ret), dev(act), dev(rows, torch.int32), len(rows), mom)
    r64 = ret[rows].astype(F64)
    close(mom, [r64.sum(), (r64 ** 2).sum(), act[rows].astype(F64).sum(), len(rows)], 1e-12, 1e-9)


@gpu
@pytest.mark.parametrize("n", VN_UPDATE_N)
@pytest.mark.parametrize("start", ["zero", "running"])
def test_valuenorm_update_n(ops, n, start):
    """valuenorm_update_n == n valuenorm_update calls bit for bit, states_out[e] the state after call e + 1, and the final state
    equal to ValueNormRef updated n times with the same batch (2e-6, the single-update figure)."""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(3000) * 2 + 1).astype(F32)
    mom = torch.zeros(4, dtype=torch.float64, device="cuda")
    ops.minibatch_moments(dev(x), torch.ones(x.size, device="cuda"), None, x.size, mom)
    s0 = vn_state(start)
    st_n, st_1 = dev(s0), dev(s0)
    out = torch.full((n + 1, 3), NAN, device="cuda")
    ops.valuenorm_update_n(st_n, mom, 0.99999, n, out[:n])
    ref = O.ValueNormRef(); ref.load_state(s0)
    for e in range(n):
        ops.valuenorm_update(st_1, mom, 0.99999)
        assert torch.equal(out[e], st_1), f"states_out[{e}]"
        ref.update(x.reshape(-1, 1))
    assert torch.equal(st_n, st_1)
    assert all_nan(out[n]), "wrote past states_out"
    close(st_n, ref.state(), 2e-6, 1e-9)


# ---- 3. loss ---------------------------------------------------------------------------------------------------------------
def _loss_inputs(B, A, n_rows, seed, logit_scale=2.0, **flags):
    """Minibatch-order logits / values [B], buffer-order everything else [n_rows]; rows: a permutation prefix of the buffer."""
    rng = np.random.default_rng(seed)
    f = F32
    a = O.default_args(**flags)
    logits = (rng.standard_normal((B, A)) * logit_scale).astype(f)
    values = rng.standard_normal(B).astype(f)
    rows = rng.permutation(n_rows)[:B].astype(np.int32)
    avail = (rng.random((n_rows, A)) > 0.3).astype(f)
    actions = rng.integers(0, A, n_rows).astype(f)
    avail[np.arange(n_rows), actions.astype(int)] = 1.0
    old_logp = (-np.abs(rng.standard_normal(n_rows)) - 0.3).astype(f)
    adv = rng.standard_normal(n_rows).astype(f)
    active = (rng.random(n_rows) > 0.25).astype(f)
    v_old = (values.mean() + rng.standard_normal(n_rows) * 0.3).astype(f)
    ret = (rng.standard_normal(n_rows) * 4).astype(f)
    ret[rng.random(n_rows) > 0.9] *= 20                                    # Huber's linear branch
    vn = O.ValueNormRef(); vn.update(ret[:50].reshape(-1, 1))
    for _ in range(3):
        vn.update(ret.reshape(-1, 1))
    return dict(a=a, B=B, A=A, n_rows=n_rows, logits=logits, values=values, rows=rows, avail=avail, actions=actions, old_logp=old_logp,
                adv=adv, active=active, v_old=v_old, ret=ret, vn=vn.state(), dv_noise=rng.standard_normal(n_rows).astype(f) * 0.25)


def _loss_view(inp, with_rows):
    """(rows or None, per-sample arrays as the kernel and the reference see them).  v_old lies on both sides of the clip range around
    the values of the rows the minibatch reads."""
    B = inp["B"]
    rows = inp["rows"] if with_rows else np.arange(B, dtype=np.int32)
    v_old = inp["v_old"].copy()
    v_old[rows] = inp["values"] + inp["dv_noise"][:B]
    return rows, v_old


def _loss_ref(inp, with_rows, with_avail):
    a = inp["a"]
    rows, v_old = _loss_view(inp, with_rows)
    mean, sd = vn_mean_sd(inp["vn"], F64)
    return O.ppo_loss_fwd_bwd_ref(inp["logits"], inp["avail"][rows] if with_avail else None, inp["actions"][rows], inp["old_logp"][rows],
                                  inp["adv"][rows], inp["active"][rows], inp["values"], v_old[rows], inp["ret"][rows], float(mean),
                                  float(sd) ** 2, a.clip_param, a.entropy_coef, a.value_loss_coef, a.huber_delta, a.use_huber_loss,
                                  a.use_clipped_value_loss, a.use_policy_active_masks, a.use_value_active_masks, a.use_valuenorm)


def _offset_copy(x, off):
    """A contiguous device copy of x that starts `off` floats after a 16-byte boundary, NaN around it; (view, whole buffer)."""
    n = x.numel()
    buf = torch.full((n + 8,), NAN, device="cuda")
    v = buf[off:off + n]
    v.copy_(x.reshape(-1))
    v = v.view(x.shape)
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v, buf


def _loss_launch(ops, inp, with_rows, with_avail, offsets=()):
    """One ppo_loss_fwd_bwd launch; `offsets` names the tile pointers that start one float after a 16-byte boundary.  Returns the
    six statistics, d(logits), d(values) as NumPy arrays; checks that nothing is written around d(logits)."""
    a, B, A = inp["a"], inp["B"], inp["A"]
    rows, v_old = _loss_view(inp, with_rows)
    d_rows = dev(rows, torch.int32) if with_rows else None
    mom = torch.zeros(4, dtype=torch.float64, device="cuda")
    d_ret, d_act = dev(inp["ret"]), dev(inp["active"])
    ops.minibatch_moments(d_ret, d_act, d_rows, B, mom)
    logits, _ = _offset_copy(dev(inp["logits"]), 1 if "logits" in offsets else 0)
    avail = None
    if with_avail:
        avail, _ = _offset_copy(dev(inp["avail"]), 1 if "avail" in offsets else 0)
    off = 1 if "dlogits" in offsets else 0
    dl, dl_buf = _offset_copy(torch.zeros(B, A, device="cuda"), off)
    dv_buf = torch.full((B + GUARD,), NAN, device="cuda")
    stats = torch.zeros(6, dtype=torch.float64, device="cuda")
    ops.ppo_loss_fwd_bwd(logits, dev(inp["values"]), d_rows, avail, dev(inp["actions"]), dev(inp["old_logp"]), dev(inp["adv"]), d_act,
                         dev(v_old), d_ret, dev(inp["vn"]), mom, dl, dv_buf[:B], stats, ops.ppo_cfg(a))
    assert all_nan(dl_buf[:off]) and all_nan(dl_buf[off + B * A:]) and all_nan(dv_buf[B:]), "wrote around d(logits) / d(values)"
    return stats.cpu().numpy(), dl.cpu().numpy(), dv_buf[:B].cpu().numpy()


def _check_loss(ops, inp, with_rows, with_avail, offsets=()):
    """Launch and compare with ppo_loss_fwd_bwd_ref at the tolerances of test_gpu_kernels._loss_case; every row counts."""
    ref = _loss_ref(inp, with_rows, with_avail)
    s, dl, dv = _loss_launch(ops, inp, with_rows, with_avail, offsets)
    rows, _ = _loss_view(inp, with_rows)
    close(s[0], ref["value_loss"], 1e-5, 1e-7, "value_loss")
    close(s[1], ref["policy_loss"], 1e-5, 1e-7, "policy_loss")
    close(s[2], ref["dist_entropy"], 1e-5, 1e-7, "entropy")
    close(s[3], ref["ratio_mean"], 1e-5, 1e-7, "ratio")
    assert s[4] == inp["active"][rows].sum() and s[5] == inp["B"]
    close_rel_max(dl, ref["dlogits"], 2e-5, "dlogits")
    close_rel_max(dv, ref["dvalues"], 2e-5, "dvalues")
    return ref, s, dl, dv


@gpu
@pytest.mark.parametrize("with_rows,with_avail", LOSS_PAIRS)
@pytest.mark.parametrize("B,A", LOSS_SHAPES)
def test_ppo_loss_rows_and_avail_independent(ops, B, A, with_rows, with_avail):
    """All four (rows, avail) pairs.  (avail, no rows) stages the availability tile in LDS; at A = 32 that is the largest request the
    kernel can make, 64 KiB dynamic + 512 B static (accepted as it stands on the MI355X).  (rows, no avail) runs nowhere else."""
    inp = _loss_inputs(B, A, B + 123 if with_rows else B, B + A)
    _check_loss(ops, inp, with_rows, with_avail)


@gpu
@pytest.mark.parametrize("name", ["zero", "one_update"])
def test_loss_target_with_clamped_valuenorm_state(ops, name):
    """The iteration-0 states of ValueNorm reach the loss: its value target (ret - mean) / sd with the clamped statistics."""
    inp = _loss_inputs(600, 5, 600, 21)
    inp["vn"] = vn_state(name)
    _check_loss(ops, inp, False, True)


@gpu
def test_ppo_loss_misaligned_tiles(ops):
    """logits, avail and d(logits) each one float off a 16-byte boundary (alone, then together) take the scalar copy loops; the
    results are bit-identical to the aligned launch, which itself matches float64.  B = 513, A = 5: the last tile holds one row,
    so the aligned 16-byte copy has a scalar tail of one float."""
    inp = _loss_inputs(513, 5, 513, 31)
    _, s0, dl0, dv0 = _check_loss(ops, inp, False, True)
    for offsets in MISALIGNED:
        s, dl, dv = _loss_launch(ops, inp, False, True, offsets)
        assert np.array_equal(s, s0) and same_bits(dl, dl0) and same_bits(dv, dv0), f"misaligned {offsets}"


@gpu
def test_ppo_loss_grid_stride_second_trip(ops):
    """B = 2048 * 256 + 257: the grid is capped at 2048 workgroups, workgroups 0 and 1 take a second tile (the last one ragged)."""
    inp = _loss_inputs(LOSS_STRIDE_B, 5, LOSS_STRIDE_B, 41)
    _check_loss(ops, inp, False, True)


@gpu
@pytest.mark.parametrize("A", [5, 18])
def test_ppo_loss_saturated_softmax(ops, A):
    """Logits scaled by 30 (probabilities of 1 and of exp(-300)); every eighth row has the taken action as its only available one:
    its entropy and its gradient are exactly 0.  Old log-probs are the float64 reference's log-probs plus noise, so log-ratios stay
    inside +-20, no ratio overflows and every row is compared."""
    B = 1000
    inp = _loss_inputs(B, A, B, 51 + A, logit_scale=60.0)
    rng = np.random.default_rng(A)
    only = np.arange(B) % 8 == 0
    act = inp["actions"].astype(int)
    # half of the other rows take their most likely available action, as a saturated policy does
    z = np.where(inp["avail"] == 0, -1e10, inp["logits"].astype(F64))
    greedy = (rng.random(B) < 0.5) & ~only
    act[greedy] = z[greedy].argmax(-1)
    inp["actions"] = act.astype(F32)
    inp["avail"][only] = 0
    inp["avail"][np.arange(B), act] = 1
    z = np.where(inp["avail"] == 0, -1e10, inp["logits"].astype(F64))
    logp = (z - z.max(-1, keepdims=True) - np.log(np.exp(z - z.max(-1, keepdims=True)).sum(-1, keepdims=True)))[np.arange(B), act]
    inp["old_logp"] = (logp + np.clip(rng.standard_normal(B), -20, 20)).astype(F32)
    assert np.abs(logp - inp["old_logp"]).max() < 20 and logp.min() < -100
    ref, s, dl, dv = _check_loss(ops, inp, False, True)
    assert (dl[only] == 0).all(), "a row whose only available action is the taken one has no gradient"
    # entropy of those rows is exactly 0: with only them weighted, the statistic is 0
    inp2 = dict(inp); inp2["active"] = only.astype(F32)
    s2, dl2, _ = _loss_launch(ops, inp2, False, True)
    assert s2[2] == 0.0 and (dl2[only] == 0).all() and np.isfinite(s2).all()


@gpu
def test_ppo_loss_value_kinks_exact(ops):
    """Rows that sit exactly on the kinks of the value loss (|v - v_old| == clip, |error| == huber_delta), one step of 2^-6 inside
    and outside them, and rows where the clipped and unclipped losses tie: all operands are small dyadic rationals, so fp32 and
    float64 take the same branch everywhere.  Reference: float64 autograd through the loss expressions of r_mappo.py."""
    h = 2.0 ** -6
    clip, delta = 0.25, 8.0
    a = O.default_args(use_valuenorm=False, clip_param=clip, huber_delta=delta)
    dvs = [-clip, clip, clip - h, -(clip - h), clip + h, -(clip + h), 0.0, 0.5, -0.5]
    errs = [delta, -delta, delta - h, -(delta - h), delta + h, -(delta + h), 0.125, -3.0, 12.0]
    v_old, v, ret = [], [], []
    for i, d in enumerate(dvs):
        for j, e in enumerate(errs):
            vo = (i - 4) * 0.5 + j * h
            v_old.append(vo); v.append(vo + d); ret.append(vo + d + e)
    # clipped and unclipped losses tie outside the clip range: the target halfway between v and v_old +- clip
    for sgn in (1.0, -1.0):
        v_old.append(0.75); v.append(0.75 + sgn * 0.5); ret.append(0.75 + sgn * 0.375)
    B, A = len(v), 5
    inp = _loss_inputs(B, A, B, 61)
    inp.update(a=a, values=np.array(v, F32), ret=np.array(ret, F32), dv_noise=np.zeros(B, F32))
    inp["active"][:] = 1; inp["active"][3::7] = 0
    inp["dv_noise"] = (np.array(v_old, F32) - inp["values"])            # _loss_view: v_old[rows] = values + dv_noise
    for x in (inp["values"], inp["ret"], inp["dv_noise"]):
        assert (x.astype(F64) * 64 == np.round(x.astype(F64) * 64)).all()
    s, dl, dv = _loss_launch(ops, inp, False, False)
    t = lambda x: torch.from_numpy(np.asarray(x, F64)).view(-1, 1)
    vals = t(inp["values"]).requires_grad_(True)
    vo, tgt, act_t = t(v_old), t(inp["ret"]), t(inp["active"])
    vclip = vo + (vals - vo).clamp(-clip, clip)
    l = torch.max(O.huber_ref(tgt - vals, delta), O.huber_ref(tgt - vclip, delta))
    vl = (l * act_t).sum() / act_t.sum()
    (vl * a.value_loss_coef).backward()
    g = vals.grad.numpy().reshape(-1)
    close(s[0], vl.item(), 1e-6, 0, "value_loss")
    close_rel_max(dv, g, 1e-6, "dvalues on the kinks")
    # the tie rows got half of the unclipped slope, the rows exactly on the clip bound the full one
    on = inp["active"] != 0
    assert (np.abs(g[-2:]) > 0).all() and on[-2:].all()


# ---- 4. optimiser and slab reduction ---------------------------------------------------------------------------------------
B1, B2, EPS = float(F32(0.9)), float(F32(0.999)), float(F32(1e-5))       # the fp32 hyper-parameters as the kernel reads them
SEG_LR = [7e-4, 5e-4, 3e-4, 1e-3]
SEG_MAXNORM = [10.0, 0.5, 2.0, 0.05]


def _hyper(n_seg, wd=0.0):
    return np.array([[SEG_LR[s], 0.9, 0.999, 1e-5, wd, SEG_MAXNORM[s], 1.0, 1.0] for s in range(n_seg)], F32)


def _run_clip_adam(ops, sizes, variant):
    n_seg = len(sizes)
    bounds = [0] + list(np.cumsum(sizes))
    P = bounds[-1]
    rng = np.random.default_rng(100 + n_seg)
    hyper = _hyper(n_seg, 1e-2 if variant == "weight_decay" else 0.0)
    if variant == "no_clip_seg2":
        hyper[2, 6] = 0.0
    if variant == "seg1_disabled":
        hyper[1, 7] = 0.0
    step0 = 100000 if variant == "step_100000" else 0
    p0 = rng.standard_normal(P).astype(F32)
    m0 = (rng.standard_normal(P) * 0.01).astype(F32) if variant == "seg1_disabled" else np.zeros(P, F32)
    v0 = (rng.random(P) * 1e-3).astype(F32) if variant == "seg1_disabled" else np.zeros(P, F32)
    params, m, v = dev(p0), dev(m0), dev(v0)
    d_hyper = dev(hyper)
    step = torch.full((n_seg,), step0, dtype=torch.int32, device="cuda")
    norms = torch.full((n_seg + 4,), NAN, device="cuda")
    acc = torch.zeros(n_seg, dtype=torch.float64, device="cuda")
    ws = ops.optim_workspace(P, params.device)
    ref = [[p0[lo:hi].astype(F64), m0[lo:hi].astype(F64), v0[lo:hi].astype(F64)] for lo, hi in zip(bounds[:-1], bounds[1:])]
    acc_ref = np.zeros(n_seg)
    for it in range(5):
        scale = 0.5 if it % 2 else 0.01
        gr = (rng.standard_normal(P) * scale).astype(F32)
        if variant == "zero_grad":
            gr[:] = 0
        if variant == "huge_grad":
            for s, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
                gr[lo:hi] *= F32(1e4 * SEG_MAXNORM[s] / np.linalg.norm(gr[lo:hi].astype(F64)))
        ops.clip_adam(params, dev(gr), m, v, bounds, d_hyper, step, norms[:n_seg], ws, norm_acc=acc)
        pk, mk, vk, nk = params.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), norms.cpu().numpy()
        assert np.isnan(nk[n_seg:]).all(), "wrote past grad_norms"
        for s, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            what = f"{variant} sizes={sizes} seg {s} it {it}"
            h = hyper[s].astype(F64)
            norm = math.sqrt(float((gr[lo:hi].astype(F64) ** 2).sum()))
            acc_ref[s] += norm
            close(nk[s], norm, 1e-6, 1e-9, what + ": norm")
            if variant == "huge_grad":
                assert norm > 0.99e4 * SEG_MAXNORM[s]
            if h[7] == 0.0:                                    # disabled: untouched, bit for bit
                assert same_bits(pk[lo:hi], p0[lo:hi]) and same_bits(mk[lo:hi], m0[lo:hi]) and same_bits(vk[lo:hi], v0[lo:hi]), what
                continue
            ref[s] = list(O.clip_adam_ref(ref[s][0], gr[lo:hi], ref[s][1], ref[s][2], step0 + it, h[0], h[5], use_clip=bool(h[6]),
                                          beta1=B1, beta2=B2, eps=EPS, weight_decay=h[4])[:3])
            close(pk[lo:hi], ref[s][0], 1e-6, 1e-7, what + ": params")
            close(mk[lo:hi], ref[s][1], 1e-6, 1e-7, what + ": exp_avg")
            close(vk[lo:hi], ref[s][2], 1e-6, 1e-7, what + ": exp_avg_sq")
            if variant == "zero_grad":
                assert same_bits(pk[lo:hi], p0[lo:hi]) and nk[s] == 0.0 and not mk[lo:hi].any() and not vk[lo:hi].any(), what
        assert np.isfinite(pk).all() and np.isfinite(mk).all() and np.isfinite(vk).all()
    want = [step0 + (0 if hyper[s, 7] == 0.0 else 5) for s in range(n_seg)]
    assert step.cpu().tolist() == want
    close(acc, acc_ref, 1e-6, 1e-9, f"{variant}: norm_acc")
    if variant == "seg1_disabled":
        assert not same_bits(params.cpu().numpy()[:bounds[1]], p0[:bounds[1]]) and not same_bits(params.cpu().numpy()[bounds[2]:], p0[bounds[2]:])


@gpu
@pytest.mark.parametrize("n_seg", sorted(ADAM_LAYOUTS))
def test_clip_adam_layouts(ops, n_seg):
    """One to four segments (seg_of, workgroup 0's walk over the other segments), the three-segment layout with 258 norm partials in
    its middle segment: five steps with alternating gradient scales against clip_adam_ref in float64 — parameters, both moments,
    norms and norm_acc."""
    _run_clip_adam(ops, ADAM_LAYOUTS[n_seg], "plain")


@gpu
@pytest.mark.parametrize("variant", [v for v in ADAM_VARIANTS if v != "plain"])
def test_clip_adam_variants(ops, variant):
    """On [256, 33024, 512]: weight decay, clipping off on one segment, segment 1 disabled (untouched bit for bit while the others
    advance), an all-zero gradient (nothing moves, norm 0), a gradient norm of 1e4 x max_norm, step counters preset to 100 000."""
    _run_clip_adam(ops, ADAM_LAYOUTS[3], variant)


def _slabs(n_slabs, P, stride, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    slabs = torch.full((n_slabs, stride), NAN, device="cuda")
    slabs[:, :P] = torch.randn(n_slabs, P, device="cuda", generator=g) * 0.05
    return slabs


@gpu
@pytest.mark.parametrize("n_slabs", SLAB_N)
def test_slab_reduce_shapes(ops, n_slabs):
    """slab_reduce with empty quarters (n_slabs < 4), ragged and full 16-row batches, P around the 128-parameter workgroup and
    stride > P with NaN in the unused columns, against float64 column sums.  Bound per entry: n_slabs * 2^-24 * sum_s |slab[s, p]|,
    which holds for any order of an fp32 summation."""
    for P in SLAB_P:
        stride = P + 37
        slabs = _slabs(n_slabs, P, stride, n_slabs * 1000 + P)
        gbuf = torch.full((P + GUARD,), NAN, device="cuda")
        ops.slab_reduce(slabs, n_slabs, stride, P, gbuf[:P])
        got = gbuf.cpu().numpy()
        s64 = slabs[:, :P].cpu().numpy().astype(F64)
        bound = n_slabs * 2.0 ** -24 * np.abs(s64).sum(0)
        err = np.abs(got[:P].astype(F64) - s64.sum(0))
        assert (err <= bound).all(), f"n_slabs={n_slabs} P={P}: worst error / bound {float((err / bound).max()):.2f}"
        assert np.isnan(got[P:]).all(), f"n_slabs={n_slabs} P={P}: wrote past grad[P]"


@gpu
@pytest.mark.parametrize("n_slabs", RCA_N)
def test_reduce_clip_adam_three_segments(ops, n_slabs):
    """reduce_clip_adam on [256, 33024, 512] with an empty quarter (3 slabs) and ragged ones (67): the gradient bit-equal to
    slab_reduce, the rest equal to slab_reduce + clip_adam at the tolerances of
    test_reduce_clip_adam_matches_slab_reduce_then_clip_adam."""
    sizes = ADAM_LAYOUTS[3]
    bounds = [0] + list(np.cumsum(sizes))
    P = bounds[-1]
    stride = P + 37
    slabs = _slabs(n_slabs, P, stride, n_slabs)
    hyper = dev(_hyper(3))
    p0 = torch.randn(P, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    out = []
    for fused in (False, True):
        params = p0.clone(); m = torch.zeros(P, device="cuda"); v = torch.zeros(P, device="cuda")
        step = torch.zeros(3, dtype=torch.int32, device="cuda"); norms = torch.zeros(3, device="cuda")
        acc = torch.zeros(3, dtype=torch.float64, device="cuda")
        gbuf = torch.full((P + GUARD,), NAN, device="cuda")
        grad = gbuf[:P]
        ws = ops.optim_workspace(P, params.device)
        for it in range(3):
            if fused:
                ops.reduce_clip_adam(slabs, n_slabs, stride, params, grad, m, v, bounds, hyper, step, norms, ws, norm_acc=acc)
            else:
                ops.slab_reduce(slabs, n_slabs, stride, P, grad)
                ops.clip_adam(params, grad, m, v, bounds, hyper, step, norms, ws, norm_acc=acc)
        assert all_nan(gbuf[P:])
        out.append([t.cpu().numpy() for t in (grad, params, m, v, norms, acc, step)])
    assert np.isfinite(out[1][0]).all()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][6], out[1][6])
    for a_, b_ in zip(out[0][1:6], out[1][1:6]):
        np.testing.assert_allclose(a_, b_, rtol=2e-6, atol=1e-7)
