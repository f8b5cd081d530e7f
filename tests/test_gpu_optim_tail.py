"""The optimiser tail of a PPO epoch (mappo_slab_reduce, mappo_reduce_clip_adam, mappo_clip_adam and the grouped form) against a
host mirror, bit for bit.

The mirror restates csrc/optim.hip in NumPy with the kernel's number formats and its order of operations:
  * slab reduce — float32; quarter q of the rows [q n / 4, (q + 1) n / 4): whole batches of 16 rows into acc[j & 3], the rest
    into acc[0], (acc0 + acc1) + (acc2 + acc3), the quarters as (q0 + q1) + (q2 + q3);
  * squared-norm partials — float64 g * g per 128 entries, summed as the wave's shuffle tree (lane i += lane i + off for
    off = 32 .. 1), then wave 0 + wave 1; a segment's norm the same way over its partials (256 threads: four waves);
  * clip and Adam — float32, as written in norm_adam_body, with the two products of the bias correction in float64
    (math.pow, the host's correctly rounded pow).  The compiler fuses the last step, p - (lr / bc1) * (m / denom), into one
    fma (every other product feeds a packed multiply and is rounded on its own); the mirror does that one with a single rounding too.
Values are compared as bit patterns, so a changed order of the float32 adds (values of mixed sign over 1e-8 .. 1e3) shows.
When the loads are issued and where the step scalars are computed is the kernel's business: none of it may show here."""
import math

import numpy as np
import pytest
import torch

F32, F64 = np.float32, np.float64
SLAB_BLOCK, SLAB_Q, SLAB_BATCH, OPT_BLOCK = 128, 4, 16, 256
# an empty quarter, the tail only, exact batches, batches plus tail, 64 rows plus tail per quarter (the most one thread holds in
# registers is 4 batches and a tail of up to 15), and 5 batches plus tail per quarter: a second round of the register block
N_SLABS = [1, 3, 4, 5, 63, 64, 65, 67, 134, 256, 269, 330]
LAYOUTS = {"256+256": [0, 256, 512], "768+256": [0, 768, 1024]}


@pytest.fixture(scope="module")
def ops(gpu_device):
    from mappo_amd import ops as _ops
    return _ops


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize])


def same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} elements differ"


# ---- the mirror ------------------------------------------------------------------------------------------------------------
def slab_sum_mirror(slabs):
    """slabs [n, P] float32 -> grad [P] float32"""
    n, P = slabs.shape
    quarters = []
    for q in range(SLAB_Q):
        s, hi = q * n // SLAB_Q, (q + 1) * n // SLAB_Q
        acc = np.zeros((4, P), F32)
        while s + SLAB_BATCH <= hi:
            for j in range(SLAB_BATCH):
                acc[j & 3] = acc[j & 3] + slabs[s + j]
            s += SLAB_BATCH
        while s < hi:
            acc[0] = acc[0] + slabs[s]
            s += 1
        quarters.append((acc[0] + acc[1]) + (acc[2] + acc[3]))
    return (quarters[0] + quarters[1]) + (quarters[2] + quarters[3])


def wave_tree(x):
    """[..., 64] float64 -> what lane 0 holds after wave_sum"""
    for off in (32, 16, 8, 4, 2, 1):
        x = x[..., :off] + x[..., off:2 * off]
    return x[..., 0]


def block_sum_mirror(x):
    """[..., 64 k] float64 (one value per thread) -> block_sum's result in thread 0"""
    w = wave_tree(x.reshape(x.shape[:-1] + (-1, 64)))
    s = np.zeros(w.shape[:-1], F64)
    for k in range(w.shape[-1]):
        s = s + w[..., k]
    return s


def sq_partials_mirror(grad):
    g = grad.astype(F64).reshape(-1, SLAB_BLOCK)
    return block_sum_mirror(g * g)


def seg_norm_mirror(partials, lo, hi):
    per_thread = np.zeros(OPT_BLOCK, F64)
    for k, b in enumerate(range(lo // SLAB_BLOCK, hi // SLAB_BLOCK)):
        per_thread[k % OPT_BLOCK] += partials[b]
    return F32(np.sqrt(block_sum_mirror(per_thread)))


def fma32(a, b, c):
    """float32 a * b + c with one rounding: the exact product and the sum's exact error in float64, the sum rounded to odd there."""
    p, c = a.astype(F64) * b.astype(F64), c.astype(F64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    odd = (s.view(np.int64) & 1) != 0
    s = np.where((e != 0) & ~odd, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


class Mirror:
    """params / m / v / step / norms / acc of one flat buffer on the host; hyper [n_seg, 8] =
    lr, beta1, beta2, eps, weight_decay, max_norm, use_clip, enabled."""

    def __init__(self, bounds, hyper, params, step, acc):
        self.bounds, self.hyper = bounds, hyper.astype(F32)
        self.params, self.m, self.v = params.astype(F32).copy(), np.zeros_like(params, F32), np.zeros_like(params, F32)
        self.step, self.acc = np.array(step, np.int32), np.array(acc, F64)
        self.norms = np.zeros(len(bounds) - 1, F32)
        self.grad = self.partials = None

    def update(self, grad):
        self.grad, self.partials = grad, sq_partials_mirror(grad)
        for s, (lo, hi) in enumerate(zip(self.bounds[:-1], self.bounds[1:])):
            lr, b1, b2, eps, wd, max_norm, use_clip, enabled = self.hyper[s]
            norm = seg_norm_mirror(self.partials, lo, hi)
            self.norms[s] = norm
            self.acc[s] += F64(norm)
            if enabled == 0:
                continue
            self.step[s] += 1
            t = float(self.step[s])
            bc1, bc2 = 1.0 - math.pow(float(b1), t), 1.0 - math.pow(float(b2), t)
            lr_bc1 = F32(F64(lr) / F64(bc1 if bc1 > 0.0 else 1.0))
            sqrt_bc2 = F32(math.sqrt(bc2 if bc2 > 0.0 else 1.0))
            coef = min(max_norm / (norm + F32(1e-6)), F32(1)) if use_clip != 0 else F32(1)
            g, pp, mi, vi = grad[lo:hi] * coef, self.params[lo:hi], self.m[lo:hi], self.v[lo:hi]
            if wd != 0:
                g = g + wd * pp
            mi = mi + (g - mi) * (F32(1) - b1)
            vi = vi * b2 + g * g * (F32(1) - b2)
            denom = np.sqrt(vi) / sqrt_bc2 + eps
            self.params[lo:hi], self.m[lo:hi], self.v[lo:hi] = fma32(np.full_like(pp, -lr_bc1), mi / denom, pp), mi, vi


def random_slabs(rng, n, P, stride):
    """[n, stride] float32: mixed signs, magnitudes log-uniform over 1e-8 .. 1e3; the columns past P are never read (NaN)."""
    x = (10.0 ** rng.uniform(-8, 3, (n, stride)) * rng.choice([-1.0, 1.0], (n, stride))).astype(F32)
    x[:, P:] = np.nan
    return x


def test_mirror_fma_rounds_once():
    """a b + c = 1 + 2^-23 + 2^-24 - 2^-70 lies below a float32 tie; its float64 sum lies ON the tie and would round to even."""
    a, b, c = F32(1 + 2.0 ** -23), F32((1 - 2.0 ** -23) * 2.0 ** -24), F32(1 + 2.0 ** -23)
    assert F32(F64(a) * F64(b) + F64(c)) == F32(1 + 2.0 ** -22)                       # rounded twice
    assert fma32(np.array([a]), np.array([b]), np.array([c]))[0] == F32(1 + 2.0 ** -23)
    assert fma32(np.array([-a]), np.array([b]), np.array([-c]))[0] == -F32(1 + 2.0 ** -23)
    assert fma32(np.array([F32(3)]), np.array([F32(0.5)]), np.array([F32(0.25)]))[0] == F32(1.75)


# ---- slab reduce -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n_slabs", N_SLABS)
def test_slab_reduce_bits(ops, n_slabs, layout):
    """The gradient of mappo_slab_reduce and of mappo_reduce_clip_adam, and the latter's squared-norm partials (the head of its
    workspace: one float64 per 128 entries), equal the mirror's bit for bit."""
    bounds = LAYOUTS[layout]
    P, stride = bounds[-1], bounds[-1] + 128
    rng = np.random.default_rng(n_slabs * 7 + P)
    slabs = random_slabs(rng, n_slabs, P, stride)
    want = slab_sum_mirror(slabs[:, :P])
    d_slabs = dev(slabs)
    grad = torch.full((P,), float("nan"), device="cuda")
    ops.slab_reduce(d_slabs, n_slabs, stride, P, grad)
    same(grad, want, "slab_reduce")
    hyper = np.tile(np.array([7e-4, 0.9, 0.999, 1e-5, 0.0, 10.0, 1.0, 1.0], F32), (2, 1))
    grad2, ws = torch.full((P,), float("nan"), device="cuda"), ops.optim_workspace(P, "cuda")
    ws.fill_(255)
    st = [dev(rng.standard_normal(P)), torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")]
    ops.reduce_clip_adam(d_slabs, n_slabs, stride, st[0], grad2, st[1], st[2], bounds, dev(hyper), torch.zeros(2, dtype=torch.int32, device="cuda"),
                         torch.zeros(2, device="cuda"), ws)
    same(grad2, want, "reduce_clip_adam: gradient")
    same(ws[:P // SLAB_BLOCK * 8].view(torch.float64), sq_partials_mirror(want), "reduce_clip_adam: squared-norm partials")


# ---- clip + Adam -----------------------------------------------------------------------------------------------------------
# three segments: clipping active (a tiny max_norm) | disabled | no clipping; and two enabled ones whose clip stays at 1
def _hyper(wd):
    three = np.array([[7e-4, 0.9, 0.999, 1e-5, wd, 1e-3, 1.0, 1.0],
                      [5e-4, 0.9, 0.999, 1e-5, wd, 10.0, 1.0, 0.0],
                      [1e-3, 0.8, 0.99, 1e-8, 0.0, 10.0, 0.0, 1.0]], F32)
    two = np.array([[7e-4, 0.9, 0.999, 1e-5, wd, 1e9, 1.0, 1.0],
                    [7e-4, 0.9, 0.999, 1e-5, 0.0, 0.5, 1.0, 1.0]], F32)
    return {"three": ([0, 256, 1024, 1280], three), "two": ([0, 768, 1024], two)}


class Device:
    """The device state of one flat buffer and the three entries that advance it."""

    def __init__(self, ops, bounds, hyper, params, n_slabs, stride):
        n_seg, P = len(bounds) - 1, bounds[-1]
        self.ops, self.bounds, self.P, self.n_slabs, self.stride = ops, bounds, P, n_slabs, stride
        self.hyper, self.params = dev(hyper), dev(params)
        self.m, self.v, self.grad = torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda"), torch.full((P,), float("nan"), device="cuda")
        self.step = torch.zeros(n_seg, dtype=torch.int32, device="cuda")
        self.norms = torch.full((n_seg,), float("nan"), device="cuda")
        self.acc = torch.full((n_seg,), 0.25, dtype=torch.float64, device="cuda")
        self.ws = ops.optim_workspace(P, "cuda")
        self.slabs = torch.zeros(n_slabs, stride, device="cuda")

    def reduce_clip_adam(self):
        self.ops.reduce_clip_adam(self.slabs, self.n_slabs, self.stride, self.params, self.grad, self.m, self.v, self.bounds, self.hyper, self.step,
                                  self.norms, self.ws, norm_acc=self.acc)

    def job(self):
        return self.ops.optim_job(self.slabs, self.n_slabs, self.stride, self.params, self.grad, self.m, self.v, self.bounds, self.hyper, self.step,
                                  self.norms, self.ws, norm_acc=self.acc)

    def reduce_then_clip_adam(self):
        self.ops.slab_reduce(self.slabs, self.n_slabs, self.stride, self.P, self.grad)
        self.ops.clip_adam(self.params, self.grad, self.m, self.v, self.bounds, self.hyper, self.step, self.norms, self.ws, norm_acc=self.acc)

    def check(self, mir, what):
        torch.cuda.synchronize()
        for name in ("grad", "params", "m", "v", "norms", "acc", "step"):
            same(getattr(self, name), getattr(mir, name), f"{what}: {name}")


def _case(ops, which, wd, n_slabs=67, seed=0):
    bounds, hyper = _hyper(wd)[which]
    P = bounds[-1]
    rng = np.random.default_rng(1000 * seed + P + n_slabs)
    params = rng.standard_normal(P).astype(F32)
    steps = [random_slabs(rng, n_slabs, P, P) * F32(scale) for scale in (1.0, 1e-3, 30.0)]
    return Device(ops, bounds, hyper, params, n_slabs, P), Mirror(bounds, hyper, params, [0] * (len(bounds) - 1), [0.25] * (len(bounds) - 1)), steps


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["reduce_clip_adam", "reduce_then_clip_adam"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("which", ["three", "two"])
def test_norm_adam_bits(ops, which, wd, entry):
    """Three successive steps from t = 0 through mappo_reduce_clip_adam, and through mappo_slab_reduce + mappo_clip_adam: gradient,
    parameters, both moments, norms, the norm accumulator and the step counters equal the mirror's after every step.  The disabled
    segment keeps parameters, moments and step while its norm is still published; the clipped one is scaled by max_norm / norm."""
    d, mir, steps = _case(ops, which, wd)
    for k, slabs in enumerate(steps):
        d.slabs.copy_(dev(slabs))
        getattr(d, entry)()
        mir.update(slab_sum_mirror(slabs))
        d.check(mir, f"step {k + 1}")
    if which == "three":
        assert mir.step.tolist() == [3, 0, 3] and not mir.m[256:1024].any() and mir.norms[0] > 1.0 and mir.m[:256].any()


@pytest.mark.gpu
def test_graph_replay_equals_eager(ops):
    """The two launches captured once and replayed three times give the bits of three eager calls (and so the mirror's)."""
    eager, mir, steps = _case(ops, "three", 0.01, seed=1)
    graphed, _, _ = _case(ops, "three", 0.01, seed=1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.reduce_clip_adam()
    for k, slabs in enumerate(steps):
        eager.slabs.copy_(dev(slabs)); graphed.slabs.copy_(dev(slabs))
        eager.reduce_clip_adam()
        g.replay()
        mir.update(slab_sum_mirror(slabs))
        eager.check(mir, f"eager step {k + 1}")
        graphed.check(mir, f"replay {k + 1}")


# ---- grouped form ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_group_equals_single_calls(ops):
    """Three jobs of different P, segment count and n_slabs, two successive steps: the grouped call leaves what the single calls
    leave (and the mirror holds), in either job order."""
    shapes = [("two", 0.0, 5), ("three", 0.01, 134), ("two", 0.01, 67)]
    for order in ([0, 1, 2], [2, 0, 1]):
        cases = [_case(ops, *shapes[k], seed=k) for k in range(3)]
        singles = [_case(ops, *shapes[k], seed=k)[0] for k in range(3)]
        for step in range(2):
            for d, (g, mir, steps) in zip(singles, cases):
                d.slabs.copy_(dev(steps[step])); g.slabs.copy_(dev(steps[step]))
                d.reduce_clip_adam()
                mir.update(slab_sum_mirror(steps[step]))
            ops.reduce_clip_adam_group([cases[k][0].job() for k in order])
            for k in range(3):
                singles[k].check(cases[k][1], f"single job {k}, step {step + 1}")
                cases[k][0].check(cases[k][1], f"order {order}: job {k}, step {step + 1}")
