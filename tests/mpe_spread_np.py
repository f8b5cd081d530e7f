"""Host restatement of the simple_spread reset draws (mpe_reset_env / mpe_uniform in csrc/mpe_core.h) on the host Philox of
rollout_ref.py, plus the loader of tests/golden/mpe_spread_shapes.npz.  A plain helper: no fixtures, no pytest settings.

Layout: environment n owns the 2 (MAX_M + MAX_L) = 32 uniform numbers 32 n .. 32 n + 31 of Philox stream (seed, episode), whatever
M and L are: 32 n + 2 i, + 1 are agent i's x, y; 32 n + 16 + 2 l, + 1 landmark l's (scaled by 0.8).  Uniform number u takes the two
32-bit words at Philox indices 2 u (high) and 2 u + 1 (low)."""
import numpy as np

MAX_M, MAX_L = 8, 8
DRAWS = 2 * (MAX_M + MAX_L)                      # uniform numbers per environment


def uniform_indices(N, M, L):
    """(agents [N, M, 2], landmarks [N, L, 2]) uint64: which uniform number of the stream each coordinate is."""
    base = (np.arange(N, dtype=np.uint64) * np.uint64(DRAWS))[:, None, None]
    xy = np.arange(2, dtype=np.uint64)[None, None, :]
    a = base + (np.uint64(2) * np.arange(M, dtype=np.uint64))[None, :, None] + xy
    l = base + np.uint64(2 * MAX_M) + (np.uint64(2) * np.arange(L, dtype=np.uint64))[None, :, None] + xy
    return a, l


def philox_indices(u):
    """The two Philox word indices (high, low) that uniform number(s) u read."""
    u = np.asarray(u, dtype=np.uint64)
    return np.uint64(2) * u, np.uint64(2) * u + np.uint64(1)


def uniform(seed, episode, u):
    """mpe_uniform: U(-1, 1) in float64 from two Philox words, the operations in the kernel's order."""
    import rollout_ref as R
    ih, il = philox_indices(u)
    hi = R.philox_u32(seed, episode, ih).astype(np.float64)
    lo = R.philox_u32(seed, episode, il).astype(np.float64)
    v = (hi * 4294967296.0 + lo + 0.5) * (1.0 / 18446744073709551616.0)
    return 2.0 * v - 1.0


def reset_draws(seed, episode, N, M, L):
    """The kernels' reset of environments 0 .. N - 1 at Philox stream (seed, episode), both taken as full 64-bit numbers:
    (pos [N, M, 2], lpos [N, L, 2]) float64."""
    a, l = uniform_indices(N, M, L)
    return uniform(seed, episode, a), 0.8 * uniform(seed, episode, l)


def shapes(g):
    """[(M, L)] of the groups `{M}x{L}/` in the fixture, in the file's order."""
    out = []
    for k in g.files:
        s = tuple(int(x) for x in k.split("/")[0].split("x"))
        if s not in out:
            out.append(s)
    return out
