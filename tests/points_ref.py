"""The numpy restatement of interp_points and its gradients (include/lagomorph_hip.h: lago_interp_points,
lago_interp_points_backward), and the cases the point-set tests share.

Per axis a with extent n, in the precision R of the positions:

    f = floor(x), t = x - f                      (then float64)
    lo = clip(f, 0, n - 1), hi = clip(f + 1, 0, n - 1)

`sample` evaluates the multilinear interpolant and its position gradient on those corners in float64 (the exact
function of the rounded t, not the library's rounding sequence: the GPU tests compare to a tolerance, the bit-for-bit
statement is the one against `interp`).  `scatter_wide` is the adjoint the way tests/scatter_bound.py judges scatter-adds:
every contribution is (the weight (a_x a_y) a_z formed in R) x (g in R) taken in a wider type and summed there.
"""
import itertools

import numpy as np

SHAPES = ((5, 6, 7), (7, 9), (8, 16, 32), (1, 5, 4), (6, 1, 3), (1, 9), (2, 2, 2))
POINT_COUNTS = (1, 63, 64, 65, 257, 1000)


def _taps(x, sp):
    """Per axis (lo, hi, t): int64 corner indices (N, P) and the fraction in x's dtype."""
    out = []
    for a, n in enumerate(sp):
        xa = x[:, a]
        with np.errstate(invalid="ignore"):
            f = np.floor(xa)
            t = xa - f                                   # in R
            fi = np.where(np.isfinite(f), np.clip(f, -2.0 ** 30, 2.0 ** 30), 0.0).astype(np.int64)
        out.append((np.clip(fi, 0, n - 1), np.clip(fi + 1, 0, n - 1), t))
    return out


def sample(F, x):
    """F (N or 1, C, *sp), x (N, d, P) float32 / float64 -> (values (N, C, P), gradients (N, C, d, P)), float64:
    grad[n, c, a, p] = dF_c/dx_a at x[n, :, p], the one-sided derivative of the cell floor(x)."""
    F = np.asarray(F)
    sp, d = F.shape[2:], F.ndim - 2
    N, P = x.shape[0], x.shape[2]
    assert x.shape[1] == d and F.shape[0] in (1, N)
    tp = _taps(x, sp)
    F64 = np.broadcast_to(F.astype(np.float64), (N,) + F.shape[1:])
    item = np.arange(N).reshape(N, 1, 1)
    chan = np.arange(F.shape[1]).reshape(1, -1, 1)
    val = np.zeros((N, F.shape[1], P))
    grad = np.zeros((N, F.shape[1], d, P))
    t64 = [tp[a][2].astype(np.float64)[:, None, :] for a in range(d)]

    def corner(bits):                                                            # (N, C, P)
        return F64[(item, chan) + tuple((tp[a][1] if b else tp[a][0])[:, None, :] for a, b in enumerate(bits))]

    def weight(bits, skip=None):
        return np.prod([t64[a] if b else 1.0 - t64[a] for a, b in enumerate(bits) if a != skip], axis=0)

    with np.errstate(invalid="ignore"):
        for bits in itertools.product((0, 1), repeat=d):
            val += weight(bits) * corner(bits)
            # the derivative along axis a: the difference of the two corners of that axis (exactly 0 where they
            # coincide), weighted over the other axes
            for a in range(d):
                if bits[a] == 0:
                    up = bits[:a] + (1,) + bits[a + 1:]
                    grad[:, :, a] += weight(bits, skip=a) * (corner(up) - corner(bits))
    return val, grad


def scatter_wide(g, x, sp, nF):
    """(sum, sabs, count), each (nF, C, *sp): per cell of d_F the wide sum of the contributions w_q g of every point's
    2^d clamped corners (coinciding corners each add), the sum of their magnitudes and their number.  w_q = (a_x a_y) a_z
    in the working precision (a_y a_z in 2D), a = 1 - t below and t above; the product with g and the sums in float64
    for float32 inputs and in np.longdouble for float64, the convention of tests/scatter_bound.py.  nF = 1: every item
    adds into one volume (a broadcast F)."""
    g = np.asarray(g)
    R = g.dtype.type
    assert x.dtype == g.dtype and R in (np.float32, np.float64)
    wide = np.float64 if R is np.float32 else np.longdouble
    N, C, P = g.shape
    d = len(sp)
    assert nF in (1, N) and x.shape == (N, d, P)
    tp = _taps(x, sp)
    nvox = int(np.prod(sp))
    s = np.zeros((nF, C, nvox), dtype=wide)
    sabs = np.zeros((nF, C, nvox), dtype=wide)
    count = np.zeros((nF, C, nvox), dtype=np.float64)
    item = np.broadcast_to((np.arange(N) if nF == N else np.zeros(N, dtype=np.int64)).reshape(N, 1, 1), (N, C, P))
    chan = np.broadcast_to(np.arange(C).reshape(1, C, 1), (N, C, P))
    for bits in itertools.product((0, 1), repeat=d):
        fac = [tp[a][2] if b else R(1) - tp[a][2] for a, b in enumerate(bits)]            # in R
        w = (fac[0] * fac[1]) * fac[2] if d == 3 else fac[0] * fac[1]                     # in R, rounded as written
        assert w.dtype == g.dtype
        lin = np.zeros((N, P), dtype=np.int64)
        for a, b in enumerate(bits):
            lin = lin * sp[a] + (tp[a][1] if b else tp[a][0])
        lin = np.broadcast_to(lin[:, None, :], (N, C, P))
        t = w[:, None, :].astype(wide) * g.astype(wide)
        np.add.at(s, (item, chan, lin), t)
        np.add.at(sabs, (item, chan, lin), np.abs(t))
        np.add.at(count, (item, chan, lin), 1.0)
    shape = (nF, C) + tuple(sp)
    return s.reshape(shape), sabs.reshape(shape).astype(np.float64), count.reshape(shape)


# ---- cases (all seeded)

def _rng(tag, *key):
    return np.random.default_rng([tag, *[int(k) for k in key]])


def field(NF, C, sp, dtype, seed=0):
    """(NF, C, *sp) of standard normal values."""
    return _rng(1, seed, NF, C, *sp).standard_normal((NF, C) + tuple(sp)).astype(dtype)


def upstream(N, C, P, dtype, seed=0):
    """(N, C, P): the upstream gradient of a backward."""
    return _rng(2, seed, N, C, P).standard_normal((N, C, P)).astype(dtype)


def scattered(N, sp, P, dtype, seed=0):
    """(x (N, d, P), first): the points [first:] are uniform in [-2.5, n + 1.5] per axis, the points [:first] uniform
    inside [0, n - 1]; first = P // 2 (a single point is of the wide kind)."""
    rng = _rng(3, seed, N, P, *sp)
    d, first = len(sp), P // 2
    x = np.empty((N, d, P))
    for a, n in enumerate(sp):
        x[:, a, :first] = rng.uniform(0.0, n - 1.0, (N, first))
        x[:, a, first:] = rng.uniform(-2.5, n + 1.5, (N, P - first))
    return x.astype(dtype), first


def outside(x, sp):
    """Boolean (N, P): the point has a coordinate outside [0, n - 1]."""
    return np.any([(x[:, a] < 0) | (x[:, a] > n - 1) for a, n in enumerate(sp)], axis=0)


def crowd(N, sp, P, dtype, seed=0):
    """(N, d, P): every point of an item inside ONE cell (the same for all items: with a broadcast F both items add into
    the same 2^d cells); along an axis of extent 1 the cell is the voxel itself."""
    rng = _rng(4, seed, N, P, *sp)
    x = np.empty((N, len(sp), P))
    for a, n in enumerate(sp):
        x[:, a] = max((n - 2) // 2, 0) + rng.uniform(0.0, 1.0, (N, P))
    return x.astype(dtype)


def interior(N, sp, P, dtype, seed=0):
    """(N, d, P) inside the grid with fractional parts in [0.1, 0.9]: a finite difference of less than 0.1 crosses no
    cell face (the interpolant is piecewise multilinear)."""
    rng = _rng(5, seed, N, P, *sp)
    x = np.empty((N, len(sp), P))
    for a, n in enumerate(sp):
        assert n >= 2
        x[:, a] = rng.integers(0, n - 1, (N, P)) + rng.uniform(0.1, 0.9, (N, P))
    return x.astype(dtype)


def identity_points(N, sp, dtype):
    """The voxel positions of the grid as a point set (N, d, nvox), in grid order."""
    idx = np.indices(sp).astype(dtype).reshape(len(sp), -1)
    return np.ascontiguousarray(np.broadcast_to(idx, (N,) + idx.shape))
