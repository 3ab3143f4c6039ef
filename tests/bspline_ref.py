"""The numpy reference for bspline_prefilter, interp_bspline and interp_cubic (include/lagomorph_hip.h), in float64, and
the float32 restatement of the weight expressions of lagomorph_amd/csrc/bspline_weights.hpp.

Prefilter, per spatial axis of extent n > 1, axes in order: c solves B c = f, B the (1, 4, 1) / 6 tridiagonal with a
whole-sample mirror border (period 2n - 2), by the recursion (pole z = sqrt(3) - 2, gain 6, the FULL start sum).  The
adjoint solves B^T c = f with a dense solve: it shares nothing with the D B D^-1 trick the kernel uses.

Sampling, per axis: the position p = i + dt u in u's precision (labels_ref.sample_pos: the library's expression),
clamped to [0, n - 1]; f = min(floor(p), n - 2) (0 for n = 1), t = p - f; taps f - 1 ... f + 2 folded once (k -> |k|,
then k -> 2 (n - 1) - k beyond n - 1; n = 1: index 0); weights ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6
in float64 from the SAME t the library forms.  The derivative with respect to u is dt times the derivative weights'
sum, 0 along an axis whose position was clamped, NaN in every component where a coordinate is NaN.
"""
import itertools

import numpy as np

from labels_ref import sample_pos

Z = np.sqrt(3.0) - 2.0


# ---- prefilter

def matrix(n):
    """B (n, n): row i holds (1, 4, 1) / 6 at the mirrored columns i - 1, i, i + 1."""
    B = np.zeros((n, n))
    if n == 1:
        B[0, 0] = 1.0
        return B
    for i in range(n):
        for k, w in ((i - 1, 1.0), (i, 4.0), (i + 1, 1.0)):
            k = abs(k)
            k = 2 * (n - 1) - k if k > n - 1 else k
            B[i, k] += w / 6.0
    return B


def prefilter_axis(f, axis):
    """The recursion along one axis of a float64 array (any leading / trailing shape)."""
    n = f.shape[axis]
    if n == 1:
        return f.copy()
    f = np.moveaxis(f, axis, 0)
    per = 2 * n - 2
    idx = [k if k <= n - 1 else per - k for k in range(per)]
    cp = np.empty_like(f)
    cp[0] = 6.0 * sum(Z ** k * f[m] for k, m in enumerate(idx)) / (1.0 - Z ** per)
    for i in range(1, n):
        cp[i] = 6.0 * f[i] + Z * cp[i - 1]
    c = np.empty_like(f)
    c[n - 1] = Z / (Z * Z - 1.0) * (cp[n - 1] + Z * cp[n - 2])
    for i in range(n - 2, -1, -1):
        c[i] = Z * (c[i + 1] - cp[i])
    return np.moveaxis(c, 0, axis)


def prefilter(I, adjoint=False):
    """I (N, C, *sp) -> float64 coefficients; adjoint: B^-T along every axis (dense solve)."""
    out = np.asarray(I, dtype=np.float64)
    for a in range(2, out.ndim):
        if adjoint:
            n = out.shape[a]
            m = np.moveaxis(out, a, 0)
            out = np.moveaxis(np.linalg.solve(matrix(n).T, m.reshape(n, -1)).reshape(m.shape), 0, a)
        else:
            out = prefilter_axis(out, a)
    return np.ascontiguousarray(out)


# ---- sampling

def fold(k, n):
    if n == 1:
        return np.zeros_like(k)
    k = np.abs(k)
    return np.where(k > n - 1, 2 * (n - 1) - k, k)


def weights(t, work=np.float64):
    """(4, ...) in `work` (float64, or long double as the yardstick of float64 results) from t (any float dtype)."""
    t = np.asarray(t, dtype=work)
    s = 1.0 - t
    return np.stack([s ** 3, 3 * t ** 3 - 6 * t ** 2 + 4, -3 * t ** 3 + 3 * t ** 2 + 3 * t + 1, t ** 3]) / 6.0


def dweights(t, work=np.float64):
    t = np.asarray(t, dtype=work)
    s = 1.0 - t
    return np.stack([-s ** 2, 3 * t ** 2 - 4 * t, -3 * t ** 2 + 2 * t + 1, t ** 2]) / 2.0


def axis(p, n):
    """(k (4, ...) int64, f int64, t in p's dtype, clamped, nan) of positions p along an axis of extent n."""
    R = p.dtype.type
    nan = np.isnan(p)
    with np.errstate(invalid="ignore"):
        clamped = (p < R(0)) | (p > R(n - 1))
        x = np.where(p < R(0), R(0), p)
        x = np.where(x > R(n - 1), R(n - 1), x)
        f = np.where(nan, 0.0, np.floor(x)).astype(np.int64)
        f = np.minimum(f, max(n - 2, 0))
        t = (x - f.astype(p.dtype)).astype(p.dtype)
    k = np.stack([fold(f - 1 + q, n) for q in range(4)])
    return k, f, t, clamped, nan


def weights_f32(t):
    """bspline_weights.hpp's own expressions, operation by operation in t's precision (numpy rounds every one)."""
    R = t.dtype.type
    s = R(1) - t
    sixth = R(1.0 / 6.0)

    def poly(r):
        return ((R(3) - R(3) * r) * r + R(3)) * r + R(1)

    return np.stack([((s * s) * s) * sixth, poly(s) * sixth, poly(t) * sixth, ((t * t) * t) * sixth])


def dweights_f32(t):
    R = t.dtype.type
    s = R(1) - t
    half = R(0.5)

    def dpoly(r):
        return (R(3) * r - R(4)) * r

    return np.stack([-((s * s) * half), dpoly(t) * half, -(dpoly(s) * half), (t * t) * half])


def taps(u, dt):
    """Per axis a, (k, f, t, clamped, nan) for the positions of u (N, d, *sp)."""
    sp = u.shape[2:]
    idx = np.indices(sp)
    return [axis(sample_pos(np.broadcast_to(idx[a], (u.shape[0],) + sp), dt, u[:, a]), sp[a]) for a in range(len(sp))]


def _terms(C, u, dt, wfun=weights):
    """Yields (index tuple into (N or 1 broadcast item, *sp) of the tap, weight (N, *sp)) for the 4^d taps, first axis
    slowest, the weight (w_x w_y) w_z (w_y w_z in 2D) in wfun's precision."""
    N, d = u.shape[0], u.shape[1]
    tp = taps(u, dt)
    w = [wfun(x[2]) for x in tp]
    for q in itertools.product(range(4), repeat=d):
        wq = w[0][q[0]] * w[1][q[1]]
        if d == 3:
            wq = wq * w[2][q[2]]
        yield tuple(tp[a][0][q[a]] for a in range(d)), wq


def interp(C, u, dt=1.0):
    """C (N or 1, K, *sp) float64 coefficients, u (N, d, *sp) float32 / float64 -> (N, K, *sp) float64."""
    N, d, sp = u.shape[0], u.shape[1], u.shape[2:]
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (N,) + C.shape[1:])
    item = np.arange(N).reshape((N,) + (1,) * d)
    out = np.zeros((N, C.shape[1]) + sp)
    with np.errstate(invalid="ignore"):
        for where, w in _terms(C, u, dt):
            out += w[:, None] * np.moveaxis(C[(item, slice(None)) + where], -1, 1)
    return out


def interp_cubic(I, u, dt=1.0):
    return interp(prefilter(I), u, dt)


def grad_u(go, C, u, dt=1.0):
    """d_u (N, d, *sp) float64 for grad_out go (N, K, *sp)."""
    N, d, sp = u.shape[0], u.shape[1], u.shape[2:]
    C = np.broadcast_to(np.asarray(C, dtype=np.float64), (N,) + C.shape[1:])
    go = np.asarray(go, dtype=np.float64)
    item = np.arange(N).reshape((N,) + (1,) * d)
    tp = taps(u, dt)
    w = [weights(x[2]) for x in tp]
    dw = [dweights(x[2]) for x in tp]
    out = np.zeros((N, d) + sp)
    anynan = np.zeros((N,) + sp, dtype=bool)
    for x in tp:
        anynan |= x[4]
    with np.errstate(invalid="ignore"):
        for q in itertools.product(range(4), repeat=d):
            where = tuple(tp[a][0][q[a]] for a in range(d))
            val = (np.moveaxis(C[(item, slice(None)) + where], -1, 1) * go).sum(1)   # sum_k g_k C_k at the tap
            for a in range(d):
                fac = np.ones((N,) + sp)
                for b in range(d):
                    fac = fac * (dw[b][q[b]] if b == a else w[b][q[b]])
                out[:, a] += dt * fac * val
    for a in range(d):
        out[:, a] = np.where(tp[a][3], 0.0, out[:, a])
        out[:, a] = np.where(anynan, np.nan, out[:, a])
    return out


def grad_C_wide(go, Cshape, u, dt=1.0, wfun=weights, add_dtype=np.float64):
    """(sum, sabs, count), each of shape Cshape: per cell of d_C the sum of the contributions w g, the sum of their
    magnitudes and their number.  A voxel with a NaN coordinate adds nothing; broadcast C (Cshape[0] == 1 < N): summed
    over the items.  wfun / add_dtype: with weights_f32 and np.float32 the same walk in the kernel's own precision (the
    products (w_x w_y) w_z, then times g, and the adds tap by tap, voxels in order -- ONE possible order of the atomics)."""
    N, d, sp = u.shape[0], u.shape[1], u.shape[2:]
    K = Cshape[1]
    go = np.asarray(go)
    g = go.astype(add_dtype)
    s = np.zeros(Cshape, dtype=add_dtype)
    sabs = np.zeros(Cshape)
    count = np.zeros(Cshape)
    anynan = np.zeros((N,) + sp, dtype=bool)
    for x in taps(u, dt):
        anynan |= x[4]
    ok = ~anynan
    item = np.broadcast_to(np.arange(N).reshape((N,) + (1,) * d), (N,) + sp)
    if Cshape[0] == 1:
        item = np.zeros_like(item)
    for where, w in _terms(None, u, dt, wfun):
        at = (item[ok],) + tuple(x[ok] for x in where)
        for k in range(K):
            contrib = (w[ok].astype(add_dtype) * g[:, k][ok]).astype(add_dtype)
            np.add.at(s[:, k], at, contrib)
            np.add.at(sabs[:, k], at, np.abs(contrib.astype(np.float64)))
            np.add.at(count[:, k], at, 1.0)
    return s, sabs, count


def weights_wide(t):
    return weights(t, np.longdouble)


UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def cell_bound(sabs, count, dtype, d):
    """tests/scatter_bound.py's bound with this operator's rounding count: for a cell with n contributions of total
    magnitude A, k = n + 9 d and bound = k u / (1 - k u) A + n tiny.  Each contribution w_x w_y [w_z] g of the yardstick
    is the exact cubic weights at the t the library forms, times g.  On the library's path it picks up at most 8 u per
    axis in the weight (bspline_weights.hpp derives 7.5 u from its own expressions), d - 1 weight products and the
    product with g, n - 1 rounded additions in any order, and one for the yardstick's own rounding:
    8 d + d + (n - 1) + 1 = n + 9 d factors (1 + delta), |delta| <= u (Higham, Lemma 3.1)."""
    dtype = np.dtype(dtype)
    u, tiny = UNIT[dtype], float(np.finfo(dtype).tiny)
    n = np.asarray(count, dtype=np.float64)
    ku = (n + 9.0 * d) * u
    assert (ku < 1.0).all()
    return ku / (1.0 - ku) * np.asarray(sabs, dtype=np.float64) + n * tiny


def cell_ratio(got, wide, dtype, d):
    """max over the cells of |got - sum| / bound (0 where the error is 0), and whether every empty cell holds exactly 0."""
    s, sabs, count = wide
    work = np.longdouble if np.dtype(dtype) == np.float64 else np.float64
    err = np.abs(np.asarray(got).astype(work) - s.astype(work)).astype(np.float64)
    bound = cell_bound(sabs, count, dtype, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()), bool((np.asarray(got)[count == 0] == 0).all())


# ---- cases

def image(N, K, sp, dtype, seed=0):
    rng = np.random.default_rng([seed, N, K, *sp])
    return rng.standard_normal((N, K) + tuple(sp)).astype(dtype)
