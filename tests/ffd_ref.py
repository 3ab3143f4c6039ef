"""The numpy reference for ffd_expand and its adjoint (include/lagomorph_hip.h), in float64 (long double on request),
the float32 restatement of lagomorph_amd/csrc/ffd_weights.hpp and of the kernels' sums, and the two error bounds the
GPU tests use.

Per spatial axis with extent n and integer spacing s: m = (n - 1) // s + 4 control points, point j at voxel (j - 1) s;
voxel x has i = x // s, r = x % s, t = R(r) / R(s) in the field's precision R, taps i ... i + 3 with the weights
((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6.  That is an n x m matrix W per axis;

    expand:   out[n, k, x, y, z] = sum_{a, b, c} Wx[x, a] Wy[y, b] Wz[z, c] ctrl[n, k, a, b, c]
    adjoint:  d_ctrl[n, k, a, b, c] = sum_{x, y, z} Wx[x, a] Wy[y, b] Wz[z, c] g[n, k, x, y, z]

The reference forms the weights in float64 (or long double) from the SAME t the library forms -- the definition puts
the one rounded division into R -- so that the bounds below count the roundings of the weights' polynomials and of the
sums, and nothing else.
"""
import numpy as np

import bspline_ref

UNIT = bspline_ref.UNIT
MAX_SPACING = 32


def spacing_tuple(spacing, d):
    return (spacing,) * d if isinstance(spacing, int) else tuple(spacing)


def grid_shape(shape, spacing):
    return tuple((n - 1) // s + 4 for n, s in zip(shape, spacing_tuple(spacing, len(shape))))


def axis_t(n, s, dtype):
    """(i, t): the cell of every voxel and r / s rounded once in `dtype`."""
    x = np.arange(n)
    R = np.dtype(dtype).type
    return x // s, (x % s).astype(dtype) / R(s)


def W(n, s, dtype=np.float64, work=np.float64):
    """The (n, m) matrix of one axis in `work`, from t in `dtype`."""
    i, t = axis_t(n, s, dtype)
    w = bspline_ref.weights(t, work)   # (4, n)
    M = np.zeros((n, (n - 1) // s + 4), dtype=work)
    for q in range(4):
        M[np.arange(n), i + q] = w[q]
    return M


def _apply(mats, f, work, transpose):
    out = np.asarray(f, dtype=work)
    for a, M in enumerate(mats):
        M = M.T if transpose else M
        out = np.moveaxis(np.tensordot(M, np.moveaxis(out, 2 + a, 0), 1), 0, 2 + a)
    return np.ascontiguousarray(out)


def expand(ctrl, shape, spacing, tdtype=None, work=np.float64):
    """ctrl (N, C, *m) -> (N, C, *shape) in `work`; the t of the weights in `tdtype` (default: ctrl's dtype)."""
    tdtype = ctrl.dtype if tdtype is None else tdtype
    sp = spacing_tuple(spacing, len(shape))
    assert tuple(ctrl.shape[2:]) == grid_shape(shape, sp)
    return _apply([W(n, s, tdtype, work) for n, s in zip(shape, sp)], ctrl, work, False)


def adjoint(g, spacing, tdtype=None, work=np.float64):
    """g (N, C, *sp) -> (N, C, *m) in `work`."""
    tdtype = g.dtype if tdtype is None else tdtype
    shape = g.shape[2:]
    sp = spacing_tuple(spacing, len(shape))
    return _apply([W(n, s, tdtype, work) for n, s in zip(shape, sp)], g, work, True)


# ---- the header's expressions and the kernels' sums, operation by operation in the field's precision

def weights_native(r, s, dtype):
    """(t, w (4, ...)) as ffd_weights.hpp forms them: t = R(r) / R(s), then bspline_weights.hpp's expressions."""
    R = np.dtype(dtype).type
    t = np.asarray(r).astype(dtype) / R(s)
    return t, bspline_ref.weights_f32(t)


def _fma(a, b, c):
    """fl(a b + c) for float32 operands (the product is exact in float64; the double rounding of the sum is one more
    admissible rounding for the bounds); float64 operands: two roundings, the unfused form."""
    if a.dtype == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def expand_native(ctrl, shape, spacing):
    """The forward kernel's order in ctrl's precision: the axes one after the other, first axis first, each 4-tap sum
    as the tap-0 product and one fma per further tap, ascending."""
    sp = spacing_tuple(spacing, len(shape))
    out = np.asarray(ctrl)
    dtype = out.dtype
    for a, (n, s) in enumerate(zip(shape, sp)):
        x = np.arange(n)
        i = x // s
        _, w = weights_native(x % s, s, dtype)
        v = np.moveaxis(out, 2 + a, -1)
        acc = w[0] * v[..., i]
        for q in range(1, 4):
            acc = _fma(np.broadcast_to(w[q], acc.shape), v[..., i + q], acc)
        out = np.moveaxis(acc, -1, 2 + a)
    assert out.dtype == dtype
    return np.ascontiguousarray(out)


def adjoint_native(g, spacing):
    """The adjoint kernels' order with one tile per axis, in g's precision: last axis first; per control point the taps
    q = 0 .. 3 in order (cell = point - q), the voxels of a cell ascending, acc = fma(w, v, acc) from 0."""
    out = np.asarray(g)
    dtype = out.dtype
    shape = out.shape[2:]
    sp = spacing_tuple(spacing, len(shape))
    for a in reversed(range(len(shape))):
        n, s = shape[a], sp[a]
        m = (n - 1) // s + 4
        _, w = weights_native(np.arange(s), s, dtype)   # (4, s)
        v = np.moveaxis(out, 2 + a, -1)
        res = np.zeros(v.shape[:-1] + (m,), dtype=dtype)
        for j in range(m):
            acc = np.zeros(v.shape[:-1], dtype=dtype)
            for q in range(4):
                cell = j - q
                for x in range(max(cell * s, 0), min(cell * s + s, n)):
                    acc = _fma(np.broadcast_to(w[q, x - cell * s], acc.shape), v[..., x], acc)
            res[..., j] = acc
        out = np.moveaxis(res, -1, 2 + a)
    assert out.dtype == dtype
    return np.ascontiguousarray(out)


# ---- bounds

def voxel_K(d):
    """Roundings between the yardstick (exact weights at the library's t, exact sums) and a voxel of the forward
    kernel, along any one of its 4^d terms: per axis the weight (within 8 u of the exact cubic: bspline_weights.hpp
    derives 7.5 u), its product with the value and at most 3 additions of the 4-tap sum (the fma form has fewer
    roundings, never more) -- 12 per axis -- plus one for the yardstick's own rounding to its working precision and
    one of slack for the second-order terms: K = 12 d + 2, 38 in 3D and 26 in 2D.  (The caps an any-order kernel
    would need are 96 and 40.)"""
    K = 12 * d + 2
    assert K <= (96 if d == 3 else 40)
    return K


def voxel_bound(ctrl, shape, spacing, dtype):
    """Per voxel K u sum_taps w |ctrl|."""
    d = len(shape)
    return voxel_K(d) * UNIT[np.dtype(dtype)] * expand(np.abs(np.asarray(ctrl, dtype=np.float64)), shape, spacing, tdtype=dtype)


def support_counts(n, s):
    """Per control point of one axis the number of voxels whose taps include it."""
    m = (n - 1) // s + 4
    cnt = np.zeros(m)
    i = np.arange(n) // s
    for q in range(4):
        np.add.at(cnt, i + q, 1.0)
    return cnt


def entry_bound(g, spacing, dtype):
    """Per control point (T_j + 32) u sum_x W[x, j] |g[x]|, T_j the voxels in its support: the any-order summation bound
    (T_j - 1 additions) plus the three weights at 8 u, the products and the yardstick's rounding."""
    shape = g.shape[2:]
    sp = spacing_tuple(spacing, len(shape))
    T = np.ones(())
    for n, s in zip(shape, sp):
        T = np.multiply.outer(T, support_counts(n, s))
    return (T + 32.0) * UNIT[np.dtype(dtype)] * adjoint(np.abs(np.asarray(g, dtype=np.float64)), sp, tdtype=dtype)


def worst_ratio(err, bound):
    """max |err| / bound, 0 where the error is 0 (a bound of 0 with an error is inf)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max())


# ---- cases

def field(N, C, sp, dtype, seed=0):
    return bspline_ref.image(N, C, tuple(sp), dtype, seed=seed)


# (shape, spacing): the GPU test's shapes.  The kernels' tiles are 8 x 8 x 64 voxels (2D: 64 x 64), so the two
# tile-boundary shapes of the issue, (70, 37, 41) and (33, 70), have one axis enlarged -- 41 -> 75 and 33 -> 97 -- to
# give every axis at least two tiles and a partial one.
CASES = (
    ((5, 6, 7), (2, 3, 4)),
    ((9, 11), (4, 1)),
    ((3, 4, 5), 8),
    ((1, 6, 3), (5, 2, 2)),
    ((9, 9, 9), 4),
    ((70, 37, 75), (5, 3, 7)),
    ((97, 70), (32, 7)),
    ((3, 4, 63), 3),
    ((3, 4, 64), 3),
    ((3, 4, 65), 3),
    ((5, 4, 6), 1),   # s = 1 on every axis of a 3D field: the largest LDS box (more than 64 KB in float64)
)
