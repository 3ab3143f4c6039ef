"""numpy reference of the image pyramid (lagomorph_amd/pyramid.py): dense per-axis matrices built from the definition,
independent of lagomorph_amd/csrc/pyramid_weights.hpp.

Per axis with fine extent n >= 1 and coarse extent m = (n + 1) // 2:

    R (m x n)   (R a)[j] = sum_{k=-2..2} w_k a[clamp(2 j + k, 0, n - 1)],  w = (1, 4, 6, 4, 1) / 16
    E (n x m)   (E c)[2 j] = c[j],  (E c)[2 j + 1] = (c[j] + c[min(j + 1, m - 1)]) / 2

OPS names the four operators; `reference` applies the tensor product of an operator's per-axis matrices in float64 (or
long double), `abs_reference` the same with |M| and |a| (the scale of the rounding bound), and `native` restates the
ONE evaluation order of the header in the array's own precision: it must give the emulator's and the kernels' bits.

CASES are the smallest shapes that reach every path of the kernels' tile, 8 x 8 x 64 fine voxels in 3D and 64 x 64 in
2D (4 x 4 x 32 and 32 x 32 coarse): odd and even extents, extents of 1 and 2, a wave's edge on the contiguous axis
(63 / 64 / 65 coarse or fine), and at least two tiles plus a partial one on every axis.  The shipped tile is the one
the shapes were proposed for, so no axis had to be enlarged."""
import numpy as np

OPS = ("reduce", "reduce_adjoint", "expand", "expand_adjoint")
DOWN = ("reduce", "expand_adjoint")          # fine in, coarse out
CASES_3D = ((1, 1, 1), (2, 3, 1), (5, 4, 7), (9, 17, 65), (17, 10, 129), (16, 16, 128), (18, 19, 130))
CASES_2D = ((1, 1), (2, 3), (64, 64), (65, 127), (130, 66))
CASES = CASES_3D + CASES_2D
BATCHES = (1, 2)


def channels(dim):
    return (1, dim, 4)


def coarse_shape(shape):
    return tuple((n + 1) // 2 for n in shape)


def reduce_matrix(n):
    m = (n + 1) // 2
    M = np.zeros((m, n))
    for j in range(m):
        for k, w in zip(range(-2, 3), (1, 4, 6, 4, 1)):
            M[j, min(max(2 * j + k, 0), n - 1)] += w / 16.0
    return M


def expand_matrix(n):
    m = (n + 1) // 2
    M = np.zeros((n, m))
    for x in range(n):
        j = x // 2
        if x % 2 == 0:
            M[x, j] = 1.0
        else:
            M[x, j] += 0.5
            M[x, min(j + 1, m - 1)] += 0.5
    return M


def axis_matrix(op, n):
    """The per-axis matrix of `op` for an axis of FINE extent n, as (out extent) x (in extent)."""
    M = reduce_matrix(n) if op.startswith("reduce") else expand_matrix(n)
    return M.T if op.endswith("_adjoint") else M


def in_shape(op, shape):
    """Spatial shape of the input of `op` on the fine grid `shape`."""
    return tuple(shape) if op in DOWN else coarse_shape(shape)


def out_shape(op, shape):
    return coarse_shape(shape) if op in DOWN else tuple(shape)


def _contract(M, a, axis):
    return np.moveaxis(np.tensordot(M, a, axes=([1], [axis])), 0, axis)


def reference(op, a, shape, scale=1.0, dtype=np.float64):
    """scale (Mx (x) My (x) Mz) a for a (N, C, *in_shape(op, shape)), summed in `dtype` (float64 or long double)."""
    out = np.asarray(a).astype(dtype)
    assert out.shape[2:] == in_shape(op, shape), (op, out.shape, shape)
    for ax, n in enumerate(shape):
        out = _contract(axis_matrix(op, n).astype(dtype), out, 2 + ax)
    return out * dtype(scale)


def abs_reference(op, a, shape, scale=1.0, dtype=np.float64):
    """|scale| (|Mx| (x) |My| (x) |Mz|) |a|: sum_taps |W| |a| of the rounding bound."""
    out = np.abs(np.asarray(a).astype(dtype))
    for ax, n in enumerate(shape):
        out = _contract(np.abs(axis_matrix(op, n)).astype(dtype), out, 2 + ax)
    return out * dtype(abs(scale))


def _native_axis(op, v, n, axis):
    """One contraction in v's precision, as pyramid_weights.hpp orders it: taps ascending, acc = w_0 v_0, then
    acc = acc + w_t v_t; a tap outside the input's axis weighs 0 and reads the clamped cell (down) or 0 (up)."""
    dt = v.dtype.type
    M = axis_matrix(op, n)   # out x in
    v = np.moveaxis(v, axis, -1)
    nout, nin = M.shape
    o = np.arange(nout)
    down = op in DOWN
    first = 2 * o - 2 if down else o // 2 - 1
    acc = None
    for t in range(5 if down else 3):
        i = first + t
        ok = (i >= 0) & (i < nin)
        ic = np.clip(i, 0, nin - 1)
        w = np.where(ok, M[o, ic], 0.0).astype(dt)
        val = v[..., ic] if down else np.where(ok, v[..., ic], dt(0))
        p = w * val
        acc = p if acc is None else acc + p
    return np.moveaxis(acc, -1, axis)


def native(op, a, shape, scale=1.0):
    """The header's evaluation order in a's own precision: down contracts the last axis first, up the first axis first,
    then the scale, rounded to the precision once."""
    out = np.ascontiguousarray(a)
    dt = out.dtype.type
    axes = range(len(shape))
    for ax in (reversed(axes) if op in DOWN else axes):
        out = _native_axis(op, out, shape[ax], 2 + ax)
    return dt(scale) * out


def header_roundings(dim):
    """K, the header's own count of roundings per output element (lagomorph_amd/csrc/pyramid_weights.hpp:
    kPyrRoundings), read from its text -- the only thing this module takes from the header."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lagomorph_amd", "csrc", "pyramid_weights.hpp")
    a, b = re.search(r"kPyrRoundings\(int dim\) \{ return (\d+) \* dim \+ (\d+); \}", open(path).read()).groups()
    return int(a) * dim + int(b)


def real_field(nn, nc, shape, dtype, seed=0):
    """Image-like values, uniform in [0, 1)."""
    rng = np.random.default_rng(seed)
    return rng.random((nn, nc) + tuple(shape)).astype(dtype)


def integer_field(nn, nc, shape, dtype, seed=0):
    """Integer values in [-512, 512]: every partial sum of the four operators is exact in float32."""
    rng = np.random.default_rng(seed)
    return rng.integers(-512, 513, size=(nn, nc) + tuple(shape)).astype(dtype)
