"""Test-side reference for the image gradient of affine_interp_backward (numpy, no GPU): the splat of
cuda/affine.cu:171-536 with every TERM formed as the kernels and the oracle form it, and the terms of a cell summed
in float64 -- with the term count n and S = sum |term| per cell, so that a result can be judged cell by cell:

    |any float summation of those n terms, plus one final rounding, - exact sum|  <=  u (n + 1) S,

the textbook bound for n floating adds in ANY order (each add errs by at most u times a partial sum, and every partial
sum is at most S in magnitude; window sums kept in double and rounded once are inside it as well).  The float64 sum
here is off from the exact one by at most 2^-53 n S, eight orders below the float32 bound.

  * positions: h = A (x - o) + T + o with the fma chain of cuda/affine.cu:42-61, o = .5 * (n - 1) (as oracle/
    lago_oracle_impl.h restates it);
  * floor / clamp: include/interp.h:64-70, include/extrap.h:41-57;
  * weights: the sequentially flipped dx, dy, dz of include/interp.h:426-454, term = (dx * dy * dz) * grad_out.

Float32 only.  numpy's float32 arithmetic rounds every operation and never contracts; a fused multiply-add is emulated
as float32(float64(a) * float64(b) + float64(c)): the product of two float32 is exact in double, so only the double
rounding of the sum can differ from a true fma, on a near-tie -- tests/test_affine_ref.py pins the positions against
the oracle's forward bit for bit on the inputs the suite uses.  Float64 inputs would need an exact double fma and an
accumulator wider than double for the bound to be a derivation; they stay on the comparison with the oracle.
"""
import numpy as np

F = np.float32
U32 = 2.0 ** -24


def _fma(a, b, c):
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    return (a * b + c).astype(F)


def _half_extent(n):
    return F(0.5 * np.float64(F(n - 1)))


def positions(A, T, shape):
    """hx, hy, hz of shape `shape` for one item: A (3, 3), T (3,), float32."""
    A, T = np.asarray(A, F), np.asarray(T, F)
    nx, ny, nz = shape
    ox, oy, oz = _half_extent(nx), _half_extent(ny), _half_extent(nz)
    fi = (np.arange(nx, dtype=F) - ox)[:, None, None]
    fj = (np.arange(ny, dtype=F) - oy)[None, :, None]
    fk = (np.arange(nz, dtype=F) - oz)[None, None, :]
    out = []
    for d, o in enumerate((ox, oy, oz)):
        a0, a1, a2 = A[d]
        inner = _fma(a0, fi, a1 * fj)   # LG_FMA(A0, fi, A1 * fj)
        h = _fma(a2, fk, inner)         # LG_FMA(A2, fk, .)
        out.append(((h + T[d]) + o).astype(F))
    return out


def _floor(x):
    """include/interp.h:64-70 with the oracle's saturation at +-2^30."""
    return np.floor(np.clip(x, F(-1073741824.0), F(1073741824.0))).astype(np.int64)


def forward(I, A, T):
    """affine_interp_forward (cuda/affine.cu:23-112, triLerp of include/interp.h:60-123) from the positions, floors and
    clamps above.  I: (nn or 1, nc, nx, ny, nz) float32."""
    I = np.ascontiguousarray(I, F)
    nn, shape = A.shape[0], I.shape[2:]
    out = np.empty((nn, I.shape[1]) + shape, F)
    for n in range(nn):
        hx, hy, hz = positions(A[n], T[n], shape)
        f = [_floor(h) for h in (hx, hy, hz)]
        t, u, v = [(h - fl.astype(F)).astype(F) for h, fl in zip((hx, hy, hz), f)]
        omt, omu, omv = F(1) - t, F(1) - u, F(1) - v
        lo, hi = [], []
        for fl, size in zip(f, shape):   # clampBackground on (floor, floor + 1)
            lo.append(np.clip(fl, 0, size - 1))
            hi.append(np.clip(fl + 1, 0, size - 1))
        In = I[0 if I.shape[0] == 1 else n]
        for c in range(I.shape[1]):
            at = lambda a, b, cc: In[c][tuple(np.broadcast_arrays(a, b, cc))]
            (fx, fy, fz), (cx, cy, cz) = lo, hi
            v0, v1, v2, v3 = at(fx, fy, fz), at(cx, fy, fz), at(cx, cy, fz), at(fx, cy, fz)
            v4, v5, v6, v7 = at(fx, fy, cz), at(cx, fy, cz), at(cx, cy, cz), at(fx, cy, cz)
            b = np.broadcast_to
            s = v0.shape
            T_, U_, V_, OT, OU, OV = (b(w, s) for w in (t, u, v, omt, omu, omv))
            low = _fma(OU, _fma(OT, v0, T_ * v1), U_ * _fma(OT, v3, T_ * v2))
            high = _fma(OU, _fma(OT, v4, T_ * v5), U_ * _fma(OT, v7, T_ * v6))
            out[n, c] = _fma(OV, low, V_ * high)
    return out


def terms(A, T, shape):
    """For one item: the eight (flat target cell, weight) pairs of every source, in the splat's order (x outer, y, z
    inner; include/interp.h:426-454): a list of eight (cell (nv,) int64, weight (nv,) float32)."""
    nx, ny, nz = shape
    hx, hy, hz = (np.broadcast_to(h, shape) for h in positions(A, T, shape))
    fx, fy, fz = _floor(hx), _floor(hy), _floor(hz)
    dx = F(1) - (hx - fx.astype(F))
    dy = F(1) - (hy - fy.astype(F))
    dz = F(1) - (hz - fz.astype(F))
    out = []
    for a in range(2):
        i = np.clip(fx + a, 0, nx - 1)
        for b in range(2):
            j = np.clip(fy + b, 0, ny - 1)
            for c in range(2):
                k = np.clip(fz + c, 0, nz - 1)
                w = (dx * dy) * dz
                out.append((((i * ny + j) * nz + k).reshape(-1), w.astype(F).reshape(-1)))
                dz = F(1) - dz
            dy = F(1) - dy
        dx = F(1) - dx
    return out


def backward_dI(go, A, T, bc):
    """(sum float64, n int64, S float64), each shaped like d_I: (1 if bc else nn, nc, nx, ny, nz)."""
    go = np.ascontiguousarray(go, F)
    nn, nc = go.shape[:2]
    shape = go.shape[2:]
    nv = int(np.prod(shape))
    lead = 1 if bc else nn
    tot = np.zeros((lead, nc, nv))
    cnt = np.zeros((lead, nc, nv), np.int64)
    mag = np.zeros((lead, nc, nv))
    for n in range(nn):
        m = 0 if bc else n
        tw = terms(A[n], T[n], shape)
        for cell, w in tw:
            c1 = np.bincount(cell, minlength=nv)
            for c in range(nc):
                term = (w * go[n, c].reshape(-1)).astype(F).astype(np.float64)   # rounded in float32, as the kernels do
                tot[m, c] += np.bincount(cell, weights=term, minlength=nv)        # (bincount adds in float64)
                mag[m, c] += np.bincount(cell, weights=np.abs(term), minlength=nv)
                cnt[m, c] += c1
    full = (lead, nc) + tuple(shape)
    return tot.reshape(full), cnt.reshape(full), mag.reshape(full)


def bound(n, S, u=U32):
    return u * (n + 1.0) * S


def worst_ratio(got, ref):
    """max over cells of |got - sum| / (u (n + 1) S); a cell that no term reaches (S = 0) must be exactly zero (inf
    otherwise).  Also returns the cell."""
    tot, n, S = ref
    got = np.asarray(got, np.float64)
    assert got.shape == tot.shape, (got.shape, tot.shape)
    err = np.abs(got - tot)
    lim = bound(n, S)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0))
    at = np.unravel_index(np.argmax(r), r.shape)
    return float(r[at]), at


def sensitive(n, u=U32):
    """A cell where one missing term of average size exceeds the bound sixteen times: n (n + 1) u <= 1 / 16."""
    n = np.asarray(n, np.float64)
    return n * (n + 1.0) * u <= 1.0 / 16.0


def interior(shape):
    """mask of the cells that are not on a face of the grid."""
    m = np.zeros(shape, bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m
