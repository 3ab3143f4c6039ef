"""Test-side float64 reference of the Parzen joint histogram, mutual information and their backward (numpy only; nothing
of the product is imported), and the list of cases the tests share.

Per image with range (lo, hi) and B bins, in double and in exactly this order (numpy fuses nothing):

    s  = (B - 3) / (hi - lo)
    vc = fmin(fmax(v, lo), hi)                     (a NaN voxel becomes lo)
    c  = (vc - lo) * s + 1
    k  = min(floor(c), B - 3) - 1                  (then clamped as an integer to [0, B - 4])
    t  = c - (k + 1),  u = 1 - t
    w0 = u u u / 6   w1 = ((3 t - 6) t t + 4) / 6   w2 = (((-3 t + 3) t + 3) t + 1) / 6   w3 = t t t / 6
    w0' = -(u u) / 2 s   w1' = (3 t - 4) t / 2 s   w2' = ((-3 t + 2) t + 1) / 2 s   w3' = t t / 2 s   (0 unless lo <= v <= hi)

    H[kI + a][kJ + b] += rint(wI_a wJ_b 2^32)  as int64,    P = H / (nvox 2^32)
    a = P.sum(-1), b = P.sum(-2);  H_I = -sum a log(a + eps), H_J = -sum b log(b + eps), H_IJ = -sum P log(P + eps)
    MI = H_I + H_J - H_IJ,  NMI = (H_I + H_J) / H_IJ     (every sum in the fixed order of fold_sum)
    dI(x) = (sum_a wI_a' (sum_b wJ_b G[kI + a][kJ + b])) / nvox,  dJ with the roles swapped    (G = dL/dP)

tests/test_mi_host.py holds the gradient against central differences and the C++ header against the integers here."""
import numpy as np

ONE = 4294967296.0                              # 2^32
EPS = 1e-10


def window(v, rng, B):
    """(k int64, w (..., 4), dw (..., 4)) of the values v (any shape) for the range rng = (lo, hi)."""
    lo, hi = float(rng[0]), float(rng[1])
    v = np.asarray(v, dtype=np.float64)
    s = float(B - 3) / (hi - lo)
    with np.errstate(invalid="ignore"):
        vc = np.fmin(np.fmax(v, lo), hi)
        inside = (v >= lo) & (v <= hi)
    c = (vc - lo) * s + 1.0
    k = np.clip((np.minimum(np.floor(c), float(B - 3)) - 1.0).astype(np.int64), 0, B - 4)
    t = c - (k + 1).astype(np.float64)
    u = 1.0 - t
    w = np.stack([u * u * u / 6.0, ((3.0 * t - 6.0) * t * t + 4.0) / 6.0, (((-3.0 * t + 3.0) * t + 3.0) * t + 1.0) / 6.0,
                  t * t * t / 6.0], axis=-1)
    dw = np.stack([-(u * u) / 2.0 * s, (3.0 * t - 4.0) * t / 2.0 * s, ((-3.0 * t + 2.0) * t + 1.0) / 2.0 * s,
                   t * t / 2.0 * s], axis=-1)
    dw = np.where(inside[..., None], dw, 0.0)
    return k, w, dw


def _rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(x.shape[0] * x.shape[1], -1)


def auto_range(x):
    """What a range of None means: (min, max) of the whole tensor, (lo, lo + 1) for a constant one."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return 0.0, 1.0
    lo, hi = float(x.min()), float(x.max())
    return (lo, hi) if lo < hi else (lo, lo + 1.0)


def histogram_int(I, J, B, range_I, range_J):
    """The fixed-point table (rows, B, B) as exact int64 sums.  The route: every product is an integer below 2^32, cut into
    its low 16 bits and the rest; np.bincount sums each part in double, exactly (below 2^30 x 2^16 = 2^46 a bin), and the
    two sums are joined as integers.  It agrees with np.add.at on int64 (tests/test_mi_host.py) and takes seconds at
    128^3."""
    Ir, Jr = _rows(I), _rows(J)
    H = np.zeros((Ir.shape[0], B, B), dtype=np.int64)
    for r in range(Ir.shape[0]):
        kI, wI, _ = window(Ir[r], range_I, B)
        kJ, wJ, _ = window(Jr[r], range_J, B)
        for a in range(4):
            for b in range(4):
                q = np.rint(wI[:, a] * wJ[:, b] * ONE).astype(np.int64)
                idx = (kI + a) * B + (kJ + b)
                lo = np.bincount(idx, weights=(q & 0xFFFF).astype(np.float64), minlength=B * B)
                hi = np.bincount(idx, weights=(q >> 16).astype(np.float64), minlength=B * B)
                H[r] += ((hi.astype(np.int64) << 16) + lo.astype(np.int64)).reshape(B, B)
    return H


def histogram_int_add_at(I, J, B, range_I, range_J):
    """The same table by np.add.at on int64 (slow, small cases): the plain statement of the definition."""
    Ir, Jr = _rows(I), _rows(J)
    H = np.zeros((Ir.shape[0], B, B), dtype=np.int64)
    for r in range(Ir.shape[0]):
        kI, wI, _ = window(Ir[r], range_I, B)
        kJ, wJ, _ = window(Jr[r], range_J, B)
        for a in range(4):
            for b in range(4):
                np.add.at(H[r], (kI + a, kJ + b), np.rint(wI[:, a] * wJ[:, b] * ONE).astype(np.int64))
    return H


def P_of(H, nvox):
    return H.astype(np.float64) / (float(nvox) * ONE)


def histogram_float(I, J, B, range_I, range_J):
    """The unquantised P (rows, B, B): float sums of wI_a wJ_b / nvox (what the analytic gradient differentiates)."""
    Ir, Jr = _rows(I), _rows(J)
    P = np.zeros((Ir.shape[0], B * B))
    for r in range(Ir.shape[0]):
        kI, wI, _ = window(Ir[r], range_I, B)
        kJ, wJ, _ = window(Jr[r], range_J, B)
        for a in range(4):
            for b in range(4):
                P[r] += np.bincount((kI + a) * B + (kJ + b), weights=wI[:, a] * wJ[:, b], minlength=B * B)
    return P.reshape(-1, B, B) / Ir.shape[1]


def joint_histogram(I, J, B, range_I, range_J):
    """P (N, C, B, B) of the definition (fixed point)."""
    I = np.asarray(I)
    nvox = int(np.prod(I.shape[2:]))
    return P_of(histogram_int(I, J, B, range_I, range_J), nvox).reshape(I.shape[:2] + (B, B))


def fold_sum(x):
    """The sum over the last axis in the order the definition fixes: padded with zeros to a power of two, then the upper
    half added onto the lower half until one entry is left."""
    n = 1
    while n < x.shape[-1]:
        n *= 2
    x = np.concatenate([x, np.zeros(x.shape[:-1] + (n - x.shape[-1],))], axis=-1)
    while n > 1:
        n //= 2
        x = x[..., :n] + x[..., n:]
    return x[..., 0]


def mi_of(P, normalized=False, eps=EPS):
    """(MI or NMI (...,), G = d(MI or NMI)/dP (..., B, B)) of tables P (..., B, B); every sum by fold_sum, the last axis
    of P first in H_IJ."""
    a, b = fold_sum(P), fold_sum(np.swapaxes(P, -1, -2))
    h_i = -fold_sum(a * np.log(a + eps))
    h_j = -fold_sum(b * np.log(b + eps))
    h_ij = -fold_sum(fold_sum(P * np.log(P + eps)))
    d_i = -(np.log(a + eps) + a / (a + eps))[..., :, None]
    d_j = -(np.log(b + eps) + b / (b + eps))[..., None, :]
    d_ij = -(np.log(P + eps) + P / (P + eps))
    if normalized:
        hij = h_ij[..., None, None]
        return (h_i + h_j) / h_ij, (d_i + d_j) / hij - ((h_i + h_j)[..., None, None] / (hij * hij)) * d_ij
    return h_i + h_j - h_ij, d_i + d_j - d_ij


def backward(G, I, J, B, range_I, range_J):
    """(dI, dJ), shaped like I, for G = dL/dP (N, C, B, B) or (rows, B, B); the sums in the order of the definition."""
    I = np.asarray(I, dtype=np.float64)
    Ir, Jr = _rows(I), _rows(J)
    G = np.asarray(G, dtype=np.float64).reshape(-1, B, B)
    nvox = float(Ir.shape[1])
    dI, dJ = np.zeros_like(Ir), np.zeros_like(Jr)
    for r in range(Ir.shape[0]):
        kI, wI, dwI = window(Ir[r], range_I, B)
        kJ, wJ, dwJ = window(Jr[r], range_J, B)
        g = [[G[r][kI + a, kJ + b] for b in range(4)] for a in range(4)]
        for out, dw, w, tr in ((dI, dwI, wJ, False), (dJ, dwJ, wI, True)):
            acc = None
            for a in range(4):
                inner = w[:, 0] * (g[0][a] if tr else g[a][0])
                for b in range(1, 4):
                    inner = inner + w[:, b] * (g[b][a] if tr else g[a][b])
                acc = dw[:, 0] * inner if a == 0 else acc + dw[:, a] * inner
            out[r] = acc / nvox
    return dI.reshape(I.shape), dJ.reshape(I.shape)


def reference(I, J, B, range_I=None, range_J=None, g=None, normalized=False, eps=EPS):
    """(P, MI, dI, dJ) for the upstream gradient g (N, C) on MI (ones when None); ranges of None as the product takes them."""
    I, J = np.asarray(I, dtype=np.float64), np.asarray(J, dtype=np.float64)
    range_I = auto_range(I) if range_I is None else range_I
    range_J = auto_range(J) if range_J is None else range_J
    P = joint_histogram(I, J, B, range_I, range_J)
    mi, G = mi_of(P, normalized, eps)
    g = np.ones(I.shape[:2]) if g is None else np.asarray(g, dtype=np.float64)
    dI, dJ = backward(G * g[..., None, None], I, J, B, range_I, range_J)
    return P, mi, dI, dJ


def mi_float(I, J, B, range_I, range_J, normalized=False, eps=EPS):
    """MI (rows,) of the unquantised histogram: the function the analytic gradient belongs to."""
    return mi_of(histogram_float(I, J, B, range_I, range_J), normalized, eps)[0]


# ---- the cases tests/test_mi_host.py and tests/test_gpu_mi.py share

BINS = [4, 5, 32, 64]
# (N, C), spatial: ragged tails in 3D and 2D, and a row of 54 120 voxels that several workgroups share
SHAPES = [((2, 2), (5, 6, 7)), ((1, 2), (9, 5, 70)), ((1, 1), (3, 130)), ((1, 2), (33, 40, 41))]
KINDS = ["noise", "smooth", "constant", "same", "clamp", "edges", "nonfinite"]
FD_SHAPES = [((1, 1), (5, 6, 7)), ((1, 1), (3, 130)), ((1, 1), (9, 5, 70))]

_INPUTS = {}


def inputs(lead, sp, kind):
    """(I, J, g, range_I, range_J): float64 arrays of float32-representable values (N, C) + sp (both precisions share one
    reference), the upstream gradient g (N, C) and the ranges handed to the product (None: taken from the tensor).

    noise      I normal, J = 0.8 I + 0.6 N
    smooth     a sum of slow sines and J = cos(3 I): neighbouring voxels share their 16 bins
    constant   I = 0.25, J = -1.5 everywhere: all mass in at most 16 bins
    same       J is I
    clamp      the noise pair with ranges that clamp both ends of both images (about 15 % of the voxels)
    edges      the noise pair cut to [-1, 1] with the range (-1, 1): many voxels exactly at lo and at hi
    nonfinite  the noise pair with a few NaN, +inf and -inf voxels in both images, ranges (-2, 2) and (-1.5, 2.5)"""
    key = (lead, sp, kind)
    if key not in _INPUTS:
        rng = np.random.default_rng([len(sp), *sp, *lead, KINDS.index(kind)])
        shape = tuple(lead) + tuple(sp)
        I, N = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
        g = rng.standard_normal(lead).astype(np.float32)
        J = (np.float32(0.8) * I + np.float32(0.6) * N).astype(np.float32)
        rI = rJ = None
        if kind == "smooth":
            x = np.indices(sp).astype(np.float64)
            I = sum(np.sin(0.11 * (a + 1) * x[a] + 0.3 * a) for a in range(len(sp)))
            I = (I[None, None] + 0.05 * np.arange(shape[0] * shape[1]).reshape(lead + (1,) * len(sp))).astype(np.float32)
            J = np.cos(3.0 * I.astype(np.float64)).astype(np.float32)
        elif kind == "constant":
            I, J = np.full(shape, 0.25, dtype=np.float32), np.full(shape, -1.5, dtype=np.float32)
        elif kind == "same":
            J = I
        elif kind == "clamp":
            rI, rJ = (-1.5, 1.25), (-1.25, 1.75)
        elif kind == "edges":
            I, J = np.clip(I, -1.0, 1.0), np.clip(J, -1.0, 1.0)
            rI = rJ = (-1.0, 1.0)
        elif kind == "nonfinite":
            I, J = I.copy(), J.copy()
            flatI, flatJ = I.reshape(-1), J.reshape(-1)
            where = rng.permutation(flatI.size)[:12]
            for n, bad in enumerate((np.nan, np.inf, -np.inf)):
                flatI[where[4 * n:4 * n + 2]] = bad
                flatJ[where[4 * n + 2:4 * n + 4]] = bad
            flatJ[where[0]] = np.inf   # one voxel bad in both
            rI, rJ = (-2.0, 2.0), (-1.5, 2.5)
        out = (I.astype(np.float64), J.astype(np.float64), g.astype(np.float64))
        for a in out:
            a.setflags(write=False)
        _INPUTS[key] = out + (rI, rJ)
    return _INPUTS[key]


_REFS = {}


def case_reference(lead, sp, kind, B, normalized=False):
    """reference(...) of inputs(lead, sp, kind) at B bins with the case's upstream gradient, computed once."""
    key = (lead, sp, kind, B, normalized)
    if key not in _REFS:
        I, J, g, rI, rJ = inputs(lead, sp, kind)
        r = reference(I, J, B, rI, rJ, g=g, normalized=normalized)
        for a in r:
            a.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]
