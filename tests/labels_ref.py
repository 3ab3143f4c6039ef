"""The numpy restatement of warp_labels and label_overlap (include/lagomorph_hip.h), and the cases the label tests share.

Per axis with extent n and voxel index i, in the displacement's precision R:

    p = i + dt u                 (`sample_pos`: one float32 add for float32 and dt = +-1, else fma(dt, u, i) in float64
                                  narrowed to R -- the fma is restated exactly by `fma`, numpy has none)
    p = fmin(fmax(p, -1), n)
    f = floor(p), t = p - f      (then float64)
    lo = clip(f, 0, n - 1), hi = clip(f + 1, 0, n - 1)

"nearest" takes hi where t > 0.5, else lo.  "vote": corner q (first axis slowest) weighs (a_x a_y) a_z in float64, a
label's score is the sum of the weights of its corners in ascending q from 0.0, the largest score wins and the smallest
label among equal scores.  numpy neither fuses nor reorders, so every bit of this is what the library computes.
"""
import itertools

import numpy as np

MODES = ("nearest", "vote")
LABEL_KINDS = ("random5", "two", "constant", "blobs", "extreme")
DISP_KINDS = ("zero", "shift", "shift_out", "half", "random", "huge", "nonfinite")
DTS = (1.0, -1.0, 0.7)


# ---- fma(a, b, c) in float64, correctly rounded

def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """RN(a b + c) for float64 arrays: the exact product as two doubles, the exact sum of its head and c as two
    doubles, the two tails added with ROUNDING TO ODD, and one last rounded add (Boldo and Melquiond, "Emulation of FMA
    and correctly rounded sums: proved algorithms using rounding to odd", 2008).  Operands that are not finite, or so
    large that the splitting overflows, take a b + c: the result is then not finite either way, or a huge position
    that the clamp sends to the border."""
    a, b, c = (np.asarray(x, dtype=np.float64) for x in np.broadcast_arrays(a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        plain = a * b + c
        ok = np.isfinite(plain) & (np.abs(a) < 1e150) & (np.abs(b) < 1e150) & (np.abs(c) < 1e300)
        aa, bb, cc = np.where(ok, a, 0.0), np.where(ok, b, 0.0), np.where(ok, c, 0.0)
        ph, pl = _two_prod(aa, bb)
        sh, sl = _two_sum(cc, ph)
        vh, vl = _two_sum(sl, pl)
        even = (np.ascontiguousarray(vh).view(np.int64) & 1) == 0
        odd = np.where((vl != 0) & even, np.nextafter(vh, np.where(vl > 0, np.inf, -np.inf)), vh)
        return np.where(ok, sh + odd, plain)


# ---- warp_labels

def sample_pos(i, dt, u):
    """i: integer index array, u: float32 or float64 array of the same shape."""
    R = u.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        if R is np.float32 and dt == 1.0:
            return i.astype(np.float32) + u
        if R is np.float32 and dt == -1.0:
            return i.astype(np.float32) - u
        return fma(np.float64(dt), u.astype(np.float64), i.astype(np.float64)).astype(R)


def axis(p, n):
    """(lo, hi, t) of positions p along an axis of extent n."""
    R = p.dtype.type
    p = np.fmin(np.fmax(p, R(-1)), R(n))
    f = np.floor(p)
    t = (p - f).astype(np.float64)
    fi = f.astype(np.int64)
    return np.clip(fi, 0, n - 1), np.clip(fi + 1, 0, n - 1), t


def taps(u, dt):
    """Per axis a, (lo, hi, t) with the shape (N, *sp) of one component of u (N, d, *sp)."""
    sp = u.shape[2:]
    idx = np.indices(sp)
    return [axis(sample_pos(np.broadcast_to(idx[a], (u.shape[0],) + sp), dt, u[:, a]), sp[a]) for a in range(len(sp))]


def corners(L, u, dt):
    """(labels (N, *sp, 2^d) int64, weights (N, *sp, 2^d) float64) of every sample, corner q with the first axis slowest."""
    N, d, sp = u.shape[0], u.shape[1], u.shape[2:]
    tp = taps(u, dt)
    Ln = np.broadcast_to(L[:, 0].astype(np.int64), (N,) + sp)
    item = np.arange(N).reshape((N,) + (1,) * d)
    labs, ws = [], []
    for bits in itertools.product((0, 1), repeat=d):
        where = tuple(tp[a][1] if b else tp[a][0] for a, b in enumerate(bits))
        labs.append(Ln[(item,) + where])
        fac = [tp[a][2] if b else 1.0 - tp[a][2] for a, b in enumerate(bits)]
        ws.append((fac[0] * fac[1]) * fac[2] if d == 3 else fac[0] * fac[1])
    return np.stack(labs, -1), np.stack(ws, -1)


def scores(c, w):
    """score[..., q]: the sum of w over the corners that carry c[..., q], ascending from 0.0."""
    s = np.zeros(c.shape)
    for r in range(c.shape[-1]):
        s = s + np.where(c[..., r:r + 1] == c, w[..., r:r + 1], 0.0)
    return s


def warp(L, u, dt=1.0, mode="vote"):
    """L (N or 1, 1, *sp) integers, u (N, d, *sp) float32 / float64 -> (N, 1, *sp) in L's dtype."""
    N, d, sp = u.shape[0], u.shape[1], u.shape[2:]
    assert L.shape[1] == 1 and L.shape[2:] == sp and d == len(sp) and L.shape[0] in (1, N) and mode in MODES
    if mode == "nearest":
        tp = taps(u, dt)
        Ln = np.broadcast_to(L[:, 0], (N,) + sp)
        item = np.arange(N).reshape((N,) + (1,) * d)
        out = Ln[(item,) + tuple(np.where(t > 0.5, hi, lo) for lo, hi, t in tp)]
    else:
        c, w = corners(L, u, dt)
        s = scores(c, w)
        out = np.where(s == s.max(-1, keepdims=True), c, np.iinfo(np.int64).max).min(-1)
    return out[:, None].astype(L.dtype)


# ---- label_overlap and dice

def overlap(A, B, K):
    """int64 (N, K, 3): [#(A == k), #(B == k), #(A == k and B == k)], labels outside [0, K) counting in nothing."""
    N = A.shape[0]
    out = np.zeros((N, K, 3), dtype=np.int64)
    for n in range(N):
        a, b = A[n].reshape(-1).astype(np.int64), B[n].reshape(-1).astype(np.int64)
        ina, inb = (a >= 0) & (a < K), (b >= 0) & (b < K)
        out[n, :, 0] = np.bincount(a[ina], minlength=K)
        out[n, :, 1] = np.bincount(b[inb], minlength=K)
        out[n, :, 2] = np.bincount(a[ina & (a == b)], minlength=K)
    return out


def dice(counts, empty=np.nan):
    both = counts[..., 0] + counts[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(both == 0, empty, 2 * counts[..., 2] / both)


# ---- cases

def _smooth(x, passes=3):
    for _ in range(passes):
        for a in range(1, x.ndim):
            x = (np.roll(x, 1, a) + 2 * x + np.roll(x, -1, a)) / 4
    return x


def blobs(rng, N, sp, K):
    """argmax over K channels of smoothed noise: connected structures, label 0..K-1."""
    return np.stack([_smooth(rng.standard_normal((K,) + sp)).argmax(0) for _ in range(N)])[:, None].astype(np.int32)


def labels(kind, N, sp, seed=0):
    """(N, 1, *sp) int32."""
    rng = np.random.default_rng([seed, LABEL_KINDS.index(kind), N, *sp])
    if kind == "random5":
        return rng.integers(0, 5, (N, 1) + sp).astype(np.int32)
    if kind == "two":
        return (rng.integers(0, 2, (N, 1) + sp) * 7 + 3).astype(np.int32)
    if kind == "constant":
        return np.full((N, 1) + sp, 4, dtype=np.int32)
    if kind == "blobs":
        return blobs(rng, N, sp, 6)
    if kind == "extreme":
        return np.array([-2 ** 31, 2035, 2 ** 31 - 1], dtype=np.int64)[rng.integers(0, 3, (N, 1) + sp)].astype(np.int32)
    raise ValueError(kind)


def displacement(kind, N, sp, dtype, seed=0):
    """(N, d, *sp) of dtype."""
    d = len(sp)
    rng = np.random.default_rng([seed, DISP_KINDS.index(kind), N, *sp])
    u = np.zeros((N, d) + sp)
    if kind == "shift":
        for a, s in enumerate((2.0, -1.0, 3.0)[:d]):
            u[:, a] = s
        u[N - 1] *= -1
    elif kind == "shift_out":
        for a, s in enumerate((-40.0, 50.0, -3.0)[:d]):
            u[:, a] = s
        u[N - 1] *= -1
    elif kind == "half":
        u[:] = 0.5
    elif kind in ("random", "huge", "nonfinite"):
        u = 1.7 * rng.standard_normal(u.shape)
        flat = u.reshape(-1)
        special = (1e6, -1e6, 3e9, -3e9) if kind == "huge" else (np.nan, np.inf, -np.inf)
        if kind != "random":
            at = rng.permutation(flat.size)[:2 * len(special)]
            flat[at] = np.tile(special, 2)[:at.size]
    elif kind != "zero":
        raise ValueError(kind)
    return u.astype(dtype)


def warp_cases(N, sp, dtype):
    """(label kind, displacement kind, dt, L (N, 1, *sp) int32, u (N, d, *sp)) for every combination."""
    for lk in LABEL_KINDS:
        L = labels(lk, N, sp)
        for dk in DISP_KINDS:
            u = displacement(dk, N, sp, dtype)
            for dt in DTS:
                yield lk, dk, dt, L, u
