"""Numpy reference of lagomorph_amd.distance: the feature predicates, the separable squared Euclidean distance transform
and the surface distances.

The transform is the recurrence the kernels run, one pass per axis with the last axis first,

    out[i] = min_j g[j] + (s (i - j))^2,

here in int64 at unit spacing (the exact squared distance; NO_FEATURE stands for +inf) and in float64 otherwise.
`brute` is the definition itself: the minimum over all feature voxels.
"""
import numpy as np

WHERES = ("nonzero", "equal", "not_equal", "surface")
KINDS = ("sparse", "dense", "corner", "none", "all", "blobs", "boxes")
NO_FEATURE = np.iinfo(np.int64).max


# ---- features

def surface(m):
    """m and not eroded by the face-connected cross with everything outside the volume counted as background: a voxel
    of m with at least one face neighbour (or the border) outside m.  m: (N, 1, *sp) bool."""
    inner = m.copy()
    for a in range(2, m.ndim):
        p = np.pad(m, [(0, 0)] * a + [(1, 1)] + [(0, 0)] * (m.ndim - a - 1), constant_values=False)
        lo = [slice(None)] * m.ndim
        hi = [slice(None)] * m.ndim
        lo[a], hi[a] = slice(0, -2), slice(2, None)
        inner &= p[tuple(lo)] & p[tuple(hi)]
    return m & ~inner


def features(L, where="nonzero", label=0):
    if where == "nonzero":
        return L != 0
    if where == "equal":
        return L == label
    if where == "not_equal":
        return L != label
    if where == "surface":
        return surface(L == label)
    raise ValueError(where)


# ---- the transform

def _spacing(spacing, d):
    return (float(spacing),) * d if np.ndim(spacing) == 0 else tuple(float(s) for s in spacing)


def _pass(g, axis, cost, none):
    """out[i] = min_j g[j] + cost[i, j] along `axis`; entries equal to `none` stay out of the sums."""
    g = np.moveaxis(g, axis, -1)
    out = np.full_like(g, none)
    for j in range(g.shape[-1]):
        gj = g[..., j:j + 1]
        with np.errstate(over="ignore"):
            out = np.minimum(out, np.where(gj == none, none, gj + cost[:, j]))
    return np.moveaxis(out, -1, axis)


def edt_sq(f, spacing=1.0):
    """The squared distance to the nearest True voxel of f (N, 1, *sp) per item: int64 (NO_FEATURE in an item without
    one) at unit spacing, float64 (+inf) otherwise."""
    d = f.ndim - 2
    sp = _spacing(spacing, d)
    unit = all(s == 1.0 for s in sp)
    none = NO_FEATURE if unit else np.inf
    g = np.where(f, 0, none).astype(np.int64 if unit else np.float64)
    for a in range(d - 1, -1, -1):
        i = np.arange(f.shape[2 + a])
        delta = i[:, None] - i[None, :]
        cost = delta * delta if unit else (sp[a] * delta.astype(np.float64)) ** 2
        g = _pass(g, 2 + a, cost, none)
    return g


def as_float(sq):
    """edt_sq's result as the float64 squared distance (+inf for NO_FEATURE)."""
    if sq.dtype == np.int64:
        return np.where(sq == NO_FEATURE, np.inf, sq.astype(np.float64))
    return sq


def distance_transform(L, where="nonzero", label=0, spacing=1.0, squared=False):
    """What lagomorph_amd.distance_transform returns, float32: at unit spacing bit for bit (the squared distance is an
    exact integer, its root correctly rounded by numpy), otherwise the float64 value rounded once."""
    sq = as_float(edt_sq(features(L, where, label), spacing))
    if np.ndim(spacing) == 0 and float(spacing) == 1.0 or np.ndim(spacing) and all(float(s) == 1.0 for s in spacing):
        sq = sq.astype(np.float32)
        return sq if squared else np.sqrt(sq)
    return (sq if squared else np.sqrt(sq)).astype(np.float32)


def brute(f, spacing=1.0):
    """The definition: per voxel the minimum over ALL feature voxels of the item (int64 / float64 as edt_sq)."""
    d = f.ndim - 2
    sp = _spacing(spacing, d)
    unit = all(s == 1.0 for s in sp)
    none = NO_FEATURE if unit else np.inf
    out = np.full(f.shape, none, dtype=np.int64 if unit else np.float64)
    grid = np.indices(f.shape[2:])
    for n in range(f.shape[0]):
        for p in np.argwhere(f[n, 0]):
            delta = [grid[a] - p[a] for a in range(d)]
            if unit:
                cand = sum(x * x for x in delta)
            else:
                cand = sum((sp[a] * delta[a].astype(np.float64)) ** 2 for a in range(d))
            out[n, 0] = np.minimum(out[n, 0], cand)
    return out


def signed_distance(L, label=None, spacing=1.0):
    """float64: negative inside the structure, positive outside."""
    m = (L != 0) if label is None else (L == label)
    with np.errstate(invalid="ignore"):
        return np.sqrt(as_float(edt_sq(m, spacing))) - np.sqrt(as_float(edt_sq(~m, spacing)))


# ---- surface distances

def surface_distance(A, B, labels, spacing=1.0, float32_distances=True):
    """dict of float64 (N, K): hausdorff, hd95 (np.percentile's default linear interpolation), assd; nan where either
    surface is empty.  The distances are the float32 square roots the library forms (float32_distances) widened to
    float64, or plain float64 roots."""
    N, K = A.shape[0], len(labels)
    res = {k: np.full((N, K), np.nan) for k in ("hausdorff", "hd95", "assd")}
    for c, k in enumerate(labels):
        sA, sB = surface(A == k), surface(B == k)
        dA, dB = as_float(edt_sq(sA, spacing)), as_float(edt_sq(sB, spacing))
        if float32_distances:
            dA, dB = dA.astype(np.float32), dB.astype(np.float32)
        dA, dB = np.sqrt(dA).astype(np.float64), np.sqrt(dB).astype(np.float64)
        for n in range(N):
            d_ab, d_ba = dB[n][sA[n]], dA[n][sB[n]]
            if d_ab.size == 0 or d_ba.size == 0:
                continue
            res["hausdorff"][n, c] = max(d_ab.max(), d_ba.max())
            res["hd95"][n, c] = max(np.percentile(d_ab, 95), np.percentile(d_ba, 95))
            res["assd"][n, c] = (d_ab.sum() + d_ba.sum()) / (d_ab.size + d_ba.size)
    return res


# ---- inputs

def _smooth(x, passes=3):
    for _ in range(passes):
        for a in range(1, x.ndim):
            x = (np.roll(x, 1, a) + 2 * x + np.roll(x, -1, a)) / 4
    return x


def blobs(rng, N, sp, K):
    """argmax over K channels of smoothed noise: connected structures, labels 0..K-1 (the idea of labels_ref.blobs)."""
    return np.stack([_smooth(rng.standard_normal((K,) + sp)).argmax(0) for _ in range(N)])[:, None].astype(np.int32)


def box(sp, lo, hi, label=1):
    """(1, 1, *sp) int32: `label` on the box lo[a] <= x_a < hi[a] (clipped to the volume), 0 elsewhere."""
    L = np.zeros((1, 1) + tuple(sp), dtype=np.int32)
    L[(0, 0) + tuple(slice(max(l, 0), min(h, n)) for l, h, n in zip(lo, hi, sp))] = label
    return L


def labels(kind, N, sp, seed=0):
    """(N, 1, *sp) int32 with different content per item.  The label of interest is 1 in every kind ("blobs" has 0..3)."""
    sp = tuple(sp)
    rng = np.random.default_rng([seed, KINDS.index(kind), N, *sp])
    if kind == "sparse":   # about 2 % features, at least one per item
        L = (rng.random((N, 1) + sp) < 0.02).astype(np.int32)
        for n in range(N):
            L[n, 0][tuple(rng.integers(0, s) for s in sp)] = 1
        return L
    if kind == "dense":
        return (rng.random((N, 1) + sp) < 0.5).astype(np.int32) * rng.integers(1, 3, (N, 1) + sp).astype(np.int32)
    if kind == "corner":   # one feature: the first voxel of even items, the last voxel of odd ones
        L = np.zeros((N, 1) + sp, dtype=np.int32)
        for n in range(N):
            L[n, 0][tuple((s - 1) * (n & 1) for s in sp)] = 1
        return L
    if kind == "none":
        return np.zeros((N, 1) + sp, dtype=np.int32)
    if kind == "all":
        return np.ones((N, 1) + sp, dtype=np.int32)
    if kind == "blobs":
        return blobs(rng, N, sp, 4)
    if kind == "boxes":   # a box per item, shifted by one voxel from item to item
        return np.concatenate([box(sp, [s // 4 + n for s in sp], [s - s // 4 + n for s in sp]) for n in range(N)])
    raise ValueError(kind)


def concentric_boxes(d=3, n=24, a=(6, 16), grow=3, shift=1):
    """Two boxes in a volume of extent n per axis (one item): A is [a0, a1)^d, B is A grown by `grow` voxels on every
    side and then moved by `shift` along the last axis.  Returns (A, B, hausdorff, assd), the surface distances in
    closed form at unit spacing, per surface_distance's definition (every surface voxel counts once):

    - B's surface is farthest from A at its far corner (grow voxels out along every axis, `shift` more along the last):
      hausdorff^2 = (d - 1) grow^2 + (grow + shift)^2;
    - assd has no short closed form; it is returned as the plain count over the two voxel sets by brute force in exact
      integer arithmetic (independent of the separable recurrence)."""
    sp = (n,) * d
    A = box(sp, (a[0],) * d, (a[1],) * d)
    lo = [a[0] - grow] * d
    hi = [a[1] + grow] * d
    lo[-1] += shift
    hi[-1] += shift
    B = box(sp, lo, hi)
    hausdorff = float(np.sqrt((d - 1) * grow ** 2 + (grow + shift) ** 2))
    sA, sB = surface(A == 1), surface(B == 1)
    pa, pb = np.argwhere(sA[0, 0]), np.argwhere(sB[0, 0])
    d2 = ((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1)
    assd = float((np.sqrt(d2.min(1).astype(np.float64)).sum() + np.sqrt(d2.min(0).astype(np.float64)).sum()) / (len(pa) + len(pb)))
    return A, B, hausdorff, assd
