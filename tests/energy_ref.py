"""numpy reference of diffusion_energy, bending_energy and energy_operator (the definition of include/lagomorph_hip.h:
lago_field_energy), the restatement of lagomorph_amd/csrc/energy_stencil.hpp in the kernels' own order and precision,
and the rounding bound the GPU test holds the float32 operator to.

The reference builds A u = sum_t w_t D_t^T (D_t u) from the difference operators themselves: D_t u on the rows where it
exists and zero elsewhere, then the transpose as slice additions -- nothing of the kernels' clamped-neighbour form.
tests/test_energy_host.py ties it to an independent torch restatement and to known answers."""
import itertools

import numpy as np

KINDS = ("diffusion", "bending")
K = {"diffusion": 8, "bending": 13}   # roundings between u and (A u)(x): energy_stencil.hpp
U32 = 2.0 ** -24

# the kernels' voxel tile (csrc/energy.hip: EnergyTile): 3D (x, y, z), 2D (y, z).  A change of tile changes TILE_SHAPES
TILE3, TILE2 = (8, 8, 64), (64, 64)
HOST_SHAPES = ((5, 6, 7), (2, 2, 2), (3, 3, 3), (3, 4, 1), (5, 1, 4), (9, 5, 70), (7, 9), (2, 2), (5, 1), (24, 20, 36))


def _tile_shapes(tile, small):
    """Per axis: one tile + 1, one tile + 2 and two tiles + 1, the other axes small."""
    out = []
    for a, t in enumerate(tile):
        for n in (t + 1, t + 2, 2 * t + 1):
            s = list(small)
            s[a] = n
            out.append(tuple(s))
    return tuple(out)


TILE_SHAPES = _tile_shapes(TILE3, (5, 6, 7)) + _tile_shapes(TILE2, (7, 9)) + ((17, 18, 131),)   # + two tiles + 1 on every axis at once
THIN_SHAPES = ((2, 70), (9, 1, 66), (2, 11, 5))   # an axis of extent 1 or 2, in 2D and in 3D
GPU_SHAPES = HOST_SHAPES + TILE_SHAPES + THIN_SHAPES
SPACINGS = (1.0, (1.0, 1.5, 0.7))


def spacing_tuple(spacing, d):
    sp = tuple(float(s) for s in spacing) if hasattr(spacing, "__len__") else (float(spacing),) * 3
    return sp[:d]


def field(N, C, shape, dtype, seed=0, affine=False):
    """Standard normal noise, a different field per item; affine=True: a field affine in the voxel index with
    coefficients of order 1 plus 1e-3 x noise (A u is then small against u)."""
    rng = np.random.default_rng(seed + 1000 * len(shape) + sum(shape))
    u = rng.standard_normal((N, C) + tuple(shape))
    if affine:
        x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
        coef = rng.uniform(-1.0, 1.0, (N, C, len(shape) + 1))
        lin = coef[..., -1].reshape((N, C) + (1,) * len(shape)) + sum(
            coef[..., a].reshape((N, C) + (1,) * len(shape)) * x[a] for a in range(len(shape)))
        u = lin + 1e-3 * u
    return np.ascontiguousarray(u.astype(dtype))


def _sl(u, a, s):
    i = [slice(None)] * u.ndim
    i[2 + a] = s
    return tuple(i)


def _fwd(u, a, h, absolute=False):
    """d_a u: rows x_a + 1 < n_a."""
    r = np.zeros_like(u)
    if u.shape[2 + a] > 1:
        hi, lo = u[_sl(u, a, slice(1, None))], u[_sl(u, a, slice(0, -1))]
        r[_sl(u, a, slice(0, -1))] = (hi + lo if absolute else hi - lo) / h
    return r


def _fwd_t(r, a, h, absolute=False):
    g = np.zeros_like(r)
    if r.shape[2 + a] > 1:
        c = r[_sl(r, a, slice(0, -1))] / h
        g[_sl(r, a, slice(1, None))] += c
        if absolute:
            g[_sl(r, a, slice(0, -1))] += c
        else:
            g[_sl(r, a, slice(0, -1))] -= c
    return g


def _sec(u, a, h, absolute=False):
    """d_aa u: rows 1 <= x_a <= n_a - 2."""
    r = np.zeros_like(u)
    if u.shape[2 + a] > 2:
        p, c, m = u[_sl(u, a, slice(2, None))], u[_sl(u, a, slice(1, -1))], u[_sl(u, a, slice(0, -2))]
        r[_sl(u, a, slice(1, -1))] = (p + 2 * c + m if absolute else p - 2 * c + m) / h ** 2
    return r


def _sec_t(r, a, h, absolute=False):
    g = np.zeros_like(r)
    if r.shape[2 + a] > 2:
        c = r[_sl(r, a, slice(1, -1))] / h ** 2
        g[_sl(r, a, slice(2, None))] += c
        g[_sl(r, a, slice(0, -2))] += c
        if absolute:
            g[_sl(r, a, slice(1, -1))] += 2 * c
        else:
            g[_sl(r, a, slice(1, -1))] -= 2 * c
    return g


def energy(u, kind, spacing=1.0):
    """E (N,) in float64, from the definition."""
    assert kind in KINDS
    u = np.asarray(u, dtype=np.float64)
    d = u.ndim - 2
    h = spacing_tuple(spacing, d)
    V = int(np.prod(u.shape[2:]))
    ax = tuple(range(1, u.ndim))
    if kind == "diffusion":
        e = sum((_fwd(u, a, h[a]) ** 2).sum(ax) for a in range(d))
    else:
        e = sum((_sec(u, a, h[a]) ** 2).sum(ax) for a in range(d))
        for a, b in itertools.combinations(range(d), 2):
            e = e + 2 * (_fwd(_fwd(u, a, h[a]), b, h[b]) ** 2).sum(ax)
    return e / V


def operator(u, kind, spacing=1.0, absolute=False):
    """A u (N, C, *sp) in float64 = sum_t w_t D_t^T (D_t u); absolute=True: every coefficient of every D_t and D_t^T
    by its absolute value, applied to |u| (abs_operator)."""
    assert kind in KINDS
    u = np.asarray(u, dtype=np.float64)
    if absolute:
        u = np.abs(u)
    d = u.ndim - 2
    h = spacing_tuple(spacing, d)
    if kind == "diffusion":
        return sum(_fwd_t(_fwd(u, a, h[a], absolute), a, h[a], absolute) for a in range(d))
    g = sum(_sec_t(_sec(u, a, h[a], absolute), a, h[a], absolute) for a in range(d))
    for a, b in itertools.combinations(range(d), 2):
        g = g + 2 * _fwd_t(_fwd_t(_fwd(_fwd(u, a, h[a], absolute), b, h[b], absolute), b, h[b], absolute), a, h[a], absolute)
    return g


def abs_operator(u, kind, spacing=1.0):
    """sum |A| |u| per voxel: the scale of the operator's rounding error."""
    return operator(u, kind, spacing, absolute=True)


def operator_bound(u, kind, spacing=1.0, scale=None):
    """K 2^-24 |scale_n| abs_operator(u)(x): what a float32 kernel value may differ from the exact one by."""
    b = K[kind] * U32 * abs_operator(u, kind, spacing)
    if scale is not None:
        b = b * np.abs(np.asarray(scale, dtype=np.float64)).reshape((-1,) + (1,) * (b.ndim - 1))
    return b


def worst_ratio(err, bound):
    """max err / bound; where the bound is 0 the error has to be 0 (inf otherwise)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if ((bound == 0) & (err != 0)).any():
        return np.inf
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


# ---- energy_stencil.hpp restated: the same operations in the same order in u's own precision

class _Native:
    def __init__(self, u, kind, spacing):
        self.R = u.dtype.type
        self.d = d = u.ndim - 2
        self.shape = u.shape[2:]
        self.pad = np.pad(u, ((0, 0), (0, 0)) + ((2, 2),) * d, mode="edge")   # every coordinate clamped to its axis
        h2 = [h * h for h in spacing_tuple(spacing, d)]   # Python floats: the header's doubles
        self.wa = [self.R(1.0 / (v * v) if kind == "bending" else 1.0 / v) for v in h2]
        self.wab = {(a, b): self.R(2.0 / (h2[a] * h2[b])) for a, b in itertools.combinations(range(d), 2)}

    def at(self, off):
        i = [slice(None), slice(None)] + [slice(2 + o, 2 + o + n) for o, n in zip(off, self.shape)]
        return self.pad[tuple(i)]

    def at1(self, a, i):
        off = [0] * self.d
        off[a] = i
        return self.at(off)

    def at2(self, a, b, i, j):
        off = [0] * self.d
        off[a], off[b] = i, j
        return self.at(off)

    def mask(self, a):
        n = self.shape[a]
        x = np.arange(n)
        sh = [1] * (self.d + 2)
        sh[2 + a] = n
        return [((x >= lo) & (x <= hi)).astype(self.R).reshape(sh) for lo, hi in ((2, n - 1), (1, n - 2), (0, n - 3))]

    def total(self, terms):
        acc = None
        for w, t in terms:
            acc = w * t if acc is None else acc + w * t
        return acc


def density_native(u, kind, spacing=1.0):
    """The per-voxel energy density (N, C, *sp) as energy_diffusion_density / energy_bending_density compute it."""
    s = _Native(u, kind, spacing)
    u0 = s.at1(0, 0)
    terms = []
    if kind == "diffusion":
        for a in range(s.d):
            f = s.at1(a, 1) - u0
            terms.append((s.wa[a], f * f))
    else:
        for a in range(s.d):
            v = s.mask(a)[1] * ((s.at1(a, 1) - u0) - (u0 - s.at1(a, -1)))
            terms.append((s.wa[a], v * v))
        for a, b in itertools.combinations(range(s.d), 2):
            m = (s.at2(a, b, 1, 1) - s.at2(a, b, 1, 0)) - (s.at2(a, b, 0, 1) - u0)
            terms.append((s.wab[a, b], m * m))
    out = s.total(terms)
    assert out.dtype == u.dtype
    return out


def operator_native(u, kind, spacing=1.0):
    """A u (N, C, *sp) as energy_diffusion_apply / energy_bending_apply compute it (scale 1)."""
    s = _Native(u, kind, spacing)
    u0 = s.at1(0, 0)
    terms, L = [], {}
    for a in range(s.d):
        um2, um1, up1, up2 = s.at1(a, -2), s.at1(a, -1), s.at1(a, 1), s.at1(a, 2)
        fm2, fm1, f0, f1 = um1 - um2, u0 - um1, up1 - u0, up2 - up1
        L[a] = fm1 - f0
        if kind == "diffusion":
            terms.append((s.wa[a], L[a]))
        else:
            qm, qc, qp = s.mask(a)
            sm, s0, sp = qm * (fm1 - fm2), qc * (f0 - fm1), qp * (f1 - f0)
            terms.append((s.wa[a], (sm - s0) + (sp - s0)))
    if kind == "bending":
        for a, b in itertools.combinations(range(s.d), 2):
            cm, cp = s.at2(a, b, 0, -1), s.at2(a, b, 0, 1)
            gm = (cm - s.at2(a, b, -1, -1)) - (s.at2(a, b, 1, -1) - cm)
            gp = (cp - s.at2(a, b, -1, 1)) - (s.at2(a, b, 1, 1) - cp)
            terms.append((s.wab[a, b], (L[a] - gm) + (L[a] - gp)))
    out = s.total(terms)
    assert out.dtype == u.dtype
    return out
