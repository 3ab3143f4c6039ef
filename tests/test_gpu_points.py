"""GPU: interp_points, deform_points and their gradients (csrc/points.hip) against `interp` bit for bit, against the
numpy reference tests/points_ref.py (which tests/test_points_host.py ties to grid_sample and to known answers), cell by
cell for the scattered d_F (tests/scatter_bound.py), and through torch.autograd.gradcheck.

Shapes: (5, 6, 7), (7, 9) and (8, 16, 32) are general; (1, 5, 4), (6, 1, 3) and (1, 9) have one-voxel extents and a thin
z (nz == 1: Lerp3's single loads); in (2, 2, 2) a corner pair is the whole row.  Point counts: 1 is a single lane, 63, 64
and 65 sit around a wave, 257 crosses a workgroup, 1000 gives several blocks with a tail."""
import functools

import numpy as np
import pytest
import torch

import labels_ref
import points_ref as ref
import scatter_bound
from gpu_util import assert_close, dev

pytestmark = pytest.mark.gpu

N = 2
SHAPES = ref.SHAPES
PS = ref.POINT_COUNTS
_close = functools.partial(assert_close, floor=0, record=False)   # the bound is RTOL * max|want| exactly: no floor under a zero reference
both_dtypes = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
all_shapes = pytest.mark.parametrize("sp", SHAPES, ids=str)


def _channels(sp):
    return sorted({1, len(sp), 4})


def _same_bits(a, b):
    """torch.equal, with NaNs equal to NaNs (positions that are not finite)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


# ---- 1. the same bits as interp

@both_dtypes
@all_shapes
def test_same_bits_as_interp(sp, dtype):
    import lagomorph_amd as lm

    d = len(sp)
    ident = lm.identity((N, d) + sp, dtype=dtype)
    rng = np.random.default_rng([11, *sp])
    fields = [(k, labels_ref.displacement(k, N, sp, dtype)) for k in ("random", "shift_out", "half", "huge", "nonfinite")]
    fields.append(("normal", (0.6 * max(sp) * rng.standard_normal((N, d) + sp)).astype(dtype)))
    for kind, u in fields:
        p = (ident + u).reshape(N, d, -1)          # ONE rounding in the working dtype: interp's dt = 1 position
        assert p.dtype == np.dtype(dtype)
        if kind in ("random", "normal"):
            out = ref.outside(p, sp)
            assert out.mean() > 0.02 and (min(sp) < 5 or not out.all()), kind   # some samples leave the grid, some stay
        ud, pd = dev(u), dev(p)
        for C in _channels(sp):
            I = ref.field(N, C, sp, dtype)
            for bc in (False, True):
                Id = dev(I[:1] if bc else I)
                got = lm.interp_points(Id, pd)
                want = lm.interp(Id, ud).reshape(N, C, -1)
                assert got.shape == (N, C, int(np.prod(sp))) and got.dtype == Id.dtype
                if kind == "nonfinite":
                    assert _same_bits(got, want), (kind, C, bc)
                    assert torch.isnan(got).any() and not torch.isnan(got).all()
                else:
                    assert torch.equal(got, want), (kind, C, bc)


# ---- 2. scattered positions against the reference

@both_dtypes
@all_shapes
def test_scattered_positions_against_the_reference(sp, dtype):
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    d = len(sp)
    for P in PS:
        x, first = ref.scattered(N, sp, P, dtype)
        assert ref.outside(x[:, :, first:], sp).mean() >= 0.25, P     # of the wide half, a quarter or more is outside
        assert not ref.outside(x[:, :, :first], sp).any()
        xd = dev(x)
        for C in _channels(sp):
            F = ref.field(N, C, sp, dtype, seed=P)
            g = ref.upstream(N, C, P, dtype)
            gd = dev(g)
            for bc in (False, True):
                Fh = F[:1] if bc else F
                val, grad = ref.sample(Fh, x)
                Fd, xg = dev(Fh), xd.clone().requires_grad_(True)
                out = lm.interp_points(Fd, xg)
                assert out.shape == (N, C, P)
                _close(out, val, dtype, f"values {sp} P {P} C {C} bc {bc}")
                out.backward(gd)
                _close(xg.grad, (g[:, :, None, :].astype(np.float64) * grad).sum(1), dtype, f"d_x {sp} P {P} C {C} bc {bc}")
                d_F, d_x = ext.interp_points_backward(gd, Fd, xd, False, True)     # a second call: identical d_x
                assert d_F is None and torch.equal(d_x, xg.grad)


@both_dtypes
@all_shapes
def test_far_and_non_finite_positions(sp, dtype):
    import lagomorph_amd as lm

    d, C, P = len(sp), 2, 65
    F = ref.field(N, C, sp, dtype)
    base, _ = ref.scattered(N, sp, P, dtype, seed=3)
    g = ref.upstream(N, C, P, dtype)
    for a, n in enumerate(sp):
        for far, edge in ((-1e6 - 0.25, 0.0), (1e6 + 0.25, n - 1.0)):
            x, xe = base.copy(), base.copy()
            x[:, a] = far
            xe[:, a] = edge
            assert x.dtype == np.dtype(dtype) and np.all(x[:, a].astype(np.float64) == far)
            xg = dev(x).requires_grad_(True)
            out = lm.interp_points(dev(F), xg)
            val, grad = ref.sample(F, x)
            _close(out, val, dtype, f"far values {sp} axis {a}")
            _close(out, ref.sample(F, xe)[0], dtype, f"border values {sp} axis {a}")     # the border value
            out.backward(dev(g))
            assert torch.all(xg.grad[:, a] == 0), (a, far)                             # no gradient along that axis
            _close(xg.grad, (g[:, :, None, :].astype(np.float64) * grad).sum(1), dtype, f"far d_x {sp} axis {a}")
    # coordinates that are not finite: NaN for that point, every other point untouched
    x = base.copy()
    bad = {0: np.nan, 7: np.inf, 64: -np.inf}
    for p, v in bad.items():
        x[:, p % d, p] = v
    out = lm.interp_points(dev(F), dev(x)).cpu().numpy()
    want = lm.interp_points(dev(F), dev(base)).cpu().numpy()
    for p in range(P):
        if p in bad:
            assert np.all(np.isnan(out[:, :, p])), p
        else:
            assert np.array_equal(out[:, :, p], want[:, :, p]), p


# ---- 3. d_F cell by cell

def _d_F_cases(sp):
    d = len(sp)
    yield "scattered", 1000, 4, False
    yield "scattered", 1000, 4, True
    yield "scattered", 257, d, False
    yield "crowd", 257, 1, False
    yield "crowd", 257, d, True
    for P in (1, 63, 64, 65):
        yield "scattered", P, 1, P == 64


@both_dtypes
@all_shapes
def test_d_F_cell_by_cell(sp, dtype):
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    worst = 0.0
    for kind, P, C, bc in _d_F_cases(sp):
        x = ref.crowd(N, sp, P, dtype) if kind == "crowd" else ref.scattered(N, sp, P, dtype, seed=1)[0]
        NF = 1 if bc else N
        F = ref.field(NF, C, sp, dtype)
        g = ref.upstream(N, C, P, dtype, seed=1)
        wide = ref.scatter_wide(g, x, sp, NF)
        if kind == "crowd":      # many atomics on few cells: every contribution lands on the 2^d corners of one cell
            assert (wide[2][0, 0] > 0).sum() <= 2 ** len(sp) and wide[2].max() >= P
        Fd, xd, gd = dev(F).requires_grad_(True), dev(x).requires_grad_(True), dev(g)
        lm.interp_points(Fd, xd).backward(gd)
        assert Fd.grad.shape == Fd.shape
        what = f"d_F {sp} {np.dtype(dtype).name} {kind} P {P} C {C} bc {bc}"
        worst = max(worst, scatter_bound.assert_cells(Fd.grad.cpu().numpy(), wide, dtype, what))
        assert torch.all(Fd.grad[dev(wide[2] == 0)] == 0)          # cells that receive nothing: exactly 0
        # need_F without need_x and the reverse: the gradient that was not requested is None
        F2, x2 = dev(F).requires_grad_(True), dev(x)
        lm.interp_points(F2, x2).backward(gd)
        assert x2.grad is None
        worst = max(worst, scatter_bound.assert_cells(F2.grad.cpu().numpy(), wide, dtype, what + " (need_F only)"))
        F3, x3 = dev(F), dev(x).requires_grad_(True)
        lm.interp_points(F3, x3).backward(gd)
        assert F3.grad is None and torch.equal(x3.grad, xd.grad)
        d_F, d_x = ext.interp_points_backward(gd, F3, x2, True, False)
        assert d_x is None and d_F.shape == F3.shape
        d_F, d_x = ext.interp_points_backward(gd, F3, x2, False, False)
        assert d_F is None and d_x is None
    print(f"d_F {sp} {np.dtype(dtype).name}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


# ---- 4. gradcheck

@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9)], ids=str)
@pytest.mark.parametrize("bc", [False, True], ids=["per_item", "broadcast"])
def test_gradcheck(sp, bc):
    import lagomorph_amd as lm

    d, P = len(sp), 9
    x = dev(ref.interior(N, sp, P, np.float64)).requires_grad_(True)       # fractions in [0.1, 0.9]: eps crosses no face
    F = dev(ref.field(1 if bc else N, 3, sp, np.float64)).requires_grad_(True)
    u = dev(0.5 * ref.field(1 if bc else N, d, sp, np.float64, seed=2)).requires_grad_(True)
    # (nondet_tol: d_F is a sum of float atomics, its last bits differ between the two backward runs gradcheck compares)
    kw = dict(eps=1e-5, atol=1e-8, rtol=1e-6, nondet_tol=1e-10)
    assert torch.autograd.gradcheck(lm.interp_points, (F, x), **kw)
    assert torch.autograd.gradcheck(lambda xx, uu: lm.deform_points(xx, uu, 0.7), (x, u), **kw)
    assert torch.autograd.gradcheck(lambda xx, yy: lm.landmark_distance(lm.deform_points(xx, u.detach()), yy, (1.0, 0.5, 2.0)[:d],
                                                                         squared=True), (x, x.detach() + 0.3), **kw)


# ---- 5. deform_points

@both_dtypes
@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9), (8, 16, 32), (1, 5, 4)], ids=str)
def test_deform_points(sp, dtype):
    import lagomorph_amd as lm

    d, P = len(sp), 257
    u = labels_ref.displacement("random", N, sp, dtype)
    x, _ = ref.scattered(N, sp, P, dtype, seed=2)
    ud, xd = dev(u), dev(x)
    for bc in (False, True):
        uu = ud[:1].contiguous() if bc else ud
        for dt in (1.0, -0.5):
            got = lm.deform_points(xd, uu, dt)
            assert got.shape == (N, d, P) and torch.equal(got, xd + dt * lm.interp_points(uu, xd)), (bc, dt)
        assert torch.equal(lm.deform_points(xd, uu), lm.deform_points(xd, uu, 1.0))
    # the identity grid as the point set: identity + u exactly, which is also identity + compose(0 u, u)
    ident = dev(lm.identity((N, d) + sp, dtype=dtype))
    got = lm.deform_points(ident.reshape(N, d, -1), ud).reshape((N, d) + sp)
    assert torch.equal(got, ident + ud)
    assert torch.equal(got, ident + lm.compose(0 * ud, ud))
    # target registration error of an integer translation: exactly 0.  The landmarks sit on eighths of a voxel, so that
    # every product and sum of the interpolation of the constant field is exact, and they and their images stay inside
    shift = (1.0, -2.0, 2.0)[:d] if min(sp) > 2 else (0.0, -2.0, 1.0)[:d]
    rng = np.random.default_rng([5, *sp])
    lms = np.empty((N, d, 40))
    for a, n in enumerate(sp):
        lo, hi = max(0.0, -shift[a]), min(n - 1.0, n - 1.0 - shift[a])
        lms[:, a] = lo + rng.integers(0, int(8 * (hi - lo)) + 1, (N, 40)) / 8.0
    lmd = dev(lms.astype(dtype))
    t = torch.tensor(shift, dtype=lmd.dtype, device="cuda").view(1, d, 1)
    const = (t.view((1, d) + (1,) * d) * torch.ones((1, d) + sp, dtype=lmd.dtype, device="cuda")).contiguous()
    tre = lm.landmark_distance(lm.deform_points(lmd, const), lmd + t, spacing=(0.8, 1.0, 1.5)[:d])
    assert tre.shape == (N, 40) and torch.all(tre == 0)
    moved = lm.landmark_distance(lm.deform_points(lmd, const), lmd)          # ... and against where they were: |shift|
    assert (moved - float(np.sqrt(sum(s * s for s in shift)))).abs().max() <= 1e-6


# ---- 6. argument errors on GPU tensors

def test_argument_errors_on_gpu_tensors():
    import lagomorph_amd as lm

    F = torch.zeros((2, 3, 4, 5, 6), device="cuda")
    x = torch.zeros((2, 3, 10), device="cuda")
    with pytest.raises(RuntimeError, match="x must be contiguous"):
        lm.interp_points(F, torch.zeros((2, 10, 3), device="cuda").transpose(1, 2))
    with pytest.raises(RuntimeError, match="point set of shape"):
        lm.interp_points(F, x[:, :2].contiguous())
    with pytest.raises(RuntimeError, match="batch sizes"):
        lm.interp_points(F, torch.zeros((3, 3, 10), device="cuda"))
    with pytest.raises(RuntimeError, match="float32 and float64"):
        lm.interp_points(F.half(), x.half())
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        lm.interp_points(F, x.double())
    with pytest.raises(RuntimeError, match="device mismatch"):
        lm.interp_points(F, x.cpu())
    with pytest.raises(RuntimeError, match="displacement field"):
        lm.deform_points(x, F[:, :2].contiguous())
    # and what is accepted: no points, no channels
    assert lm.interp_points(F, x[:, :, :0].contiguous()).shape == (2, 3, 0)
    assert lm.interp_points(F[:, :0].contiguous(), x).shape == (2, 0, 10)
    Fg = F.clone().requires_grad_(True)
    lm.interp_points(Fg, x[:, :, :0].contiguous()).sum().backward()
    assert torch.equal(Fg.grad, torch.zeros_like(F))
