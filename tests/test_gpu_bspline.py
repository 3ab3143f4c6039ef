"""GPU: bspline_prefilter, interp_bspline and interp_cubic (csrc/bspline.hip) against the numpy reference
tests/bspline_ref.py (which tests/test_bspline_host.py ties to scipy and to known answers), cell by cell for the
scattered d_C, bit for bit from call to call where no atomic is involved, and through torch.autograd.gradcheck.

Parity is the project's criterion: max |got - reference| <= rtol * max |reference|, rtol 1e-5 (float32), 1e-12 (float64).

Prefilter shapes.  (5, 6, 7) and (7, 9) are general; (1, 5, 4), (6, 1, 3), (2, 2, 2), (2, 2) and (1, 9) have one- and
two-voxel extents (an axis of extent 1 is skipped, extent 2 is the shortest recursion and the full start sum), and in
(1, 1, 1) no pass runs at all: a copy;
(3, 4, n), n = 63, 64, 65 put a wave's edge on the contiguous axis and (3, n, 4) on a strided one; the line tile is 256
lines up to n = 40 (float32) / 20 (float64), 128 up to 80 / 40 and 64 beyond, so these shapes take all three.  The staged
passes end at n = 256 in both types (csrc/bspline.hip: kBsStagedMax): 256 on each axis in turn is the largest LDS
tile (128 KiB in float64), 257 and 700 on each axis in turn, in thin volumes, run the long-line path through global
memory.  Rows N * C in {1, 3, 70}: 70 rows of (5, 6, 7) are several workgroups of every pass."""
import functools

import numpy as np
import pytest
import torch

import bspline_ref as ref
import labels_ref
from gpu_util import assert_close, dev, host

pytestmark = pytest.mark.gpu

N = 2
_close = functools.partial(assert_close, floor=0, record=False)   # the bound is RTOL * max|want| exactly: no floor under a zero reference
both_dtypes = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
KINDS = ("random", "shift_out", "half", "huge", "nonfinite")
GENERAL = ((5, 6, 7), (7, 9))
SMALL = ((1, 5, 4), (6, 1, 3), (2, 2, 2), (2, 2), (1, 9))
EDGES = tuple((3, 4, n) for n in (63, 64, 65)) + tuple((3, n, 4) for n in (63, 65)) + ((65, 3, 4), (63, 5), (5, 65))
LONG = tuple(s for n in (256, 257, 700) for s in ((n, 2, 3), (2, n, 3), (2, 3, n), (n, 3), (3, n)))


def _channels(sp):
    return sorted({1, len(sp), 4})


# ---- 1. prefilter and adjoint

def _prefilter_case(sp, rows, dtype):
    import lagomorph_amd as lm

    n, c = {1: (1, 1), 3: (1, 3), 70: (7, 10)}[rows]
    I = ref.image(n, c, sp, dtype, seed=rows)
    Id = dev(I)
    for adjoint in (False, True):
        got = lm.bspline_prefilter(Id, adjoint=adjoint)
        assert got.shape == Id.shape and got.dtype == Id.dtype
        _close(got, ref.prefilter(I, adjoint), dtype, f"prefilter {sp} rows {rows} adjoint {adjoint}")
        assert torch.equal(got, lm.bspline_prefilter(Id, adjoint=adjoint))   # no atomics: the same bits
    assert torch.equal(Id, dev(I))   # the input is left alone


@both_dtypes
@pytest.mark.parametrize("rows", [1, 3, 70])
@pytest.mark.parametrize("sp", GENERAL + SMALL + ((1, 1, 1),), ids=str)
def test_prefilter_general_and_small_shapes(sp, rows, dtype):
    _prefilter_case(sp, rows, dtype)


@both_dtypes
@pytest.mark.parametrize("sp", EDGES, ids=str)
def test_prefilter_around_a_wave(sp, dtype):
    _prefilter_case(sp, 3, dtype)


@both_dtypes
@pytest.mark.parametrize("sp", LONG, ids=str)
def test_prefilter_largest_staged_and_long_lines(sp, dtype):
    _prefilter_case(sp, 3, dtype)


# ---- 2. round trip and adjoint identity

@both_dtypes
@pytest.mark.parametrize("sp", GENERAL + SMALL + ((3, 4, 65), (257, 2, 3)), ids=str)
def test_round_trip_and_adjoint_identity(sp, dtype):
    import lagomorph_amd as lm

    d = len(sp)
    I = ref.image(N, 3, sp, dtype)
    Id = dev(I)
    zero = torch.zeros((N, d) + sp, dtype=Id.dtype, device="cuda")
    _close(lm.interp_cubic(Id, zero), I.astype(np.float64), dtype, f"interp_cubic(I, 0) {sp}")
    _close(lm.interp_cubic(Id[:1].contiguous(), zero), np.broadcast_to(I[:1], I.shape).astype(np.float64), dtype, f"broadcast {sp}")
    if dtype == np.float64:
        g = ref.image(N, 3, sp, dtype, seed=1)
        gd = dev(g)
        lhs = float((lm.bspline_prefilter(Id) * gd).sum())
        rhs = float((Id * lm.bspline_prefilter(gd, adjoint=True)).sum())
        scale = float((lm.bspline_prefilter(Id).abs() * gd.abs()).sum())
        assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs, scale)


# ---- 3. forward, 4. d_u

@both_dtypes
@pytest.mark.parametrize("sp", GENERAL + SMALL + ((3, 4, 65),), ids=str)
def test_forward_and_position_gradient(sp, dtype):
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    d = len(sp)
    for kind in KINDS:
        u = labels_ref.displacement(kind, N, sp, dtype)
        tp = ref.taps(u, 1.0)
        nan = np.zeros((N,) + sp, dtype=bool)
        for x in tp:
            nan |= x[4]
        if kind == "random":   # some samples leave the grid, some stay
            out = np.zeros((N,) + sp, dtype=bool)
            for x in tp:
                out |= x[3]
            assert out.any() and (min(sp) < 3 or not out.all()), sp
        assert nan.any() == (kind == "nonfinite")
        ud = dev(u)
        for K in _channels(sp):
            Cf = ref.image(N, K, sp, dtype, seed=K)
            go = ref.image(N, K, sp, dtype, seed=100 + K)
            god = dev(go)
            for bc in (False, True):
                Ch = Cf[:1] if bc else Cf
                Cd = dev(Ch)
                for dt in ((1.0, -0.7) if kind == "random" and not bc else (1.0,)):
                    if dt != 1.0:
                        assert not np.isnan(u).any()
                    what = f"{sp} {kind} K {K} bc {bc} dt {dt}"
                    want = ref.interp(Ch.astype(np.float64), u, dt)
                    ug = ud.clone().requires_grad_(True)
                    got = lm.interp_bspline(Cd, ug, dt)
                    assert got.shape == (N, K) + sp and got.dtype == Cd.dtype
                    gh = host(got)
                    if dt == 1.0:   # NaN exactly where a coordinate is NaN
                        assert np.array_equal(np.isnan(gh), np.broadcast_to(nan[:, None], gh.shape)), what
                    ok = ~np.isnan(want)
                    _close(torch.from_numpy(np.where(ok, gh, 0)), np.where(ok, want, 0), dtype, "values " + what)
                    got.backward(god)
                    du_want = ref.grad_u(go, Ch.astype(np.float64), u, dt)
                    du = host(ug.grad)
                    assert np.array_equal(np.isnan(du), np.isnan(du_want)), what
                    okd = ~np.isnan(du_want)
                    _close(torch.from_numpy(np.where(okd, du, 0)), np.where(okd, du_want, 0), dtype, "d_u " + what)
                    tpd = ref.taps(u, dt)
                    for a in range(d):   # exactly 0 on clamped axes
                        cl = tpd[a][3] & okd[:, a]
                        assert (du[:, a][cl] == 0).all(), what
                    # 6. the forward and d_u repeat bit for bit
                    again = lm.interp_bspline(Cd, ud, dt)
                    d_C, d_u = ext.interp_bspline_backward(god, Cd, ud, dt, False, True)
                    assert d_C is None
                    for a, b in ((got, again), (ug.grad, d_u)):
                        na, nb = torch.isnan(a), torch.isnan(b)
                        assert torch.equal(na, nb) and torch.equal(a[~na], b[~nb]), what


# ---- 5. d_C cell by cell

@both_dtypes
@pytest.mark.parametrize("sp", GENERAL + ((1, 5, 4), (2, 2, 2), (1, 9), (3, 4, 65)), ids=str)
def test_coefficient_gradient_cell_by_cell(sp, dtype):
    """Every cell of d_C within bound_i = (n_i + K) u / (1 - (n_i + K) u) A_i + n_i tiny of the wide sum (float64 sums
    for float32 results, long double for float64), n_i the number of contributions to the cell, A_i the sum of their
    magnitudes.

    K = 9 d, from the expressions of csrc/bspline_weights.hpp and the kernel's product, not from any output.  The
    yardstick's contribution is (exact cubic weights at the t the library forms) x g.  On the library's path: s = 1 - t
    is one rounding; w_0 = ((s s) s) sixth: 3 u from s, two products, the rounded constant and its product, 7 u;
    w_3 likewise without s, 4 u; p(r) = ((3 - 3r) r + 3) r + 1 adds terms of one sign only: 3r (u), 3 - 3r (absolute
    error <= 3 u + u b), b r, + 3 (>= 3, relative 2.5 u), times r (3.5 u), + 1 (4.5 u), times sixth (6.5 u); w_1 = p(s)
    takes one more u through s times the condition s p'(s) / p(s) < 1: 7.5 u.  So <= 8 u per axis, 8 d in all
    (tests/test_bspline_host.py measures the expressions: under 6 u); then d - 1 weight products and the product with
    g: d; n_i - 1 rounded additions in whatever order the atomics arrive (the first lands on the zeroed cell exactly);
    one for the yardstick's own rounding.  8 d + d + n_i - 1 + 1 = n_i + 9 d factors (1 + delta), |delta| <= u, and
    Higham's Lemma 3.1 gives the bound; n_i tiny covers subnormal sums flushed by the atomic unit.

    Cells that receive nothing hold exactly 0; with a broadcast C the sums run over the items; a voxel with a NaN
    coordinate adds nothing.  d_I of interp_cubic is the reference's P^T d_C."""
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    d = len(sp)
    wide_kw = dict(wfun=ref.weights_wide, add_dtype=np.longdouble) if dtype == np.float64 else {}
    worst = 0.0
    for kind in KINDS:
        u = labels_ref.displacement(kind, N, sp, dtype)
        ud = dev(u)
        for K in _channels(sp):
            go = ref.image(N, K, sp, dtype, seed=7)
            god = dev(go)
            for bc in (False, True):
                what = f"{sp} {kind} K {K} bc {bc}"
                shape = (1 if bc else N, K) + sp
                Cd = dev(ref.image(shape[0], K, sp, dtype, seed=9))
                wide = ref.grad_C_wide(go, shape, u, **wide_kw)
                d_C, d_u = ext.interp_bspline_backward(god, Cd, ud, 1.0, True, False)
                assert d_u is None and d_C.shape == shape
                ratio, empty_ok = ref.cell_ratio(host(d_C), wide, dtype, d)
                assert empty_ok, what
                assert ratio <= 1.0, f"{what}: worst cell at {ratio:.3f} of its bound"
                worst = max(worst, ratio)
                if kind in ("random", "nonfinite") and K == 1:   # d_I of interp_cubic = P^T d_C
                    Ig = Cd.clone().requires_grad_(True)
                    lm.interp_cubic(Ig, ud).backward(god)
                    want = ref.prefilter(wide[0].astype(np.float64), adjoint=True)
                    _close(Ig.grad, want, dtype, "d_I " + what)
    print(f"{sp} {np.dtype(dtype).name}: worst d_C cell at {worst:.3f} of its bound")


# ---- 7. gradcheck

@pytest.mark.parametrize("sp", [(4, 5, 6), (5, 6)], ids=str)
def test_gradcheck(sp):
    import lagomorph_amd as lm

    d = len(sp)
    rng = np.random.default_rng([5, *sp])
    # positions at least 0.1 voxel inside the grid: i + u in [0.1, n - 1.1]
    idx = np.indices(sp).astype(np.float64)
    target = np.stack([rng.uniform(0.1, n - 1.1, (N,) + sp) for n in sp], 1)
    u = dev(target - idx[None]).requires_grad_(True)
    I = dev(ref.image(N, 2, sp, np.float64)).requires_grad_(True)
    I1 = dev(ref.image(1, 2, sp, np.float64)).requires_grad_(True)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-6, nondet_tol=1e-9)
    assert torch.autograd.gradcheck(lambda x: lm.bspline_prefilter(x), (I,), **kw)
    assert torch.autograd.gradcheck(lambda x: lm.bspline_prefilter(x, adjoint=True), (I,), **kw)
    assert torch.autograd.gradcheck(lambda c, v: lm.interp_bspline(c, v), (I, u), **kw)
    assert torch.autograd.gradcheck(lambda c, v: lm.interp_bspline(c, v, -0.5), (I1, (-2.0 * u).detach().requires_grad_(True)), **kw)
    assert torch.autograd.gradcheck(lambda c, v: lm.interp_cubic(c, v), (I, u), **kw)
    # a gradient that is not needed is not computed
    out = lm.interp_bspline(I.detach(), u)
    (g,) = torch.autograd.grad(out.sum(), (u,))
    assert g.shape == u.shape
