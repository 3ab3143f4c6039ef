"""CPU: the specification of bspline_prefilter, interp_bspline and interp_cubic before any GPU run.

- tests/bspline_ref.py, the numpy reference: tied to scipy.ndimage (spline_filter and map_coordinates, order 3, mode
  'mirror') at 1e-12, and to facts that need no scipy -- the spline through the coefficients reproduces the samples,
  constants stay constants, the weights sum to 1 and the derivative weights to 0, the derivative weights are the
  derivative of the weights, <P f, g> = <f, P^T g>, and B^T = D B D^-1 (the form the kernel's adjoint uses);
- lagomorph_amd/csrc/bspline_weights.hpp, the header the kernels call: tests/native/bspline_emul.cpp runs a sweep of
  positions through it with a plain host compiler, and cells, folded taps, flags, weights and derivative weights equal
  the reference bit for bit; the same program once more under -fsanitize=address,undefined;
- the rounding count behind the d_C cell bound (bspline_ref.cell_bound): each weight within 8 u of the exact cubic, and
  a float32 numpy run of the kernel's own expressions and products inside the bound on the inputs of the GPU test;
- the public surface: names, C symbols, the argument errors (raised on CPU tensors, before any device call)."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import bspline_ref as ref
import labels_ref
import native_build

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((2, 3, 5), (5, 4, 7), (9, 11), (1, 6, 3), (2, 2))
KINDS = ("random", "shift_out", "half", "huge", "nonfinite")


# ---- the reference against scipy

@pytest.mark.parametrize("sp", SHAPES, ids=str)
def test_reference_prefilter_is_scipys_spline_filter(sp):
    ndi = pytest.importorskip("scipy.ndimage")
    I = ref.image(2, 2, sp, np.float64)
    got = ref.prefilter(I)
    for n in range(2):
        for k in range(2):
            want = ndi.spline_filter(I[n, k], order=3, mode="mirror")
            assert np.abs(got[n, k] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("sp", SHAPES, ids=str)
def test_reference_sampling_is_scipys_map_coordinates_at_the_clamped_positions(sp):
    ndi = pytest.importorskip("scipy.ndimage")
    d = len(sp)
    C = ref.image(2, 2, sp, np.float64, seed=5)
    idx = np.indices(sp).astype(np.float64)
    for kind in KINDS:
        u = labels_ref.displacement(kind, 2, sp, np.float64)
        got = ref.interp(C, u)
        for n in range(2):
            nan = np.isnan(u[n]).any(0)
            with np.errstate(invalid="ignore"):
                pos = [np.where(nan, 0.0, np.clip(idx[a] + u[n, a], 0, sp[a] - 1)) for a in range(d)]
            for k in range(2):
                want = ndi.map_coordinates(C[n, k], pos, order=3, mode="mirror", prefilter=False)
                assert np.array_equal(np.isnan(got[n, k]), nan), kind
                assert np.abs(got[n, k] - want)[~nan].max() <= 1e-12 * np.abs(want).max(), kind


# ---- the reference against facts that need no scipy

@pytest.mark.parametrize("sp", SHAPES + ((1, 9), (6, 1, 3), (2, 2, 2)), ids=str)
def test_reference_reproduces_the_samples_and_constants(sp):
    d = len(sp)
    I = ref.image(2, 3, sp, np.float64)
    zero = np.zeros((2, d) + sp)
    assert np.abs(ref.interp_cubic(I, zero) - I).max() <= 1e-13 * np.abs(I).max()
    const = np.full((2, 1) + sp, 2.5)
    assert np.abs(ref.prefilter(const) - 2.5).max() <= 1e-14
    u = labels_ref.displacement("random", 2, sp, np.float64)
    assert np.abs(ref.interp_cubic(const, u) - 2.5).max() <= 1e-14
    # B c = f, by the matrix the docstring states
    c = ref.prefilter(I)
    for a, n in enumerate(sp):
        c = np.moveaxis(np.tensordot(ref.matrix(n), np.moveaxis(c, 2 + a, 0), 1), 0, 2 + a)
    assert np.abs(c - I).max() <= 1e-13 * np.abs(I).max()


def test_weights_and_derivative_weights():
    t = np.linspace(0.0, 1.0, 1001)
    w, dw = ref.weights(t), ref.dweights(t)
    assert np.abs(w.sum(0) - 1.0).max() <= 4e-16 and np.abs(dw.sum(0)).max() <= 4e-16
    assert (w >= 0).all()
    h = 1e-5
    ti = t[1:-1]
    assert np.abs((ref.weights(ti + h) - ref.weights(ti - h)) / (2 * h) - ref.dweights(ti)).max() <= 1e-9
    # the pieces join: tap q + 1 of a cell at t = 1 is tap q of the next cell at t = 0 (value and derivative)
    assert np.allclose(ref.weights(1.0)[1:], ref.weights(0.0)[:3], rtol=0, atol=1e-16) and ref.weights(1.0)[0] == 0
    assert np.allclose(ref.dweights(1.0)[1:], ref.dweights(0.0)[:3], rtol=0, atol=1e-16) and ref.dweights(1.0)[0] == 0
    # the kernel's expressions are the same cubics: within 8 u of them at the same t, in both precisions
    for R, u in ((np.float32, 2.0 ** -24), (np.float64, 2.0 ** -53)):
        rng = np.random.default_rng(3)
        tt = np.concatenate([rng.random(200000), 2.0 ** -rng.integers(1, 30, 2000), 1 - 2.0 ** -rng.integers(1, 24, 2000),
                             [0.0, 1.0, 0.5]]).astype(R)
        exact = ref.weights(tt, np.longdouble)
        got = ref.weights_f32(tt).astype(np.longdouble)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(exact == 0, np.where(got == 0, 0.0, np.inf), np.abs(got - exact) / exact)
        print(f"{np.dtype(R).name}: weights within {float(rel.max() / u):.2f} u of the exact cubics")
        assert rel.max() <= 8 * u
        dgot, dexact = ref.dweights_f32(tt).astype(np.longdouble), ref.dweights(tt, np.longdouble)
        assert np.abs(dgot - dexact).max() <= 8 * u


@pytest.mark.parametrize("sp", SHAPES + ((3, 1), (1, 1, 4)), ids=str)
def test_adjoint(sp):
    f, g = ref.image(2, 2, sp, np.float64), ref.image(2, 2, sp, np.float64, seed=1)
    lhs, rhs = (ref.prefilter(f) * g).sum(), (f * ref.prefilter(g, adjoint=True)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.abs(f).max() * np.abs(g).sum())
    for n in sp:   # B^T = D B D^-1, D = diag(1/2, 1, ..., 1, 1/2): the form the kernel runs
        if n >= 2:
            B, D = ref.matrix(n), np.diag([0.5] + [1.0] * (n - 2) + [0.5])
            assert np.abs(B.T - D @ B @ np.linalg.inv(D)).max() <= 1e-16
            assert np.abs(np.linalg.inv(B)).sum(1).max() <= 3.0 + 1e-12   # ||B^-1||_inf <= 3


def test_position_gradient_against_central_differences():
    sp = (5, 6, 7)
    C = ref.prefilter(ref.image(1, 2, sp, np.float64))
    u = labels_ref.displacement("random", 1, sp, np.float64)
    go = ref.image(1, 2, sp, np.float64, seed=3)
    for dt in (1.0, -0.7):
        du = ref.grad_u(go, C, u, dt)
        tp = ref.taps(u, dt)
        h = 1e-6
        for a in range(3):
            up, um = u.copy(), u.copy()
            up[:, a] += h
            um[:, a] -= h
            fd = ((ref.interp(C, up, dt) - ref.interp(C, um, dt)) * go).sum(1) / (2 * h)
            inside = ~tp[a][3]
            assert inside.any() and (~inside).any()
            assert np.abs(du[:, a] - fd)[inside].max() <= 1e-7 * np.abs(fd).max()
            assert (du[:, a][~inside] == 0).all()
    # and the scatter is the gather's transpose
    s, sabs, count = ref.grad_C_wide(go, C.shape, u)
    assert abs((ref.interp(C, u) * go).sum() - (C * s).sum()) <= 1e-12 * (np.abs(C) * sabs).sum()
    assert count.sum() == 64 * np.prod(sp) * 2


# ---- the header against the reference

def _positions(n, dtype):
    """Inside, outside, exactly on both borders and on every grid point, +-inf and NaN."""
    rng = np.random.default_rng([n, np.dtype(dtype).itemsize])
    grid = np.arange(-2, n + 2, dtype=np.float64)
    x = np.concatenate([grid, grid + 0.5, np.nextafter(grid, np.inf), np.nextafter(grid, -np.inf),
                        rng.uniform(0, max(n - 1, 1), 400), rng.uniform(-3, n + 3, 200), 10.0 ** rng.uniform(2, 30, 20),
                        -(10.0 ** rng.uniform(2, 30, 20)), [0.0, -0.0, n - 1.0, np.inf, -np.inf, np.nan, 3e9, -3e9, 1e-30]])
    with np.errstate(over="ignore"):
        return x.astype(dtype)


def _emul_cases():
    return [(dtype, n, _positions(n, dtype)) for dtype in (np.float32, np.float64) for n in (1, 2, 3, 7)]


def _run_emul(tmp_path, name, extra=()):
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    exe = native_build.build(tmp_path, "bspline_emul.cpp", extra=extra, name=name)
    cases = _emul_cases()
    with open(src, "wb") as f:
        for dtype, n, x in cases:
            f.write(struct.pack("<3i", np.dtype(dtype).itemsize, n, x.size))
            f.write(x.tobytes())
    native_build.run(exe, src, dst, quiet=True)
    raw, at = open(dst, "rb").read(), 0
    for dtype, n, x in cases:
        ints = np.frombuffer(raw, dtype="<i4", count=x.size * 6, offset=at).reshape(-1, 6)
        at += ints.nbytes
        reals = np.frombuffer(raw, dtype=dtype, count=x.size * 9, offset=at).reshape(-1, 9)
        at += reals.nbytes
        yield dtype, n, x, ints, reals
    assert at == len(raw)


def _check_emul(results):
    seen = 0
    for dtype, n, x, ints, reals in results:
        what = (np.dtype(dtype).name, n)
        bits = np.uint32 if dtype == np.float32 else np.uint64
        k, f, t, clamped, nan = ref.axis(x, n)
        assert np.array_equal(ints[:, :4], k.T), what
        assert np.array_equal(ints[:, 4], f), what
        assert np.array_equal(ints[:, 5], clamped.astype(np.int64) + 2 * nan), what
        assert ints[:, :4].min() >= 0 and ints[:, :4].max() <= n - 1
        assert clamped.sum() > 40 and nan.sum() == 1 and (~clamped).sum() > (40 if n > 1 else 3)   # (n = 1: only x = 0 is inside)
        assert np.array_equal(reals[:, 0].view(bits), t.view(bits)), what
        with np.errstate(invalid="ignore"):
            w, dw = ref.weights_f32(t), ref.dweights_f32(t)
        assert w.dtype == np.dtype(dtype)
        assert np.array_equal(reals[:, 1:5].view(bits), np.ascontiguousarray(w.T).view(bits)), what
        assert np.array_equal(reals[:, 5:9].view(bits), np.ascontiguousarray(dw.T).view(bits)), what
        ok = ~nan
        assert ((t[ok] >= 0) & (t[ok] <= 1)).all() and np.isnan(reals[nan]).all()
        # exactly on the borders: the border value alone, and no derivative
        for edge in (0.0, n - 1.0):
            at = np.flatnonzero(x == dtype(edge))
            assert at.size and not clamped[at].any()
            for p in at:
                tot = np.zeros(n)
                np.add.at(tot, ints[p, :4], reals[p, 1:5].astype(np.float64))
                dtot = np.zeros(n)
                np.add.at(dtot, ints[p, :4], reals[p, 5:9].astype(np.float64))
                assert abs(tot.sum() - 1) <= 1e-6 and np.abs(dtot).max() <= 1e-6, (what, edge)
        seen += x.size
    assert seen > 5000


@native_build.needs_cxx
def test_header_emulation_equals_the_reference_exactly(tmp_path):
    _check_emul(_run_emul(tmp_path, "bspline_emul"))


@native_build.needs_cxx
def test_header_emulation_under_the_sanitizers(tmp_path):
    """The same stand-alone host program with AddressSanitizer and UndefinedBehaviorSanitizer: the conversions of
    out-of-range, infinite and NaN positions stay defined."""
    _check_emul(_run_emul(tmp_path, "bspline_emul_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")))


# ---- the cell bound, without the kernel

@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9)], ids=str)
def test_float32_restatement_stays_inside_the_cell_bound(sp):
    """The walk of grad_C_wide in float32 with the header's weight expressions and product order -- one of the orders
    the kernel's atomics can take -- against the wide sums: inside bspline_ref.cell_bound on the GPU test's inputs."""
    d, N = len(sp), 2
    worst = 0.0
    for kind in KINDS:
        u = labels_ref.displacement(kind, N, sp, np.float32)
        for K in sorted({1, d, 4}):
            go = ref.image(N, K, sp, np.float32, seed=7)
            for bc in (False, True):
                shape = (1 if bc else N, K) + sp
                wide = ref.grad_C_wide(go, shape, u)
                got, _, _ = ref.grad_C_wide(go, shape, u, wfun=ref.weights_f32, add_dtype=np.float32)
                assert got.dtype == np.float32
                ratio, empty_ok = ref.cell_ratio(got, wide, np.float32, d)
                assert empty_ok and ratio <= 1.0, (kind, K, bc, ratio)
                worst = max(worst, ratio)
    print(f"{sp}: float32 restatement at most {worst:.3f} of the cell bound")
    assert worst > 0.0


# ---- the public surface

def test_names_symbols_and_abi_version():
    import lagomorph_amd as lm
    from lagomorph_amd import bspline, lagomorph_ext as ext

    for name in ("bspline_prefilter", "interp_bspline", "interp_cubic"):
        assert callable(getattr(lm, name)) and getattr(lm, name) is getattr(bspline, name)
        assert getattr(lm, name).__doc__
    assert callable(ext.bspline_prefilter) and callable(ext.interp_bspline_forward) and callable(ext.interp_bspline_backward)
    lib = ctypes.CDLL(ext.LIB_PATH)
    for stem in ("lago_bspline_prefilter", "lago_interp_bspline", "lago_interp_bspline_backward"):
        for suf in ("_f32", "_f64"):
            assert hasattr(lib, stem + suf) and stem + suf in ext._fn, stem + suf
    assert lib.lago_abi_version() == ext.ABI_VERSION == 5
    header = open(os.path.join(os.path.dirname(HERE), "include", "lagomorph_hip.h")).read()
    for text in ("lago_bspline_prefilter##SUF(", "lago_interp_bspline##SUF(", "lago_interp_bspline_backward##SUF("):
        assert text in header, text
    for doc in (bspline.interp_bspline.__doc__, ext.interp_bspline_backward.__doc__, header):
        assert "call to call" in doc   # the last bits of d_C
    assert "mirror" in bspline.bspline_prefilter.__doc__.lower()


def test_argument_errors_are_raised_on_cpu_tensors():
    import lagomorph_amd as lm

    I = torch.zeros((2, 3, 4, 5, 6))
    u = torch.zeros((2, 3, 4, 5, 6))
    I2, u2 = torch.zeros((2, 1, 5, 6)), torch.zeros((2, 2, 5, 6))
    for f in (lm.interp_bspline, lm.interp_cubic):
        with pytest.raises(TypeError):
            f(I.numpy(), u)
        with pytest.raises(TypeError):
            f(I, u.numpy())
        with pytest.raises(TypeError):
            f(I, None)
        with pytest.raises(RuntimeError, match="float32 and float64"):
            f(I.half(), u.half())
        with pytest.raises(RuntimeError, match="float32 and float64"):
            f(I.int(), u)
        with pytest.raises(RuntimeError, match="dtype mismatch"):
            f(I, u.double())
        with pytest.raises(RuntimeError, match="dtype mismatch"):
            f(I.double(), u)
        for bad in (torch.zeros((2, 3, 4)), torch.zeros((4, 5, 6)), torch.zeros((2, 3, 4, 5, 6, 7))):
            with pytest.raises(RuntimeError, match="two or three spatial axes"):
                f(bad, u)
        for bad in (u[:, :2].contiguous(), u[..., :5].contiguous(), u2, torch.zeros((2, 3, 4, 5))):
            with pytest.raises(RuntimeError, match="does not match"):
                f(I, bad)
        with pytest.raises(RuntimeError, match="does not match"):
            f(I2, u)
        with pytest.raises(RuntimeError, match="batch sizes"):
            f(torch.zeros((3, 3, 4, 5, 6)), u)
        with pytest.raises(RuntimeError, match="batch sizes"):
            f(I, u[:1])
        with pytest.raises(RuntimeError, match="contiguous"):
            f(I.transpose(3, 4), u.transpose(3, 4))
        with pytest.raises(RuntimeError, match="contiguous"):
            f(I, torch.zeros((2, 3, 4, 5, 12))[..., ::2])
        for II, uu in ((I, u), (I[:1], u), (I.double(), u.double()), (I2, u2), (I.clone().requires_grad_(True), u)):
            with pytest.raises(RuntimeError, match="CUDA tensor"):   # all fine but for the device
                f(II, uu)
            with pytest.raises(RuntimeError, match="CUDA tensor"):
                f(II, uu, dt=-0.5)
    for adjoint in (False, True):
        with pytest.raises(TypeError):
            lm.bspline_prefilter(I.numpy(), adjoint)
        with pytest.raises(TypeError):
            lm.bspline_prefilter(None, adjoint)
        with pytest.raises(RuntimeError, match="float32 and float64"):
            lm.bspline_prefilter(I.long(), adjoint)
        for bad in (torch.zeros((2, 3, 4)), torch.zeros((5,)), torch.zeros((2, 3, 4, 5, 6, 7))):
            with pytest.raises(RuntimeError, match="two or three spatial axes"):
                lm.bspline_prefilter(bad, adjoint)
        with pytest.raises(RuntimeError, match="contiguous"):
            lm.bspline_prefilter(I.transpose(2, 3), adjoint)
        for II in (I, I.double(), I2, I.clone().requires_grad_(True)):
            with pytest.raises(RuntimeError, match="CUDA tensor"):
                lm.bspline_prefilter(II, adjoint)


def test_c_entry_points_validate_before_any_device_call():
    from lagomorph_amd import lagomorph_ext as ext

    OK, INVALID = 0, -1
    p, q, r, s, t = 0x100000, 0x200000, 0x400000, 0x800000, 0x1000000   # never dereferenced: every call returns before a launch
    err = ext._lib.lago_last_error
    for suf in ("_f32", "_f64"):
        f = ext._fn["lago_bspline_prefilter" + suf]
        assert f(p, q, 0, 4, 1, 4, 4, 4, None) == INVALID and b"dimensional" in err()
        assert f(p, q, 0, 3, 1, 4, -1, 4, None) == INVALID and b"negative" in err()
        assert f(p, q, 0, 3, -1, 4, 4, 4, None) == INVALID
        assert f(p, q, 1, 3, 1, 1 << 31, 1, 1, None) == INVALID and b"2^31" in err()
        assert f(p, q, 0, 3, 1, 1 << 10, 1 << 10, 1 << 9, None) == INVALID and b"2^29" in err()
        assert f(p, p, 0, 3, 1, 4, 4, 4, None) == INVALID and b"overlap" in err()
        assert f(p, p + 16, 1, 2, 2, 4, 4, 1, None) == INVALID and b"overlap" in err()
        assert f(None, q, 0, 3, 1, 4, 4, 4, None) == INVALID and b"null" in err()
        assert f(p, None, 0, 3, 1, 4, 4, 4, None) == INVALID and b"null" in err()
        for ext_ in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0)):   # empty: nothing to do
            assert f(None, None, 0, 3, *ext_, None) == OK
        g = ext._fn["lago_interp_bspline" + suf]
        assert g(p, q, r, 1.0, 1, 1, 1, 4, 4, 4, 0, None) == INVALID and b"dimensional" in err()
        assert g(p, q, r, 1.0, 3, 1, 1, 4, -4, 4, 0, None) == INVALID and b"negative" in err()
        assert g(p, q, r, 1.0, 3, 1, 1, 1 << 10, 1 << 10, 1 << 9, 0, None) == INVALID and b"2^29" in err()
        assert g(p, p, r, 1.0, 3, 1, 1, 4, 4, 4, 0, None) == INVALID and b"overlap" in err()
        assert g(p, q, p + 64, 1.0, 3, 2, 1, 4, 4, 4, 1, None) == INVALID and b"overlap" in err()
        assert g(None, q, r, 1.0, 3, 1, 1, 4, 4, 4, 0, None) == INVALID and b"null" in err()
        for ext_ in ((0, 1, 4, 4, 4), (1, 0, 4, 4, 4), (1, 1, 0, 4, 4), (1, 1, 4, 4, 0)):
            assert g(None, None, None, 1.0, 3, *ext_, 0, None) == OK
        assert g(None, None, None, 1.0, 2, 1, 1, 4, 0, 0, 0, None) == OK
        h = ext._fn["lago_interp_bspline_backward" + suf]
        assert h(p, q, r, s, t, 1.0, 5, 1, 1, 4, 4, 4, 0, 1, 1, None) == INVALID and b"dimensional" in err()
        assert h(p, q, r, s, t, 1.0, 3, 1, 1, 4, 4, 4, 0, 0, 0, None) == OK   # neither gradient wanted
        assert h(None, q, r, s, t, 1.0, 3, 1, 1, 4, 4, 4, 0, 1, 1, None) == INVALID and b"null" in err()
        assert h(p, None, r, s, t, 1.0, 3, 1, 1, 4, 4, 4, 0, 1, 1, None) == INVALID and b"null" in err()
        assert h(p, q, r, None, t, 1.0, 3, 1, 1, 4, 4, 4, 0, 0, 1, None) == INVALID and b"null" in err()
        assert h(p, q, r, s, p, 1.0, 3, 1, 1, 4, 4, 4, 0, 1, 1, None) == INVALID and b"overlap" in err()
        assert h(p, q, q + 8, s, t, 1.0, 3, 1, 1, 4, 4, 4, 0, 0, 1, None) == INVALID and b"overlap" in err()
        assert h(p, p + 8, r, s, t, 1.0, 3, 1, 1, 4, 4, 4, 0, 1, 1, None) == INVALID and b"overlap" in err()
        assert h(None, None, None, None, None, 1.0, 3, 0, 1, 4, 4, 4, 0, 1, 1, None) == OK
