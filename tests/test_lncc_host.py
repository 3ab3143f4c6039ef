"""CPU: the test-side reference of lncc (tests/lncc_ref.py) -- its gradient against central differences, its symmetry, and
the condition the shared GPU cases are chosen under (their float32 emulation stays within half the GPU tolerance) --
and the public surface, C symbols and argument checks of the operator, none of which reaches the device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lncc_ref
import parity_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = lncc_ref.MODES


def field(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sp,sigma", [((4, 5, 6), 1.0), ((4, 5, 6), (1.0, 0.0, 0.6)), ((5, 7), (0.7, 1.5)), ((6, 9), 2.5)])
def test_reference_gradient_against_central_differences(sp, sigma, mode):
    """d/dh sum(g cc(I + h d, J + h e)) at h = 0 against <dI, d> + <dJ, e>, separately for I and J, in float64 with step
    1e-6: the truncation error is O(h^2) = 1e-12 and the rounding error 1e-16 / h = 1e-10 of the values, far inside 1e-6."""
    shape = (2, 2) + sp
    I = field(shape, 1)
    J = 0.8 * I + 0.6 * field(shape, 2)
    g, d, e = field(shape, 3), field(shape, 4), field(shape, 5)
    cc, dI, dJ = lncc_ref.lncc_with_grads(I, J, g, sigma, mode=mode)
    assert cc.shape == shape and cc.min() >= 0.0 and cc.max() <= 1.0
    h = 1e-6
    loss = lambda a, b: np.sum(g * lncc_ref.lncc(a, b, sigma, mode=mode))
    for an, fd in ((np.sum(dI * d), (loss(I + h * d, J) - loss(I - h * d, J)) / (2 * h)),
                   (np.sum(dJ * e), (loss(I, J + h * e) - loss(I, J - h * e)) / (2 * h))):
        err = abs(an - fd) / abs(fd)
        print(f"{sp} sigma {sigma} {mode}: analytic {an:.12e}, central difference {fd:.12e}, relative error {err:.2e}")
        assert err <= 1e-6


@pytest.mark.parametrize("mode", MODES)
def test_reference_is_symmetric_in_its_arguments(mode):
    shape = (2, 2, 5, 6, 7)
    I, J, g = field(shape, 6), field(shape, 7) + 0.5, field(shape, 8)
    for sigma in (1.0, (1.5, 0.0, 0.7)):
        a = lncc_ref.lncc_with_grads(I, J, g, sigma, mode=mode)
        b = lncc_ref.lncc_with_grads(J, I, g, sigma, mode=mode)
        assert np.array_equal(a[0], b[0])
        assert np.abs(a[1] - b[2]).max() <= 1e-14 * np.abs(a[1]).max() and np.abs(a[2] - b[1]).max() <= 1e-14 * np.abs(a[2]).max()
    # an image against itself: sX = sI = sJ
    cc = lncc_ref.lncc(I, I, 1.0, mode=mode, eps=0.0)
    assert np.abs(cc - 1.0).max() <= 1e-12
    # eps = 0: invariant to an affine change of contrast
    a, b = lncc_ref.lncc(I, J, 1.0, mode="wrap", eps=0.0), lncc_ref.lncc(-2.5 * I + 3.0, J, 1.0, mode="wrap", eps=0.0)
    assert np.abs(a - b).max() <= 1e-10 * np.abs(a).max()


@pytest.mark.parametrize("sp", lncc_ref.SHAPES)
def test_float32_emulation_of_the_shared_cases_is_within_half_the_gpu_tolerance(sp):
    """The input guard: float32 loses accuracy where a window holds few samples and the local variance is small against
    the local mean square -- a property of the formula, not of a kernel.  Every case tests/test_gpu_lncc.py runs must
    therefore leave the best a float32 device can do (lncc_ref.emulate) within 0.5 of the GPU tolerance, for cc, dI and
    dJ.  A case that breaks this is replaced (lncc_ref.DRAW), the cap stays."""
    worst = 0.0
    for kind in lncc_ref.KINDS:
        for sigma in lncc_ref.sigmas_of(sp, kind):
            for mode in MODES:
                em = lncc_ref.emulate(np.float32)(*lncc_ref.inputs(sp, kind), sigma, mode=mode)
                ref = lncc_ref.reference(sp, kind, sigma, mode)
                u = [parity_rule.units(a, b, np.float32) for a, b in zip(em, ref)]
                worst = max(worst, max(u))
                assert max(u) <= 0.5, f"{sp} {kind} sigma={sigma} {mode}: cc, dI, dJ at {u} of the tolerance"
    print(f"{sp}: worst {worst:.3f} of the tolerance")


def test_shared_cases_follow_the_guard():
    assert 0.5 not in lncc_ref.sigmas_of((5, 6, 7), "affine") and 0.5 in lncc_ref.sigmas_of((5, 6, 7), "corr")
    assert lncc_ref.sigmas_of((5, 6, 7), "affine") == [1.0, 2.5, 8.0, (1.5, 0.0, 0.7)]
    assert lncc_ref.sigmas_of((7, 9), "indep") == [0.5, 1.0, 2.5, 8.0, (1.5, 0.7)]
    assert lncc_ref.sigmas_of((2, 2, 2), "corr") == [0.5, 1.0, 2.5, 8.0]
    assert all(min(sp) > 1 for sp in lncc_ref.SHAPES) and len(lncc_ref.SHAPES) == 14
    I, J, g = lncc_ref.inputs((5, 6, 7), "affine")
    assert I.shape == (2, 2, 5, 6, 7) and np.array_equal(I, I.astype(np.float32)) and np.array_equal(J, J.astype(np.float32))
    assert abs(J.mean() - 3.0) < 0.5 and abs(I.mean()) < 0.2 and abs(g.std() - 1.0) < 0.2


def test_public_surface():
    import lagomorph_amd as lm

    assert callable(lm.lncc) and callable(lm.lncc_loss) and callable(lm.LNCCSimilarity(2.0))
    assert issubclass(lm.LNCCFunction, torch.autograd.Function)
    for name in ("lncc_moments", "lncc_cc", "lncc_backward"):
        assert callable(getattr(lm.lagomorph_ext, name)), name
    assert "five" in lm.LNCCFunction.__doc__.lower() and "volumes" in lm.LNCCFunction.__doc__
    doc = lm.lncc.__doc__
    assert "singleton" in doc and "float32" in doc and "wrap" in doc and "zero" in doc
    s = lm.LNCCSimilarity((1.0, 2.0, 3.0), truncate=3.0, mode="zero", eps=1e-3)
    assert (s.sigma, s.truncate, s.mode, s.eps) == ((1.0, 2.0, 3.0), 3.0, "zero", 1e-3)
    import inspect

    assert inspect.signature(lm.lddmm_step).parameters["similarity"].default is None
    assert inspect.signature(lm.LDDMMAtlasBuilder.__init__).parameters["similarity"].default is None
    assert list(inspect.signature(lm.lncc).parameters) == ["I", "J", "sigma", "truncate", "mode", "eps"]


def test_header_declares_and_library_exports_the_entry_points():
    import lagomorph_amd

    text = open(os.path.join(ROOT, "include", "lagomorph_hip.h")).read()
    block = text[text.index("#define LAGO_DECLARE(REAL, SUF)"):text.index("LAGO_DECLARE(float, _f32)")]
    lib = ctypes.CDLL(lagomorph_amd.lagomorph_ext.LIB_PATH)
    for name in ("lago_lncc_moments", "lago_lncc_cc", "lago_lncc_coeffs", "lago_lncc_combine"):
        assert re.search(r"\bint " + name + r"##SUF\s*\(", block), f"{name} is not declared inside the ##SUF block"
        assert hasattr(lib, name + "_f32") and hasattr(lib, name + "_f64"), name
    assert block.count("No counterpart in the reference") >= 5
    assert lib.lago_abi_version() == 5


def test_c_entry_points_reject_bad_arguments_before_touching_the_gpu():
    """None of these calls reaches a launch, so they are made with host addresses that are never dereferenced."""
    import lagomorph_amd

    lib = ctypes.CDLL(lagomorph_amd.lagomorph_ext.LIB_PATH)
    lib.lago_last_error.restype = ctypes.c_char_p
    a, b, c, d = (np.zeros(5 * 2 * 64, dtype=np.float64) for _ in range(4))
    taps = (ctypes.c_double * (3 * 33))(*([1.0] + [0.0] * 32) * 3)
    i64, vp, cint, dbl = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    P = lambda x: None if x is None else x.ctypes.data
    for suf in ("_f32", "_f64"):
        mom = getattr(lib, "lago_lncc_moments" + suf)
        mom.argtypes = [vp, vp, vp, vp, vp, vp, cint, cint, i64, i64, i64, i64, vp]
        cc = getattr(lib, "lago_lncc_cc" + suf)
        cc.argtypes = [vp, vp, dbl, i64, vp]
        co = getattr(lib, "lago_lncc_coeffs" + suf)
        co.argtypes = [vp, vp, vp, dbl, cint, i64, vp]
        cb = getattr(lib, "lago_lncc_combine" + suf)
        cb.argtypes = [vp, vp, vp, vp, vp, cint, i64, vp]
        for f in (mom, cc, co, cb):
            f.restype = cint

        def moments(out, I, J, scr, radii, mode=0, dim=3, rows=2, ext=(4, 4, 4), tp=taps):
            rad = (ctypes.c_int * 3)(*radii) if radii is not None else None
            return mom(P(out), P(I), P(J), P(scr), rad, tp, mode, dim, rows, *ext, None)

        assert moments(a, b, c, d, (1, 33, 1)) != 0 and b"radius 33" in lib.lago_last_error()
        assert moments(a, b, c, d, (-1, 0, 0)) != 0 and b"radius" in lib.lago_last_error()
        assert moments(a, b, c, d, (1, 1, 1), mode=2) != 0 and b"mode" in lib.lago_last_error()
        assert moments(a, b, c, d, (1, 1, 1), dim=4) != 0
        assert moments(a, b, c, d, (1, 1, 1), dim=1) != 0
        assert moments(a, b, c, d, None) != 0
        assert moments(a, b, c, d, (0, 0, 1), tp=None) != 0 and b"taps" in lib.lago_last_error()
        assert moments(a, a, c, d, (1, 1, 1)) != 0 and b"alias" in lib.lago_last_error()
        assert moments(a, b, a, d, (0, 0, 1)) != 0 and b"alias" in lib.lago_last_error()
        assert moments(a, b, c, None, (1, 0, 1)) != 0 and b"scratch" in lib.lago_last_error()
        assert moments(a, b, c, a, (0, 1, 0)) != 0 and b"scratch" in lib.lago_last_error()
        assert moments(a, b, c, d, (1, 1, 1), ext=(0, 4, 4)) != 0
        assert moments(a, b, c, d, (1, 1, 1), rows=0) == 0
        assert moments(None, None, None, None, (1, 1, 1), rows=0, dim=2, ext=(4, 4, 1)) == 0
        assert cc(P(a), P(b), -1.0, 8, None) != 0 and b"eps" in lib.lago_last_error()
        assert cc(P(a), P(b), float("nan"), 8, None) != 0
        assert cc(P(a), P(a), 1e-5, 8, None) != 0 and b"alias" in lib.lago_last_error()
        assert cc(P(a), None, 1e-5, 8, None) != 0
        assert cc(P(a), P(b), 1e-5, -1, None) != 0
        assert cc(None, None, 1e-5, 0, None) == 0
        for which in (0, 4, -1):
            assert co(P(a), P(b), P(c), 1e-5, which, 8, None) != 0 and b"which" in lib.lago_last_error()
            assert cb(P(a), P(d), P(b), P(c), P(c), which, 8, None) != 0 and b"which" in lib.lago_last_error()
        assert co(P(a), P(b), P(c), -1e-5, 3, 8, None) != 0 and b"eps" in lib.lago_last_error()
        assert co(P(a), P(a), P(c), 1e-5, 3, 8, None) != 0 and b"alias" in lib.lago_last_error()
        assert co(P(a), P(b), None, 1e-5, 1, 8, None) != 0
        assert co(None, None, None, 1e-5, 1, 0, None) == 0
        assert cb(None, P(d), P(b), P(c), P(c), 1, 8, None) != 0          # dI is what which = 1 writes
        assert cb(P(a), None, P(b), P(c), P(c), 2, 8, None) != 0
        assert cb(P(a), P(a), P(b), P(c), P(c), 3, 8, None) != 0 and b"alias" in lib.lago_last_error()
        assert cb(P(a), P(d), P(b), P(a), P(c), 3, 8, None) != 0 and b"alias" in lib.lago_last_error()
        assert cb(None, None, None, None, None, 3, 0, None) == 0


def test_argument_errors_are_raised_before_any_device_work():
    """On CPU tensors: every argument error comes first, and valid arguments end at the device check (no CPU path)."""
    import lagomorph_amd as lm

    ext = lm.lagomorph_ext
    x3, y3, x2 = torch.zeros((1, 2, 4, 5, 6)), torch.ones((1, 2, 4, 5, 6)), torch.zeros((1, 1, 4, 5))
    with pytest.raises(ValueError, match="FFT operator"):        # r = int(4 * 8.2 + 0.5) = 33
        lm.lncc(x3, y3, 8.2)
    with pytest.raises(ValueError, match="one per spatial axis"):
        lm.lncc(x3, y3, (1.0, 1.0))
    with pytest.raises(ValueError, match="unknown mode"):
        lm.lncc(x3, y3, 1.0, mode="reflect")
    with pytest.raises(ValueError, match="eps"):
        lm.lncc(x3, y3, 1.0, eps=-1e-5)
    with pytest.raises(RuntimeError, match="same shape"):
        lm.lncc(x3, x2, 1.0)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        lm.lncc(x3, y3.double(), 1.0)
    with pytest.raises(TypeError, match="torch.Tensor"):
        lm.lncc(x3, np.zeros((1, 2, 4, 5, 6)), 1.0)
    with pytest.raises(RuntimeError, match="two- and three-dimensional"):
        lm.lncc(torch.zeros((1, 1, 4)), torch.zeros((1, 1, 4)), 1.0)
    with pytest.raises(ValueError, match="reduction"):
        lm.lncc_loss(x3, y3, 1.0, reduction="max")
    with pytest.raises(ValueError, match="unknown mode"):
        lm.LNCCSimilarity(1.0, mode="nearest")
    with pytest.raises(ValueError, match="eps"):
        lm.LNCCSimilarity(1.0, eps=-1.0)
    for a, b in ((x3, y3), (x2, x2)):                            # valid arguments: r = 32 is accepted, the device check ends it
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            lm.lncc(a, b, 8.0)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            lm.lncc_loss(a, b, 0.0, mode="zero", reduction="sum")
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        lm.LNCCSimilarity(1.0)(x3, y3)
    t = [lm.gaussian_taps(0.25), None, lm.gaussian_taps(0.5)]
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ext.lncc_moments(x3, y3, [1, 0, 2], t, "wrap")
    with pytest.raises(ValueError, match="outside 0..32"):
        ext.lncc_moments(x3, y3, [33, 0, 0], [np.ones(67) / 67, None, None], "wrap")
    with pytest.raises(ValueError, match="taps"):
        ext.lncc_moments(x3, y3, [1, 0, 0], [np.ones(5) / 5, None, None], "wrap")
    with pytest.raises(ValueError, match="symmetric"):
        ext.lncc_moments(x3, y3, [1, 0, 0], [np.array([0.2, 0.5, 0.3]), None, None], "wrap")
    with pytest.raises(ValueError, match="one per spatial axis"):
        ext.lncc_moments(x3, y3, [1, 0], [None, None], "wrap")
    with pytest.raises(ValueError, match="unknown mode"):
        ext.lncc_moments(x3, y3, [0, 0, 0], [None] * 3, "clamp")
    with pytest.raises(RuntimeError, match="float32 and float64"):
        ext.lncc_moments(x3.int(), y3.int(), [0, 0, 0], [None] * 3, "wrap")
    with pytest.raises(RuntimeError, match="same shape"):
        ext.lncc_moments(x3, x2, [0, 0, 0], [None] * 3, "wrap")
    m3 = torch.zeros((5, 1, 2, 4, 5, 6))
    with pytest.raises(RuntimeError, match=r"\(5, N, C"):
        ext.lncc_cc(x3, 1e-5)
    with pytest.raises(ValueError, match="eps"):
        ext.lncc_cc(m3, -1.0)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ext.lncc_cc(m3, 1e-5)
    with pytest.raises(RuntimeError, match="grad_out must have the shape"):
        ext.lncc_backward(x2, x3, y3, m3, [1, 0, 2], t, "wrap", 1e-5)
    with pytest.raises(RuntimeError, match="grad_out must have the shape"):
        ext.lncc_backward(x3, x3, y3, m3[:3], [1, 0, 2], t, "wrap", 1e-5)
    with pytest.raises(ValueError, match="eps"):
        ext.lncc_backward(x3, x3, y3, m3, [1, 0, 2], t, "wrap", -1.0)
    with pytest.raises(ValueError, match="symmetric"):
        ext.lncc_backward(x3, x3, y3, m3, [1, 0, 0], [np.array([0.2, 0.5, 0.3]), None, None], "wrap", 1e-5)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ext.lncc_backward(x3, x3, y3, m3, [1, 0, 2], t, "wrap", 1e-5)
    assert ext.lncc_backward(x3, x3, y3, m3, [1, 0, 2], t, "wrap", 1e-5, need_I=False, need_J=False) == (None, None)


# ---- the host logic on CPU tensors: the oracle stands in for the geometry kernels, gauss_ref / lncc_ref for the filters

@pytest.fixture
def ref_lncc(monkeypatch):
    import gauss_ref
    import lagomorph_amd

    ext = lagomorph_amd.lagomorph_ext
    calls = []

    def tap_list(radii, taps):
        tl = [np.asarray(t, dtype=np.float64) if r > 0 else np.ones(1) for r, t in zip(radii, taps)]
        assert all(len(t) == 2 * r + 1 for r, t in zip(radii, tl))
        return tl

    def smooth(x, radii, taps, mode, alpha=1.0, out=None, accumulate=False):
        calls.append(("smooth", tuple(x.shape)))
        y = torch.from_numpy(alpha * gauss_ref.smooth_taps(x.detach().numpy(), tap_list(radii, taps), mode)).to(x.dtype)
        if out is None:
            assert not accumulate
            return y
        return out.add_(y) if accumulate else out.copy_(y)

    def moments(I, J, radii, taps, mode):
        a, b = I.detach().numpy().astype(np.float64), J.detach().numpy().astype(np.float64)
        calls.append(("moments", tuple(I.shape)))
        return torch.from_numpy(np.stack([gauss_ref.smooth_taps(f, tap_list(radii, taps), mode)
                                          for f in (a, b, a * a, a * b, b * b)])).to(I.dtype)

    def stats(mom):
        A, B, C, D, E = mom.double().unbind(0)
        return A, B, C - A * A, E - B * B, D - A * B

    def cc(mom, eps):
        A, B, sI, sJ, sX = stats(mom)
        return (sX * sX / (sI * sJ + eps)).to(mom.dtype)

    def backward(g, I, J, mom, radii, taps, mode, eps, need_I=True, need_J=True):
        calls.append(("backward", bool(need_I), bool(need_J)))
        A, B, sI, sJ, sX = stats(mom)
        den = sI * sJ + eps
        cX, cI, cJ = 2 * sX / den, -sX * sX * sJ / (den * den), -sX * sX * sI / (den * den)
        G = lambda f: torch.from_numpy(gauss_ref.smooth_taps(f.numpy(), tap_list(radii, taps), mode))
        g = g.double()
        dI = (G(g * (-2 * A * cI - B * cX)) + 2 * I.double() * G(g * cI) + J.double() * G(g * cX)).to(I.dtype) if need_I else None
        dJ = (G(g * (-2 * B * cJ - A * cX)) + 2 * J.double() * G(g * cJ) + I.double() * G(g * cX)).to(I.dtype) if need_J else None
        return dI, dJ

    monkeypatch.setattr(ext, "gaussian_smooth_forward", smooth)
    monkeypatch.setattr(ext, "lncc_moments", moments)
    monkeypatch.setattr(ext, "lncc_cc", cc)
    monkeypatch.setattr(ext, "lncc_backward", backward)
    return calls


@pytest.mark.parametrize("mode", MODES)
def test_function_wiring_on_the_host(ref_lncc, mode):
    """LNCCFunction saves what its backward needs, asks only for the gradients that are needed, and lncc_loss /
    LNCCSimilarity reduce 1 - cc."""
    import lagomorph_amd as lm

    sp, sigma = (5, 6, 7), (1.0, 0.0, 0.7)
    Ih, Jh, gh = lncc_ref.inputs(sp, "corr")
    want = lncc_ref.lncc_with_grads(Ih, Jh, gh, sigma, truncate=3.0, mode=mode, eps=1e-3)
    I, J, g = (torch.from_numpy(np.array(a)) for a in (Ih, Jh, gh))
    I.requires_grad_(True)
    J.requires_grad_(True)
    cc = lm.lncc(I, J, sigma, truncate=3.0, mode=mode, eps=1e-3)
    dI, dJ = torch.autograd.grad(cc, (I, J), g)
    for got, ref in zip((cc, dI, dJ), want):
        assert np.abs(got.detach().numpy() - ref).max() <= 1e-13 * np.abs(ref).max()
    assert ref_lncc[-1] == ("backward", True, True)
    (oI,) = torch.autograd.grad(lm.lncc(I, J.detach(), sigma, truncate=3.0, mode=mode, eps=1e-3), (I,), g)
    assert ref_lncc[-1] == ("backward", True, False) and torch.equal(oI, dI)
    with torch.no_grad():
        none = lm.lncc_loss(I, J, sigma, mode=mode, reduction="none")
        assert torch.equal(none, 1.0 - lm.lncc(I, J, sigma, mode=mode))
        assert torch.equal(lm.lncc_loss(I, J, sigma, mode=mode), none.mean())
        assert torch.equal(lm.lncc_loss(I, J, sigma, mode=mode, reduction="sum"), none.sum())
        assert torch.equal(lm.LNCCSimilarity(sigma, mode=mode)(I, J), none.sum())
    # a transposed view is made contiguous before it is saved
    It = I.detach().transpose(2, 3).contiguous().transpose(2, 3)
    assert not It.is_contiguous() and torch.equal(lm.lncc(It, J.detach(), sigma, mode=mode), lm.lncc(I.detach(), J.detach(), sigma, mode=mode))


def _blobs():
    sp = (16, 16, 16)
    g = np.indices(sp).astype(np.float64)
    blob = lambda c: np.exp(-sum((g[a] - c[a]) ** 2 for a in range(3)) / (2 * 3.0 ** 2))
    return sp, torch.from_numpy(blob((8, 8, 8))[None, None]), torch.from_numpy(np.stack([blob((9, 8, 7)), blob((7, 9, 8))])[:, None])


def test_lddmm_step_takes_a_similarity(oracle_ext, ref_lncc):
    """The plain form of the step on CPU tensors: the squared difference passed as `similarity` is the default call bit
    for bit, and LNCCSimilarity lowers 1 - mean cc on intensity-inverted targets that the squared difference cannot match."""
    import lagomorph_amd as lm

    sp, I, targets = _blobs()
    metric = lm.GaussianMetric([1.5, 3.0], weights=[1.0, 0.5])
    kw = dict(dataset_size=2, integration_steps=3, reg_weight=1e-2, learning_rate_pose=2e2)
    res = []
    for sim in (None, lambda a, b: torch.nn.functional.mse_loss(a, b, reduction="sum")):
        Ia = I.clone().requires_grad_(True)
        m = torch.from_numpy(0.05 * np.random.default_rng(41).standard_normal((2, 3) + sp))
        m, loss, reg = lm.lddmm_step(Ia, m, targets, metric, similarity=sim, **kw)
        res.append((m.detach().clone(), loss, reg, Ia.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*res)) and float(res[0][3].abs().max()) > 0
    img = 1.0 - 2.0 * targets
    sim = lm.LNCCSimilarity(2.0)

    def term(mm):
        with torch.no_grad():
            return float(lm.lncc_loss(lm.interp(I, lm.expmap(metric, mm, num_steps=3)), img, 2.0))

    m = torch.zeros((2, 3) + sp, dtype=torch.float64)
    before = term(m)
    m, loss1, reg1 = lm.lddmm_step(I, m, img, metric, similarity=sim, **kw)
    m, loss2, reg2 = lm.lddmm_step(I, m, img, metric, similarity=sim, **kw)
    after = term(m)
    img1, img2 = float(loss1) - float(reg1), float(loss2) - float(reg2)
    print(f"1 - mean cc: {before:.6e} at m = 0, first call {img1:.6e}, second call {img2:.6e}; after two steps {after:.6e}")
    assert abs(img1 - before) <= 1e-12 * before
    assert img2 < img1 and after < img2 and bool(torch.isfinite(m).all()) and float(m.abs().max()) > 0
