"""CPU: the test-side reference of gaussian_smooth (tests/gauss_ref.py) against scipy.ndimage.gaussian_filter, against a
torch conv1d restatement and against known answers; the float32 rounding budget of three sequential passes; the
operator's public surface, C symbols and argument checks; GaussianMetric's host logic on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gauss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(5, 6, 7), (3, 4, 1), (2, 2, 2), (9, 5, 70), (3, 4, 128), (7, 9), (5, 1), (3, 130), (1, 1, 1)]
MODES = ["wrap", "zero"]
GPU_RTOL32 = 1e-5   # tests/test_gpu_gauss.py: max|got - ref| <= 1e-5 max|ref| in float32


def sigma_sets(dim):
    """0.5 (r = 2), 1 (r = 4), 2.5 (r = 10), 8 (r = 32: far above most extents here), and a per-axis set with a zero."""
    return [0.5, 1.0, 2.5, 8.0, (0.0, 1.5, 0.7)[3 - dim:]]


def field(sp, seed=0, nc=2):
    return np.random.default_rng(seed).standard_normal((1, nc) + sp)


def rel(got, want):
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sp", SHAPES)
def test_reference_agrees_with_scipy(sp, mode):
    ndi = pytest.importorskip("scipy.ndimage")
    x = field(sp, len(sp))
    for sigma in sigma_sets(len(sp)):
        got = gauss_ref.smooth(x, sigma, mode=mode)
        want = np.stack([np.stack([ndi.gaussian_filter(x[n, c], sigma=sigma, mode="wrap" if mode == "wrap" else "constant",
                                                       cval=0.0, truncate=4.0) for c in range(x.shape[1])])
                         for n in range(x.shape[0])])
        err = rel(got, want)
        print(f"{sp} {mode} sigma {sigma}: {err:.3e} of max|scipy|")
        assert got.dtype == np.float64 and got.shape == x.shape
        assert err <= 1e-13   # two float64 evaluations of the same sums in different orders


def conv1d_restatement(x, sigma, mode):
    """The same operator through torch.nn.functional.conv1d in float64 (a cross-correlation, like the definition)."""
    y = torch.from_numpy(np.asarray(x, dtype=np.float64))
    dim = y.dim() - 2
    for a, s in enumerate(gauss_ref.per_axis(sigma, dim)):
        w = torch.from_numpy(gauss_ref.taps(s))
        r = (len(w) - 1) // 2
        if r == 0:
            continue
        y = y.movedim(2 + a, -1)
        sh = y.shape
        n = sh[-1]
        lines = y.reshape(-1, 1, n)
        idx = torch.arange(-r, n + r)
        if mode == "wrap":
            padded = lines[..., idx % n]
        else:
            padded = torch.zeros(lines.shape[:-1] + (n + 2 * r,), dtype=torch.float64)
            padded[..., r:r + n] = lines
        y = torch.nn.functional.conv1d(padded, w.reshape(1, 1, -1)).reshape(sh).movedim(-1, 2 + a)
    return y.contiguous().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sp", SHAPES)
def test_reference_agrees_with_conv1d_restatement(sp, mode):
    x = field(sp, 10 + len(sp))
    for sigma in sigma_sets(len(sp)):
        err = rel(gauss_ref.smooth(x, sigma, mode=mode), conv1d_restatement(x, sigma, mode))
        print(f"{sp} {mode} sigma {sigma}: {err:.3e}")
        assert err <= 1e-13


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9), (2, 2, 2), (3, 130)])
def test_reference_is_self_adjoint(sp, mode):
    x, y = field(sp, 1), field(sp, 2)
    for sigma in sigma_sets(len(sp)):
        a = np.sum(gauss_ref.smooth(x, sigma, mode=mode) * y)
        b = np.sum(x * gauss_ref.smooth(y, sigma, mode=mode))
        assert abs(a - b) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y)


def test_gaussian_taps_equal_the_reference_taps_bit_for_bit():
    import lagomorph_amd as lm

    for truncate in (4.0, 3.0, 2.5):
        for sigma in (0.0, -1.0, 0.1, 0.124, 0.125, 0.5, 0.7, 1.0, 1.5, 2.5, 3.3, 8.0, 8.12):
            got, want = lm.gaussian_taps(sigma, truncate), gauss_ref.taps(sigma, truncate)
            assert got.dtype == np.float64 and np.array_equal(got, want), (sigma, truncate)
            assert len(got) == 2 * int(truncate * max(sigma, 0) + 0.5) + 1
            assert abs(got.sum() - 1.0) <= 1e-15 * len(got) and np.array_equal(got, got[::-1])
    assert np.array_equal(lm.gaussian_taps(2.0), lm.gaussian_taps(2.0, truncate=4.0))


@pytest.mark.parametrize("mode", MODES)
def test_known_answers(mode):
    # a unit impulse gives the outer product of the tap vectors (away from the border in zero mode; wrapped otherwise)
    sp, sig = (13, 11, 17), (1.0, 0.7, 1.5)
    x = np.zeros((1, 1) + sp)
    x[0, 0, 6, 5, 8] = 1.0
    w = [gauss_ref.taps(s) for s in sig]
    r = [(len(t) - 1) // 2 for t in w]
    got = gauss_ref.smooth(x, sig, mode=mode)
    box = got[0, 0, 6 - r[0]:7 + r[0], 5 - r[1]:6 + r[1], 8 - r[2]:9 + r[2]]
    want = np.einsum("i,j,k->ijk", *w)
    assert box.shape == want.shape and np.abs(box - want).max() <= 1e-16
    assert abs(got.sum() - 1.0) <= 1e-14 and np.count_nonzero(got) == want.size
    # a constant: preserved by the periodic border, reduced to the partial tap sums at a zero border
    c = np.full((1, 2, 9, 12), 3.0)
    got = gauss_ref.smooth(c, (2.5, 1.0), mode=mode)
    if mode == "wrap":
        assert np.abs(got - 3.0).max() <= 1e-14
    else:
        def partial(n, t):
            rr = (len(t) - 1) // 2
            return np.array([t[max(0, rr - i):min(len(t), rr + n - i)].sum() for i in range(n)])
        want = 3.0 * np.outer(partial(9, gauss_ref.taps(2.5)), partial(12, gauss_ref.taps(1.0)))
        assert np.abs(got[0, 0] - want).max() <= 1e-14 and np.abs(got[0, 1] - want).max() <= 1e-14
        assert got[0, 0, 0, 0] < 3.0 * 0.5 and abs(got[0, 0, 4, 6] - 3.0 * partial(9, gauss_ref.taps(2.5))[4]) <= 1e-14
    # an impulse with the radius far above the extent, periodic: every tap lands somewhere, the sum stays 1
    x = np.zeros((1, 1, 3, 5))
    x[0, 0, 1, 2] = 1.0
    got = gauss_ref.smooth(x, 8.0, mode="wrap")
    assert abs(got.sum() - 1.0) <= 1e-14 and got.min() > 0.0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sp", [(5, 6, 7), (9, 5, 70), (33, 33, 33), (3, 130)])
def test_float32_emulation_of_sequential_passes_is_within_half_the_gpu_tolerance(sp, mode):
    """What a float32 device can reach: taps rounded once to float32, every pass a float32 running sum over the taps,
    every intermediate stored as float32.  Against the float64 reference that must stay within 0.5 of the bound the
    GPU tests apply (1e-5 x max|ref|), so that bound has room for another order of summation."""
    x32 = field(sp, 3).astype(np.float32)
    for sigma in sigma_sets(len(sp)):
        ref = gauss_ref.smooth(x32.astype(np.float64), sigma, mode=mode)
        y = x32
        for a, s in enumerate(gauss_ref.per_axis(sigma, len(sp))):
            w = gauss_ref.taps(s).astype(np.float32)
            r = (len(w) - 1) // 2
            if r == 0:
                continue
            acc = np.zeros_like(y)
            for k in range(-r, r + 1):
                acc = (acc + w[k + r] * gauss_ref.shifted(y, k, 2 + a, mode)).astype(np.float32)
            y = acc
        units = np.abs(y.astype(np.float64) - ref).max() / (GPU_RTOL32 * np.abs(ref).max())
        print(f"{sp} {mode} sigma {sigma}: {units:.3f} of the GPU tolerance")
        assert units <= 0.5


def test_public_surface():
    import lagomorph_amd as lm

    assert callable(lm.gaussian_smooth) and callable(lm.gaussian_taps)
    assert issubclass(lm.GaussianSmoothFunction, torch.autograd.Function)
    assert callable(lm.lagomorph_ext.gaussian_smooth_forward)
    assert lm.lagomorph_ext.GAUSS_MAX_RADIUS == 32 == gauss_ref.MAX_RADIUS
    m = lm.GaussianMetric([1.0, (2.0, 1.0, 0.5)], weights=[0.25, 2.0], mode="zero", truncate=3.0)
    assert (m.sigmas, m.weights, m.mode, m.truncate) == ([1.0, (2.0, 1.0, 0.5)], [0.25, 2.0], "zero", 3.0)
    assert lm.GaussianMetric([1.0, 2.0]).weights == [1.0, 1.0] and lm.GaussianMetric([1.0]).mode == "wrap"
    assert "not a bounded operator" in lm.GaussianMetric.__doc__ and "momentum_preconditioning" in lm.GaussianMetric.__doc__
    doc = lm.gaussian_smooth.__doc__
    assert "wrap" in doc and "zero" in doc and "32" in doc
    # the factory is unchanged
    import argparse

    p = argparse.ArgumentParser()
    lm.Metric.add_args(p)
    assert isinstance(lm.Metric.from_args(p.parse_args([])), lm.FluidMetric)


def test_header_declares_and_library_exports_the_entry_point():
    import lagomorph_amd

    text = open(os.path.join(ROOT, "include", "lagomorph_hip.h")).read()
    block = text[text.index("#define LAGO_DECLARE(REAL, SUF)"):text.index("LAGO_DECLARE(float, _f32)")]
    assert re.search(r"\bint lago_gauss_smooth##SUF\s*\(", block), "lago_gauss_smooth is not declared inside the ##SUF block"
    assert len(re.findall(r"#define LAGO_GAUSS_MAX_RADIUS 32\b", text)) == 1
    lib = ctypes.CDLL(lagomorph_amd.lagomorph_ext.LIB_PATH)
    for name in ("lago_gauss_smooth_f32", "lago_gauss_smooth_f64"):
        assert hasattr(lib, name), name
    assert lib.lago_abi_version() == 5


def test_c_entry_point_rejects_bad_arguments_before_touching_the_gpu():
    """A radius outside 0..32, an unknown mode, a dim outside {2, 3}, out aliasing in, missing scratch / radii are
    LAGO_ERR_INVALID; rows == 0 is a successful no-op.  None of these reaches a launch, so the calls are made here with
    host addresses that are never dereferenced."""
    import lagomorph_amd

    lib = ctypes.CDLL(lagomorph_amd.lagomorph_ext.LIB_PATH)
    lib.lago_last_error.restype = ctypes.c_char_p
    a, b, c = (np.zeros(2 * 64, dtype=np.float64) for _ in range(3))
    taps = (ctypes.c_double * (3 * 33))(*([1.0] + [0.0] * 32) * 3)
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    for suf in ("_f32", "_f64"):
        f = getattr(lib, "lago_gauss_smooth" + suf)
        f.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, i64, i64, i64, i64, vp]
        f.restype = ctypes.c_int

        def call(out, inp, scr, radii, mode=0, dim=3, rows=2, ext=(4, 4, 4), acc=0, tp=taps):
            rad = (ctypes.c_int * 3)(*radii) if radii is not None else None
            return f(out.ctypes.data, inp.ctypes.data, None if scr is None else scr.ctypes.data, rad, tp, mode, 1.0, acc,
                     dim, rows, *ext, None)

        assert call(a, b, c, (1, 33, 1)) != 0 and b"radius 33" in lib.lago_last_error()
        assert call(a, b, c, (-1, 0, 0)) != 0 and b"radius" in lib.lago_last_error()
        assert call(a, b, c, (1, 1, 1), mode=2) != 0 and b"mode" in lib.lago_last_error()
        assert call(a, b, c, (1, 1, 1), dim=4) != 0
        assert call(a, b, c, (1, 1, 1), dim=1) != 0
        assert call(a, b, c, None) != 0
        assert call(a, b, c, (1, 0, 0), tp=None) != 0 and b"taps" in lib.lago_last_error()
        assert call(a, a, c, (1, 1, 1)) != 0 and b"alias" in lib.lago_last_error()
        assert call(a, b, None, (1, 1, 0)) != 0 and b"scratch" in lib.lago_last_error()
        assert call(a, b, a, (1, 1, 0)) != 0 and b"scratch" in lib.lago_last_error()
        assert call(a, b, c, (1, 1, 1), ext=(0, 4, 4)) != 0
        assert call(a, b, c, (1, 1, 1), rows=0) == 0
        assert call(a, b, None, (1, 1, 1), rows=0, dim=2, ext=(4, 4, 1)) == 0


def test_argument_checks():
    import lagomorph_amd as lm

    ext = lm.lagomorph_ext
    x3, x2 = torch.zeros((1, 2, 4, 5, 6)), torch.zeros((1, 1, 4, 5))
    with pytest.raises(ValueError, match="FFT operator"):      # r = int(4 * 8.2 + 0.5) = 33
        lm.gaussian_smooth(x3, 8.2)
    with pytest.raises(ValueError, match="FFT operator"):
        lm.gaussian_smooth(x3, (1.0, 1.0, 11.0), truncate=3.0)
    with pytest.raises(ValueError, match="one per spatial axis"):
        lm.gaussian_smooth(x3, (1.0, 1.0))
    with pytest.raises(ValueError, match="one per spatial axis"):
        lm.gaussian_smooth(x2, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="unknown mode"):
        lm.gaussian_smooth(x3, 1.0, mode="reflect")
    with pytest.raises(ValueError, match="unknown mode"):
        lm.GaussianMetric([1.0], mode="nearest")
    with pytest.raises(ValueError, match="weight"):
        lm.GaussianMetric([1.0, 2.0], weights=[1.0])
    for x in (x3, x2):                                          # r = 32 is accepted and reaches the device check
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            lm.gaussian_smooth(x, 8.0)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            lm.gaussian_smooth(x, 0.0, mode="zero")
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ext.gaussian_smooth_forward(x3, [1, 0, 2], [lm.gaussian_taps(0.25), None, lm.gaussian_taps(0.5)], "wrap")
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        lm.GaussianMetric([1.0]).sharp(x3)
    with pytest.raises(ValueError, match="outside 0..32"):
        ext.gaussian_smooth_forward(x3, [33, 0, 0], [np.ones(67) / 67, None, None], "wrap")
    with pytest.raises(ValueError, match="taps"):
        ext.gaussian_smooth_forward(x3, [1, 0, 0], [np.ones(5) / 5, None, None], "wrap")
    with pytest.raises(ValueError, match="symmetric"):
        ext.gaussian_smooth_forward(x3, [1, 0, 0], [np.array([0.2, 0.5, 0.3]), None, None], "wrap")
    with pytest.raises(ValueError, match="one per spatial axis"):
        ext.gaussian_smooth_forward(x3, [1, 0], [None, None], "wrap")
    with pytest.raises(ValueError, match="unknown mode"):
        ext.gaussian_smooth_forward(x3, [0, 0, 0], [None] * 3, "clamp")
    with pytest.raises(RuntimeError, match="two- and three-dimensional"):
        lm.gaussian_smooth(torch.zeros((1, 1, 4)), 1.0)
    with pytest.raises(RuntimeError, match="float32 and float64"):
        ext.gaussian_smooth_forward(torch.zeros((1, 1, 4, 4), dtype=torch.int32), [0, 0], [None, None], "wrap")
    with pytest.raises(NotImplementedError, match="not a bounded operator"):
        lm.GaussianMetric([1.0]).flat(x3)


# ---- GaussianMetric's host logic, on CPU tensors: the oracle stands in for the geometry kernels, gauss_ref for the filter

@pytest.fixture
def ref_gauss(monkeypatch):
    import lagomorph_amd

    calls = []

    def forward(x, radii, taps, mode, alpha=1.0, out=None, accumulate=False):
        tl = [np.asarray(t, dtype=np.float64) if r > 0 else np.ones(1) for r, t in zip(radii, taps)]
        assert all(len(t) == 2 * r + 1 for r, t in zip(radii, tl))
        y = torch.from_numpy(alpha * gauss_ref.smooth_taps(x.detach().numpy(), tl, mode)).to(x.dtype)
        calls.append((tuple(radii), mode, alpha, accumulate))
        if out is None:
            assert not accumulate
            return y
        return out.add_(y) if accumulate else out.copy_(y)

    monkeypatch.setattr(lagomorph_amd.lagomorph_ext, "gaussian_smooth_forward", forward)
    return calls


def test_metric_sharp_is_the_weighted_sum(ref_gauss):
    import lagomorph_amd as lm

    m = torch.from_numpy(field((5, 6, 7), 4, nc=3))
    sig, wts = [1.0, (2.0, 0.0, 0.6), 0.5], [0.5, 2.0, -1.5]
    for mode in MODES:
        metric = lm.GaussianMetric(sig, weights=wts, mode=mode)
        for scale in (1.0, -0.25):
            want = scale * sum(w * gauss_ref.smooth(m.numpy(), s, mode=mode) for s, w in zip(sig, wts))
            got = metric.sharp(m, out_scale=scale) if scale != 1.0 else metric.sharp(m)
            assert rel(got.numpy(), want) <= 1e-14
    assert [c[3] for c in ref_gauss[:3]] == [False, True, True]     # the sum rides in the accumulate epilogue
    assert ref_gauss[1][0] == (8, 0, 2) and ref_gauss[0][2] == 0.5
    # default weights, one sigma, and the gradient: the operator is its own adjoint
    metric = lm.GaussianMetric([1.5])
    mm = m.clone().requires_grad_(True)
    go = torch.from_numpy(field((5, 6, 7), 5, nc=3))
    (metric.sharp(mm, out_scale=2.0) * go).sum().backward()
    assert rel(mm.grad.numpy(), 2.0 * gauss_ref.smooth(go.numpy(), 1.5)) <= 1e-14
    x = torch.from_numpy(field((5, 6, 7), 6)).requires_grad_(True)
    (lm.gaussian_smooth(x, (0.5, 1.0, 0.0), mode="zero") * go[:, :2]).sum().backward()
    assert rel(x.grad.numpy(), gauss_ref.smooth(go[:, :2].numpy(), (0.5, 1.0, 0.0), mode="zero")) <= 1e-14


@pytest.mark.parametrize("sp", [(6, 7, 8), (9, 10)])
def test_expmap_with_a_gaussian_metric_is_the_hand_written_loop(oracle_ext, ref_gauss, sp):
    import lagomorph_amd as lm

    d = len(sp)
    m0 = torch.from_numpy(0.5 * np.random.default_rng(8).standard_normal((2, d) + sp))
    sig, wts = [1.0, 2.0], [1.0, 0.5]
    metric = lm.GaussianMetric(sig, weights=wts)

    def sharp(m):
        return torch.from_numpy(sum(w * gauss_ref.smooth(m.numpy(), s) for s, w in zip(sig, wts)))

    steps, dt = 3, 1.0 / 3
    phi = torch.zeros_like(m0)
    for _ in range(steps):
        m = lm.Ad_star(phi, m0)
        phi = lm.compose_disp_vel(phi, sharp(m), dt=-dt)
    got = lm.expmap(metric, m0, num_steps=steps)
    assert got.shape == m0.shape and rel(got.numpy(), phi.numpy()) <= 1e-13
    assert rel(lm.expmap(metric, m0, num_steps=steps, phiinv=torch.zeros_like(m0)).numpy(), phi.numpy()) <= 1e-13
    assert float(got.abs().max()) > 1e-3
    # EPDiff_step and expmap_advect take it too
    one = lm.EPDiff_step(metric, m0, dt, torch.zeros_like(m0))
    assert rel(one.numpy(), (-dt * sharp(m0)).numpy()) <= 1e-13
    adv = lm.expmap_advect(metric, m0, num_steps=2)
    assert adv.shape == m0.shape and bool(torch.isfinite(adv).all())
    # gradients flow through the general branch
    mg = m0.clone().requires_grad_(True)
    lm.expmap(metric, mg, num_steps=2).pow(2).sum().backward()
    assert mg.grad is not None and bool(torch.isfinite(mg.grad).all()) and float(mg.grad.abs().max()) > 0
