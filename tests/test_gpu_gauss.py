"""GPU: gaussian_smooth (csrc/gauss.hip: gauss_z_kernel / gauss_s_kernel) and GaussianMetric.

Every result is judged against the float64 numpy reference tests/gauss_ref.py (held against scipy on the CPU,
tests/test_gauss_host.py) by the project's rule, unchanged: max|got - ref| <= RTOL x max|ref| with RTOL 1e-5 (float32)
and 1e-12 (float64).  The reference is computed once per (shape, sigma, mode) on the 3 x 3 field and shared: the
operator acts on every (n, c) plane on its own, so a smaller batch is judged against the reference's slices."""
import numpy as np
import pytest
import torch

import gauss_ref
from gpu_util import DTYPES, NPDT, SHAPES2, SHAPES3, dev, host, units_of
from parity_rule import rtol

pytestmark = pytest.mark.gpu

MODES = ["wrap", "zero"]
# after the lists of tests/gpu_util.py: shapes around the kernels' tile edges (64 positions of a strided axis per
# workgroup, 4 outputs per lane, rows of more than 128 voxels) and the smallest grid
EDGES = [(65, 3, 5), (4, 66, 3), (3, 4, 130), (33, 33, 33), (1, 1, 1)]


def sigma_sets(dim):
    """0.5 (r = 2); 2.5 (r = 10); 8.0 (r = 32, the cap); per-axis sets with zeros."""
    return [0.5, 2.5, 8.0, (0.0, 1.5, 0.7)[3 - dim:], (1.2, 0.0, 0.0)[:dim]]


@pytest.fixture(scope="module")
def lm():
    import lagomorph_amd

    lagomorph_amd.set_debug_mode(True)
    yield lagomorph_amd
    lagomorph_amd.set_debug_mode(False)


_FIELDS, _REFS = {}, {}


def field(sp, dtype, seed=0, nn=3, nc=3):
    """(nn, nc) + sp standard normal values, as a read-only array of `dtype`."""
    key = (sp, dtype, seed, nn, nc)
    if key not in _FIELDS:
        x = np.random.default_rng(abs(hash((sp, seed))) % 2**31).standard_normal((nn, nc) + sp).astype(NPDT[dtype])
        x.setflags(write=False)
        _FIELDS[key] = x
    return _FIELDS[key]


def reference(sp, dtype, sigma, mode, seed=0, nn=3, nc=3):
    key = (sp, dtype, str(sigma), mode, seed, nn, nc)
    if key not in _REFS:
        r = gauss_ref.smooth(field(sp, dtype, seed, nn, nc), sigma, mode=mode)
        r.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def same_values(a, b):
    """Equal element by element with NaN equal to NaN and -0 distinct from +0."""
    a, b = host(a), host(b)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) | np.isnan(a), np.signbit(b) | np.isnan(b))


# ---- 1. forward against the reference

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", SHAPES3 + SHAPES2 + EDGES)
def test_forward_against_the_reference(lm, dtype, sp):
    worst = 0.0
    for sigma in sigma_sets(len(sp)):
        for mode in MODES:
            ref = reference(sp, dtype, sigma, mode)
            for nn in (1, 3):
                for nc in (1, 3):
                    x = dev(field(sp, dtype)[:nn, :nc])
                    got = lm.gaussian_smooth(x, sigma, mode=mode)
                    assert got.dtype == dtype and got.shape == x.shape and got.is_contiguous()
                    u = units_of(got, ref[:nn, :nc], dtype)
                    worst = max(worst, u)
                    assert u <= 1.0, f"{sp} N={nn} C={nc} sigma={sigma} {mode}: {u:.3f} x RTOL x max|ref|"
    print(f"{sp} {dtype}: worst {worst:.3f} of the tolerance")


def test_truncate_is_honoured(lm):
    x = dev(field((9, 5, 70), torch.float32))
    got = lm.gaussian_smooth(x, 2.0, truncate=2.0, mode="zero")
    assert units_of(got, gauss_ref.smooth(host(x), 2.0, truncate=2.0, mode="zero"), torch.float32) <= 1.0
    assert units_of(got, reference((9, 5, 70), torch.float32, 2.0, "zero"), torch.float32) > 10.0   # truncate 4 differs


# ---- 2. copies, bits, empty batches, views

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9)])
def test_all_sigma_zero_returns_a_copy(lm, dtype, sp):
    x = dev(field(sp, dtype))
    for sigma in (0.0, -1.0, 0.1, (0.0,) * len(sp)):      # 0.1: the radius int(0.4 + 0.5) is 0
        for mode in MODES:
            y = lm.gaussian_smooth(x, sigma, mode=mode)
            assert torch.equal(y, x) and y.data_ptr() != x.data_ptr()
    y.zero_()
    assert float(x.abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_radius_zero_passes_copy_every_bit_pattern(lm, dtype):
    """inf, NaN and -0 come back as they are when no axis is filtered, also through alpha = 1 with `out` given; an axis
    with sigma 0 beside a filtered one does not spread them along itself."""
    x = dev(field((5, 6, 7), dtype)).clone()
    x[0, 0, 1, 2, 3], x[0, 1, 2, 2, 5], x[1, 0, 0, 0, 0], x[2, 2, 4, 5, 6] = float("inf"), float("nan"), -0.0, float("-inf")
    for mode in MODES:
        y = lm.gaussian_smooth(x, 0.0, mode=mode)
        assert same_values(y, x)
        out = torch.full_like(x, 7.0)
        lm.lagomorph_ext.gaussian_smooth_forward(x, [0, 0, 0], [None] * 3, mode, out=out)
        assert same_values(out, x)
        z = lm.gaussian_smooth(x, (0.0, 0.0, 0.5), mode=mode)        # only rows that hold a non-finite value lose it
        bad = ~torch.isfinite(x).all(dim=-1, keepdim=True).expand_as(x)
        assert bool(torch.isfinite(z[~bad]).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_rows_longer_than_one_segment(lm, dtype, mode):
    """nz above 1024: the z pass cuts a row into segments (a ragged last one), each with its own halo."""
    for sp, sigma in (((2, 3, 1030), (0.0, 0.0, 2.5)), ((2, 3, 2051), (0.7, 0.0, 8.0)), ((2, 1100), (1.0, 1.5))):
        x = dev(field(sp, dtype, nn=1, nc=2))
        ref = reference(sp, dtype, sigma, mode, nn=1, nc=2)
        u = units_of(lm.gaussian_smooth(x, sigma, mode=mode), ref, dtype)
        assert u <= 1.0, f"{sp} {sigma}: {u:.3f}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_pass_accumulate_without_an_in_place_pass(lm, dtype):
    """nz > 1024 with nx, ny above 64 (float32) / 32 (float64): no pass stages whole lines, the C entry point says so
    and the shim adds the term with torch instead."""
    ext = lm.lagomorph_ext
    sp = (65, 65, 1028) if dtype == torch.float32 else (33, 33, 1028)
    sigma, mode = (0.5, 0.7, 1.0), "wrap"
    x = dev(field(sp, dtype, nn=1, nc=1))
    out0 = field(sp, dtype, seed=1, nn=1, nc=1)
    ref = reference(sp, dtype, sigma, mode, nn=1, nc=1)
    radii = [gauss_ref.radius(s) for s in sigma]
    taps = [gauss_ref.taps(s) for s in sigma]
    got = ext.gaussian_smooth_forward(x, radii, taps, mode, alpha=-0.5)
    assert units_of(got, -0.5 * ref, dtype) <= 1.0
    out = dev(out0)
    res = ext.gaussian_smooth_forward(x, radii, taps, mode, alpha=-0.5, out=out, accumulate=True)
    assert res.data_ptr() == out.data_ptr()
    assert units_of(out, out0.astype(np.float64) - 0.5 * ref, dtype) <= 1.0
    assert torch.equal(out, dev(out0) + got)
    # the C entry point itself refuses the form
    import ctypes
    f = getattr(ctypes.CDLL(ext.LIB_PATH), "lago_gauss_smooth" + ("_f32" if dtype == torch.float32 else "_f64"))
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    half = (ctypes.c_double * 99)()
    for a, t in enumerate(taps):
        for k in range(radii[a] + 1):
            half[33 * a + k] = t[radii[a] + k]
    scratch, before = torch.empty_like(x), out.clone()
    rc = f(out.data_ptr(), x.data_ptr(), scratch.data_ptr(), (ctypes.c_int * 3)(*radii), half, 0, 1.0, 1, 3, 1, *sp, None)
    assert rc == -1 and torch.equal(out, before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_on_a_second_call_and_on_a_side_stream(lm, dtype):
    for sp, sigma in (((9, 5, 70), 2.5), ((33, 33, 33), (1.0, 2.0, 0.7)), ((3, 130), 1.5)):
        x = dev(field(sp, dtype))
        for mode in MODES:
            a = lm.gaussian_smooth(x, sigma, mode=mode)
            b = lm.gaussian_smooth(x, sigma, mode=mode)
            assert torch.equal(a, b)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                c = lm.gaussian_smooth(x, sigma, mode=mode)
            s.synchronize()
            assert torch.equal(a, c)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_batch(lm, dtype):
    for shape in ((0, 3, 5, 6, 7), (0, 1, 7, 9)):
        x = torch.zeros(shape, dtype=dtype, device="cuda")
        y = lm.gaussian_smooth(x, 1.0)
        assert y.shape == x.shape and y.dtype == dtype
    assert lm.GaussianMetric([1.0, 2.0]).sharp(torch.zeros((0, 3, 4, 4, 4), dtype=dtype, device="cuda")).shape == (0, 3, 4, 4, 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_contiguous_input(lm, dtype):
    sp, sigma = (6, 5, 16), (1.0, 0.7, 1.5)
    base = field(sp, dtype)                                # (3, 3, 6, 5, 16)
    for mode in MODES:
        ref = reference(sp, dtype, sigma, mode)
        x = dev(base)
        sl = x[:, 1:3]                                     # a channel slice
        assert not sl.is_contiguous()
        assert units_of(lm.gaussian_smooth(sl, sigma, mode=mode), ref[:, 1:3], dtype) <= 1.0
        pv = dev(base.transpose(0, 1, 4, 3, 2)).permute(0, 1, 4, 3, 2)   # a permuted view with the values of `base`
        assert not pv.is_contiguous() and torch.equal(pv, x)
        got = lm.gaussian_smooth(pv, sigma, mode=mode)
        assert got.is_contiguous() and units_of(got, ref, dtype) <= 1.0
        assert torch.equal(got, lm.gaussian_smooth(x, sigma, mode=mode))
        off = dev(np.concatenate([base.reshape(-1)[:1], base.reshape(-1)]))[1:].reshape(base.shape)   # 4 / 8 bytes off alignment
        assert torch.equal(lm.gaussian_smooth(off, sigma, mode=mode), got)


# ---- 3. alpha / accumulate epilogue

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", [(5, 6, 7), (9, 5, 70), (65, 3, 5), (3, 4, 130), (7, 9), (3, 130)])
def test_alpha_and_accumulate(lm, dtype, sp):
    ext = lm.lagomorph_ext
    x = dev(field(sp, dtype))
    out0 = field(sp, dtype, seed=1)
    dim = len(sp)
    for sigma in (2.5, (0.0, 1.5, 0.7)[3 - dim:], (1.2, 0.0, 0.0)[:dim], 0.0):
        sig = gauss_ref.per_axis(sigma, dim)
        radii = [gauss_ref.radius(s) for s in sig]
        taps = [gauss_ref.taps(s) for s in sig]
        for mode in MODES:
            ref = gauss_ref.smooth(field(sp, dtype), sigma, mode=mode) if sigma == 0.0 else reference(sp, dtype, sigma, mode)
            for alpha in (1.0, -0.375, 3.1):
                got = ext.gaussian_smooth_forward(x, radii, taps, mode, alpha=alpha)
                assert units_of(got, alpha * ref, dtype) <= 1.0
                assert units_of(lm.gaussian_smooth(x, sigma, mode=mode, alpha=alpha), alpha * ref, dtype) <= 1.0
                out = dev(out0)
                res = ext.gaussian_smooth_forward(x, radii, taps, mode, alpha=alpha, out=out, accumulate=True)
                assert res.data_ptr() == out.data_ptr()
                want = out0.astype(np.float64) + alpha * ref
                assert units_of(out, want, dtype) <= 1.0
                # the accumulated form adds the very term the plain form returns
                assert torch.equal(out, dev(out0) + got)
                out = dev(out0)                            # out given without accumulate: overwritten
                ext.gaussian_smooth_forward(x, radii, taps, mode, alpha=alpha, out=out)
                assert torch.equal(out, got)
    with pytest.raises(RuntimeError, match="overlap"):
        ext.gaussian_smooth_forward(x, radii, taps, "wrap", out=x)
    with pytest.raises(RuntimeError, match="accumulate needs out"):
        ext.gaussian_smooth_forward(x, radii, taps, "wrap", accumulate=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_metric_sharp_weights_and_out_scale(lm, dtype):
    sp = (9, 5, 70)
    x = dev(field(sp, dtype))
    sig, wts = [0.5, 2.5, (0.0, 1.5, 0.7)], [0.5, 2.0, -1.5]
    for mode in MODES:
        metric = lm.GaussianMetric(sig, weights=wts, mode=mode)
        want = sum(w * reference(sp, dtype, s, mode) for s, w in zip(sig, wts))
        assert units_of(metric.sharp(x), want, dtype) <= 1.0
        assert units_of(metric.sharp(x, out_scale=-0.2), -0.2 * want, dtype) <= 1.0
        ones = lm.GaussianMetric(sig[:2], mode=mode)
        assert units_of(ones.sharp(x), reference(sp, dtype, 0.5, mode) + reference(sp, dtype, 2.5, mode), dtype) <= 1.0


# ---- 4. adjoint and gradients

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", [(5, 6, 7), (9, 5, 70), (33, 33, 33), (3, 130), (2, 2)])
def test_operator_is_self_adjoint(lm, dtype, sp):
    """<G x, y> against <x, G y>, both sums in float64 on the host.  Each side carries at most RTOL x |x| |y| of error
    (|G x - ref| <= RTOL max|ref| per element is far inside RTOL |x| in norm for these fields), hence 2 RTOL |x| |y|."""
    x, y = field(sp, dtype, nn=2, nc=2), field(sp, dtype, seed=5, nn=2, nc=2)
    bound = 2 * rtol(dtype) * np.linalg.norm(x.astype(np.float64)) * np.linalg.norm(y.astype(np.float64))
    for sigma in sigma_sets(len(sp)):
        for mode in MODES:
            gx = host(lm.gaussian_smooth(dev(x), sigma, mode=mode)).astype(np.float64)
            gy = host(lm.gaussian_smooth(dev(y), sigma, mode=mode)).astype(np.float64)
            a, b = np.sum(gx * y.astype(np.float64)), np.sum(x.astype(np.float64) * gy)
            assert abs(a - b) <= bound, f"{sp} sigma={sigma} {mode}: {a} vs {b} (bound {bound:.3e})"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sp", [(4, 5, 6), (5, 7)])
def test_gradcheck_and_gradgradcheck(lm, sp, mode):
    x = dev(field(sp, torch.float64, nn=1, nc=2)).requires_grad_(True)
    sigma = (1.0, 0.6, 0.0)[:len(sp)]
    f = lambda t: lm.gaussian_smooth(t, sigma, mode=mode, alpha=1.5)
    assert torch.autograd.gradcheck(f, (x,), eps=1e-6, atol=1e-8, rtol=1e-6)
    assert torch.autograd.gradgradcheck(f, (x,), eps=1e-6, atol=1e-8, rtol=1e-6)
    metric = lm.GaussianMetric([0.6, sigma], weights=[1.0, 0.5], mode=mode)
    assert torch.autograd.gradcheck(lambda t: metric.sharp(t, out_scale=0.5), (x,), eps=1e-6, atol=1e-8, rtol=1e-6)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sp", [(9, 5, 70), (3, 130)])
def test_backward_is_the_reference_applied_to_the_gradient(lm, sp, mode):
    dtype = torch.float32
    sigma = (1.5, 0.7, 2.5)[3 - len(sp):]
    x = dev(field(sp, dtype)).requires_grad_(True)
    go = field(sp, dtype, seed=2)
    lm.gaussian_smooth(x, sigma, mode=mode).backward(dev(go))
    assert units_of(x.grad, reference(sp, dtype, sigma, mode, seed=2), dtype) <= 1.0


# ---- 5. graph capture

def test_graph_capture_of_two_calls(lm):
    """Two calls with different sigmas in one captured graph, replayed twice on new input: the bits of the eager calls.
    The taps of both calls must therefore live in the captured launches, not in host memory read at replay."""
    sp, dtype = (9, 5, 70), torch.float32
    lm.set_debug_mode(False)
    try:
        x = dev(field(sp, dtype))
        a = torch.empty_like(x)
        b = torch.empty_like(x)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):                             # warm-up: allocations happen outside the capture
                a.copy_(lm.gaussian_smooth(x, 0.5, mode="wrap"))
                b.copy_(lm.gaussian_smooth(x, (2.5, 1.0, 0.0), mode="zero"))
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            a.copy_(lm.gaussian_smooth(x, 0.5, mode="wrap"))
            b.copy_(lm.gaussian_smooth(x, (2.5, 1.0, 0.0), mode="zero"))
        for seed in (3, 4):
            x.copy_(dev(field(sp, dtype, seed=seed)))
            a.zero_()
            b.zero_()
            lm.gaussian_taps(7.0)                          # host work between replays must not matter
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(a, lm.gaussian_smooth(x, 0.5, mode="wrap"))
            assert torch.equal(b, lm.gaussian_smooth(x, (2.5, 1.0, 0.0), mode="zero"))
            assert units_of(b, reference(sp, dtype, (2.5, 1.0, 0.0), "zero", seed=seed), dtype) <= 1.0
    finally:
        lm.set_debug_mode(True)


# ---- 6. production sizes

def test_production_size_128_wrap(lm):
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((2, 1, 128, 128, 128), device="cuda", generator=g)
    got = lm.gaussian_smooth(x, 2.0, mode="wrap")
    assert units_of(got, gauss_ref.smooth(host(x), 2.0, mode="wrap"), torch.float32) <= 1.0


def test_production_size_160_192_160_zero(lm):
    g = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn((1, 1, 160, 192, 160), device="cuda", generator=g)
    got = lm.gaussian_smooth(x, (1.0, 2.0, 3.0), mode="zero")
    assert units_of(got, gauss_ref.smooth(host(x), (1.0, 2.0, 3.0), mode="zero"), torch.float32) <= 1.0


# ---- 7. GaussianMetric in use

def _momentum(dtype, seed=21):
    m = np.random.default_rng(seed).standard_normal((2, 3, 16, 16, 16))
    return dev((0.5 * gauss_ref.smooth(m, 2.0)).astype(NPDT[dtype]))     # smooth, about 0.05 in amplitude


def test_expmap_with_a_gaussian_metric_is_the_loop_over_the_public_ops(lm):
    m0 = _momentum(torch.float64)
    sig, wts = [1.0, 2.5], [1.0, 0.5]
    metric = lm.GaussianMetric(sig, weights=wts)

    def sharp(m):
        return lm.gaussian_smooth(m, sig[0], alpha=wts[0]) + lm.gaussian_smooth(m, sig[1], alpha=wts[1])

    steps, dt = 4, 0.25
    assert torch.equal(metric.sharp(m0), sharp(m0))
    phi = sharp(m0) * (-dt)
    for _ in range(steps - 1):
        phi = lm.compose_disp_vel(phi, sharp(lm.Ad_star(phi, m0)), dt=-dt)
    got = lm.expmap(metric, m0, num_steps=steps)
    assert torch.equal(got, phi) and float(got.abs().max()) > 1e-3
    # ... and the same through the branch that records a graph
    got = lm.expmap(metric, m0.clone().requires_grad_(True), num_steps=steps)
    assert torch.equal(got.detach(), phi)


def test_expmap_gradient_matches_a_central_difference(lm):
    m0 = _momentum(torch.float64).requires_grad_(True)
    metric = lm.GaussianMetric([1.0, 2.5], weights=[1.0, 0.5])
    w = dev(np.random.default_rng(22).standard_normal(m0.shape))

    def loss(m):
        return (lm.expmap(metric, m, num_steps=4) * w).sum()

    loss(m0).backward()
    assert bool(torch.isfinite(m0.grad).all()) and float(m0.grad.abs().max()) > 0
    d = dev(np.random.default_rng(23).standard_normal(m0.shape))
    d = d / d.norm()
    h = 1e-4
    with torch.no_grad():
        fd = float((loss(m0 + h * d) - loss(m0 - h * d)) / (2 * h))
    an = float((m0.grad * d).sum())
    print(f"analytic {an:.12e}, central difference {fd:.12e}")
    assert abs(an - fd) <= 1e-6 * abs(fd)


def test_lddmm_step_with_a_gaussian_metric_lowers_the_image_term(lm):
    sp = (16, 16, 16)
    g = np.indices(sp).astype(np.float64)
    blob = lambda c: np.exp(-sum((g[a] - c[a]) ** 2 for a in range(3)) / (2 * 3.0 ** 2))
    I = dev(blob((8, 8, 8))[None, None].astype(np.float32))
    img = dev(np.stack([blob((9, 8, 7)), blob((7, 9, 8))])[:, None].astype(np.float32))
    metric = lm.GaussianMetric([1.5, 3.0], weights=[1.0, 0.5])
    m = torch.zeros((2, 3) + sp, device="cuda")

    def image_term(mm):
        with torch.no_grad():
            return float(torch.nn.functional.mse_loss(lm.interp(I, lm.expmap(metric, mm, num_steps=3)), img, reduction="sum")) / img.numel()

    before = image_term(m)
    m, loss1, reg1 = lm.lddmm_step(I, m, img, metric, dataset_size=2, integration_steps=3, reg_weight=1e-2, learning_rate_pose=2e2)
    m, loss2, reg2 = lm.lddmm_step(I, m, img, metric, dataset_size=2, integration_steps=3, reg_weight=1e-2, learning_rate_pose=2e2)
    img2 = float(loss2) - float(reg2)
    img1 = float(loss1) - float(reg1)
    print(f"image term: {before:.6e} at m = 0, first call {img1:.6e}, second call {img2:.6e}; after two steps {image_term(m):.6e}")
    assert abs(img1 - before) <= 1e-5 * before
    assert img2 < img1 and bool(torch.isfinite(m).all()) and float(m.abs().max()) > 0
    with pytest.raises(NotImplementedError):
        lm.lddmm_step(I, m, img, metric, dataset_size=2, integration_steps=3, momentum_preconditioning=True)
