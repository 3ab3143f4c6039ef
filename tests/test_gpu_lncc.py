"""GPU: lncc (csrc/lncc.hip: lncc_moments_kernel, lncc_cc_kernel, lncc_coeff_kernel, lncc_combine_kernel on the passes of
csrc/gauss.hip), its backward, lncc_loss, LNCCSimilarity and the `similarity` argument of lddmm_step.

Every result is judged against the float64 numpy reference tests/lncc_ref.py (held against central differences on the
CPU, tests/test_lncc_host.py) by the project's rule, unchanged: max|got - ref| <= RTOL x max|ref| with RTOL 1e-5
(float32) and 1e-12 (float64), separately for cc, dI and dJ.  The cases (shapes, the three kinds of J, the sigmas each
kind goes with) are lncc_ref's; their inputs are float32 values, so both precisions share one reference per case."""
import numpy as np
import pytest
import torch

import lncc_ref
from gpu_util import DTYPES, NPDT, dev, host, units_of
from parity_rule import rtol

pytestmark = pytest.mark.gpu

MODES = lncc_ref.MODES


@pytest.fixture(scope="module")
def lm():
    import lagomorph_amd

    lagomorph_amd.set_debug_mode(True)
    yield lagomorph_amd
    lagomorph_amd.set_debug_mode(False)


def case(sp, kind, dtype, grad=True):
    I, J, g = (dev(a, dtype) for a in lncc_ref.inputs(sp, kind))
    return I.requires_grad_(grad), J.requires_grad_(grad), g


def normal(shape, seed, dtype=torch.float32):
    return torch.randn(shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(seed))


# ---- 1. cc, dI and dJ against the reference

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", lncc_ref.SHAPES)
def test_forward_and_backward_against_the_reference(lm, dtype, sp):
    worst = [0.0, 0.0, 0.0]
    for kind in lncc_ref.KINDS:
        I, J, g = case(sp, kind, dtype)
        for sigma in lncc_ref.sigmas_of(sp, kind):
            for mode in MODES:
                ref = lncc_ref.reference(sp, kind, sigma, mode)
                cc = lm.lncc(I, J, sigma, mode=mode)
                assert cc.dtype == dtype and cc.shape == I.shape and cc.is_contiguous()
                dI, dJ = torch.autograd.grad(cc, (I, J), g)
                u = [units_of(a, b, dtype) for a, b in zip((cc, dI, dJ), ref)]
                print(f"{sp} {kind} sigma={sigma} {mode} {dtype}: cc {u[0]:.3f} dI {u[1]:.3f} dJ {u[2]:.3f} x RTOL x max|ref|")
                worst = [max(a, b) for a, b in zip(worst, u)]
                assert max(u) <= 1.0, f"{sp} {kind} sigma={sigma} {mode}: cc, dI, dJ at {u} x RTOL x max|ref|"
    print(f"{sp} {dtype}: worst cc {worst[0]:.3f} dI {worst[1]:.3f} dJ {worst[2]:.3f} of the tolerance")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_gradient_alone_is_the_same_bits(lm, dtype):
    """The three-field coefficient kernels (one input needs a gradient) against the five-field one."""
    sp, sigma = (9, 5, 70), 1.0
    for mode in MODES:
        I, J, g = case(sp, "corr", dtype)
        dI, dJ = torch.autograd.grad(lm.lncc(I, J, sigma, mode=mode), (I, J), g)
        (oI,) = torch.autograd.grad(lm.lncc(I, J.detach(), sigma, mode=mode), (I,), g)
        (oJ,) = torch.autograd.grad(lm.lncc(I.detach(), J, sigma, mode=mode), (J,), g)
        assert torch.equal(oI, dI) and torch.equal(oJ, dJ)
        ref = lncc_ref.reference(sp, "corr", sigma, mode)
        assert units_of(oI, ref[1], dtype) <= 1.0 and units_of(oJ, ref[2], dtype) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_truncate_and_eps_are_honoured(lm, dtype):
    sp = (9, 5, 70)
    I, J, g = case(sp, "corr", dtype, grad=False)
    Ih, Jh, _ = lncc_ref.inputs(sp, "corr")
    got = lm.lncc(I, J, 2.0, truncate=2.0, mode="zero", eps=1e-2)
    assert units_of(got, lncc_ref.lncc(Ih, Jh, 2.0, truncate=2.0, mode="zero", eps=1e-2), dtype) <= 1.0
    assert units_of(got, lncc_ref.lncc(Ih, Jh, 2.0, truncate=2.0, mode="zero"), dtype) > 10.0
    assert units_of(got, lncc_ref.lncc(Ih, Jh, 2.0, mode="zero", eps=1e-2), dtype) > 10.0


# ---- 2. symmetry, self-match, contrast invariance

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", [(5, 6, 7), (9, 5, 70), (3, 130)])
def test_symmetry_and_self_match(lm, dtype, sp):
    for kind in ("corr", "indep"):
        I, J, g = case(sp, kind, dtype)
        Ih = lncc_ref.inputs(sp, kind)[0]
        for sigma in (1.0, lncc_ref.per_axis_set(len(sp))):
            for mode in MODES:
                a, b = lm.lncc(I, J, sigma, mode=mode), lm.lncc(J, I, sigma, mode=mode)
                assert torch.equal(a, b)
                aI, aJ = torch.autograd.grad(a, (I, J), g)
                bJ, bI = torch.autograd.grad(b, (J, I), g)
                assert torch.equal(aI, bI) and torch.equal(aJ, bJ)
                # against itself sX = sI = sJ: sI^2 / (sI^2 + eps), which is what the reference evaluates
                own = lm.lncc(I, I, sigma, mode=mode)
                assert units_of(own, lncc_ref.lncc(Ih, Ih, sigma, mode=mode), dtype) <= 1.0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sp", [(5, 6, 7), (9, 5, 70), (7, 9)])
def test_contrast_invariance_in_float64(lm, sp, mode):
    """eps = 0: cc(-2.5 I + 3, J) = cc(I, J) with the periodic border, where the taps of every window sum to one, so an
    offset drops out of sI and sX.  Rounding is 1e-16, the offset costs about a digit (mean square 9 + 6 against a variance
    of 6) and the smallest window variance of these cases three to four more: 1e-10 x max.  At a zero border the windows
    near it hold less than the full weight, C - A^2 is no variance there and an offset does not cancel (0.68 of max was
    measured on (5, 6, 7)): that mode is invariant to the scaling alone, which is what is asserted for it."""
    I, J, _ = case(sp, "corr", torch.float64, grad=False)
    other = -2.5 * I + 3.0 if mode == "wrap" else -2.5 * I
    for sigma in (1.0, 2.5):
        a = lm.lncc(I, J, sigma, mode=mode, eps=0.0)
        b = lm.lncc(other, J, sigma, mode=mode, eps=0.0)
        err = float((a - b).abs().max()) / float(a.abs().max())
        print(f"{sp} sigma={sigma} {mode}: {err:.3e}")
        assert err <= 1e-10


# ---- 3. gradients

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sp", [(4, 5, 6), (5, 7)])
def test_gradcheck(lm, sp, mode):
    I = normal((1, 2) + sp, 31, torch.float64)
    J = 0.8 * I + 0.6 * normal((1, 2) + sp, 32, torch.float64)
    sigma = (1.0, 0.0, 0.7)[:len(sp)] if len(sp) == 3 else (1.0, 0.7)
    f = lambda a, b: lm.lncc(a, b, sigma, mode=mode)
    kw = dict(eps=1e-6, atol=1e-8, rtol=1e-6)
    Ig, Jg = I.clone().requires_grad_(True), J.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: f(a, J), (Ig,), **kw)
    assert torch.autograd.gradcheck(lambda b: f(I, b), (Jg,), **kw)
    assert torch.autograd.gradcheck(f, (Ig, Jg), **kw)
    assert torch.autograd.gradcheck(lambda a, b: lm.lncc_loss(a, b, 1.0, mode=mode, reduction="sum"), (Ig, Jg), **kw)


# ---- 4. bits and stability

def _all(lm, I, J, g, sigma, mode):
    I, J = I.detach().requires_grad_(True), J.detach().requires_grad_(True)
    cc = lm.lncc(I, J, sigma, mode=mode)
    return (cc.detach(),) + torch.autograd.grad(cc, (I, J), g)


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_on_a_second_call_and_on_a_side_stream(lm, dtype):
    for sp, sigma in (((9, 5, 70), 2.5), ((33, 33, 33), (1.0, 2.0, 0.7)), ((3, 130), 1.5)):
        I, J, g = case(sp, "corr", dtype)
        for mode in MODES:
            a = _all(lm, I, J, g, sigma, mode)
            b = _all(lm, I, J, g, sigma, mode)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                c = _all(lm, I, J, g, sigma, mode)
            s.synchronize()
            for x, y, z in zip(a, b, c):
                assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_contiguous_and_misaligned_input(lm, dtype):
    sp, sigma = (6, 5, 16), (1.0, 0.7, 1.5)
    Ih, Jh, gh = (a.astype(NPDT[dtype]) for a in lncc_ref.inputs(sp, "corr"))
    I, J, g = dev(Ih), dev(Jh), dev(gh)
    for mode in MODES:
        want = _all(lm, I, J, g, sigma, mode)
        pI, pJ, pg = (dev(a.transpose(0, 1, 4, 3, 2)).permute(0, 1, 4, 3, 2) for a in (Ih, Jh, gh))   # permuted views
        assert not pI.is_contiguous() and torch.equal(pI, I)
        got = _all(lm, pI, pJ, pg, sigma, mode)
        assert all(x.is_contiguous() and torch.equal(x, y) for x, y in zip(got, want))
        sl = _all(lm, I[:, 1:], J[:, 1:], g[:, 1:], sigma, mode)                                       # a channel slice
        assert not I[:, 1:].is_contiguous() and all(torch.equal(x, y[:, 1:]) for x, y in zip(sl, want))
        # one element (4 / 8 bytes) off the alignment of the vector loads and stores
        oI, oJ, og = (dev(np.concatenate([a.reshape(-1)[:1], a.reshape(-1)]))[1:].reshape(a.shape) for a in (Ih, Jh, gh))
        assert oI.data_ptr() % 16 != 0
        off = _all(lm, oI, oJ, og, sigma, mode)
        assert all(torch.equal(x, y) for x, y in zip(off, want))


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_batch(lm, dtype):
    for shape in ((0, 3, 5, 6, 7), (0, 1, 7, 9)):
        I = torch.zeros(shape, dtype=dtype, device="cuda", requires_grad=True)
        J = torch.zeros(shape, dtype=dtype, device="cuda", requires_grad=True)
        cc = lm.lncc(I, J, 1.0)
        assert cc.shape == I.shape and cc.dtype == dtype
        dI, dJ = torch.autograd.grad(cc, (I, J), torch.zeros_like(cc))
        assert dI.shape == I.shape and dJ.shape == J.shape
        assert lm.lncc_loss(I, J, 1.0, reduction="none").shape == I.shape
        assert float(lm.lncc_loss(I.detach(), J.detach(), 1.0, reduction="sum")) == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_longer_than_one_segment(lm, dtype):
    """nz above 1024: the moments pass cuts a row into segments (a ragged last one), each with its own halo."""
    sp, sigma, mode = (2, 3, 1030), (0.0, 1.0, 2.5), "wrap"
    Ih, Jh, gh = lncc_ref.inputs(sp, "corr", nn=1, nc=2)
    I, J, g = (dev(a, dtype) for a in (Ih, Jh, gh))
    got = _all(lm, I, J, g, sigma, mode)
    ref = lncc_ref.lncc_with_grads(Ih, Jh, gh, sigma, mode=mode)
    u = [units_of(a, b, dtype) for a, b in zip(got, ref)]
    assert max(u) <= 1.0, u


# ---- 4b. the moments pass IS the z pass of gaussian_smooth (csrc/gauss.hpp: gauss_z_pass, two instantiations)

def _taps(lm, radii):
    """Per axis the 2 r + 1 taps of radius r (sigma = r / 4 at truncate 4 gives exactly r; [1.] for r = 0)."""
    taps = [lm.gaussian_taps(r / 4.0) for r in radii]
    assert [(len(t) - 1) // 2 for t in taps] == list(radii)
    return taps


def _off_by_one(t):
    """The values of t in a contiguous view whose storage starts one element (4 / 8 bytes) off the vector alignment."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_z_only_moments_are_the_z_pass_of_gaussian_smooth(lm, dtype, mode):
    """Radii 0 on the other axes: moments[0] and moments[1] are gaussian_smooth_forward of I and J, bit for bit.  The
    shapes: a short last 4-group with masked scalar stores; vector stores; two segments with the halo across the segment
    edge; 32 rows per workgroup with a ragged last row block; 2D.  Radii 1, 4, 9 are H = 4, 4, 12, and 9 on extent 7
    wraps more than once.  Each case also runs on inputs one element off the vector alignment, with gaussian_smooth
    writing into an `out` that is off as well (its scalar stores; the moments tensor is always allocated aligned, so the
    scalar stores of that kernel are those of the extent 7 case)."""
    from lagomorph_amd import lagomorph_ext as ext

    for n, shape in enumerate(((1, 2, 3, 5, 7), (2, 1, 2, 3, 64), (1, 1, 2, 2, 1030), (1, 33, 1, 1, 8), (1, 1, 6, 9))):
        I, J = normal(shape, 60 + 2 * n, dtype), normal(shape, 61 + 2 * n, dtype)
        for r in (1, 4, 9):
            radii = [0] * (len(shape) - 3) + [r]
            taps = _taps(lm, radii)
            want = [ext.gaussian_smooth_forward(x, radii, taps, mode) for x in (I, J)]
            mom = ext.lncc_moments(I, J, radii, taps, mode)
            assert mom.shape == (5,) + shape
            assert torch.equal(mom[0], want[0]) and torch.equal(mom[1], want[1]), (shape, r)
            oI, oJ = _off_by_one(I), _off_by_one(J)
            off = ext.lncc_moments(oI, oJ, radii, taps, mode)
            assert torch.equal(off, mom), (shape, r)
            for x, w in zip((oI, oJ), want):
                out = _off_by_one(torch.zeros_like(x))
                assert ext.gaussian_smooth_forward(x, radii, taps, mode, out=out) is out
                assert torch.equal(out, w), (shape, r)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_moments_then_x_and_y_are_gaussian_smooth_of_the_products(lm, dtype, mode):
    """z radius 0, x and / or y filtered: the copy pass rounds each exact double product once and both paths then run x
    before y, so all five moments are gaussian_smooth_forward of I, J and the products formed the same way.  70 > 64 gives
    two axis tiles in float32."""
    from lagomorph_amd import lagomorph_ext as ext

    for n, shape in enumerate(((1, 2, 5, 6, 7), (1, 1, 70, 3, 8))):
        I, J = normal(shape, 80 + 2 * n, dtype), normal(shape, 81 + 2 * n, dtype)
        a, b = I.double(), J.double()
        fields = (I, J, (a * a).to(dtype), (a * b).to(dtype), (b * b).to(dtype))
        for radii in ((2, 0, 0), (0, 3, 0), (2, 3, 0)):
            taps = _taps(lm, radii)
            mom = ext.lncc_moments(I, J, list(radii), taps, mode)
            for m, x in enumerate(fields):
                assert torch.equal(mom[m], ext.gaussian_smooth_forward(x, list(radii), taps, mode)), (shape, radii, m)


# ---- 5. graph capture

def test_graph_capture_of_forward_and_backward(lm):
    """Forward and backward of two calls with different sigmas in one captured graph, replayed on new data: the bits of
    the eager calls.  The taps must therefore live in the captured launches, not in host memory read at replay."""
    sp, dtype = (9, 5, 70), torch.float32
    calls = ((0.5, "wrap"), ((2.5, 1.0, 0.0), "zero"))
    lm.set_debug_mode(False)
    try:
        I, J, g = case(sp, "corr", dtype)
        outs = [[torch.empty_like(I.detach()) for _ in range(3)] for _ in calls]

        def work():
            for (sigma, mode), o in zip(calls, outs):
                cc = lm.lncc(I, J, sigma, mode=mode)
                dI, dJ = torch.autograd.grad(cc, (I, J), g)
                for dst, src in zip(o, (cc.detach(), dI, dJ)):
                    dst.copy_(src)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):                             # warm-up: allocations happen outside the capture
                work()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            work()
        for kind in ("indep", "affine"):
            nI, nJ, ng = lncc_ref.inputs(sp, kind)
            with torch.no_grad():
                I.copy_(dev(nI, dtype))
                J.copy_(dev(nJ, dtype))
                g.copy_(dev(ng, dtype))
            for o in outs:
                for t in o:
                    t.zero_()
            lm.gaussian_taps(7.0)                          # host work between replays must not matter
            graph.replay()
            torch.cuda.synchronize()
            for (sigma, mode), o in zip(calls, outs):
                eager = _all(lm, I, J, g, sigma, mode)
                assert all(torch.equal(x, y) for x, y in zip(o, eager))
            if kind == "indep":
                ref = lncc_ref.reference(sp, "indep", 0.5, "wrap")
                assert max(units_of(a, b, dtype) for a, b in zip(outs[0], ref)) <= 1.0
    finally:
        lm.set_debug_mode(True)


# ---- 6. lncc_loss, LNCCSimilarity

@pytest.mark.parametrize("dtype", DTYPES)
def test_loss_reductions(lm, dtype):
    sp, sigma = (5, 6, 7), 1.0
    I, J, _ = case(sp, "corr", dtype, grad=False)
    cc = lm.lncc(I, J, sigma, mode="zero")
    none = lm.lncc_loss(I, J, sigma, mode="zero", reduction="none")
    assert torch.equal(none, 1.0 - cc)
    assert torch.equal(lm.lncc_loss(I, J, sigma, mode="zero", reduction="sum"), none.sum())
    assert torch.equal(lm.lncc_loss(I, J, sigma, mode="zero"), none.mean())
    assert torch.equal(lm.LNCCSimilarity(sigma, mode="zero")(I, J), none.sum())
    ref = lncc_ref.reference(sp, "corr", sigma, "zero")[0]
    assert abs(float(lm.lncc_loss(I, J, sigma, mode="zero")) - (1.0 - ref.mean())) <= rtol(dtype) * 10
    # the gradient of the mean: -dI / numel with g = 1
    Ig = I.clone().requires_grad_(True)
    lm.lncc_loss(Ig, J, sigma, mode="zero").backward()
    ones = np.ones(I.shape)
    want = -lncc_ref.lncc_with_grads(*lncc_ref.inputs(sp, "corr")[:2], ones, sigma, mode="zero")[1] / I.numel()
    assert units_of(Ig.grad, want, dtype) <= 1.0


# ---- 7. the matching step

def _blobs():
    sp = (16, 16, 16)
    g = np.indices(sp).astype(np.float64)
    blob = lambda c: np.exp(-sum((g[a] - c[a]) ** 2 for a in range(3)) / (2 * 3.0 ** 2))
    I = dev(blob((8, 8, 8))[None, None].astype(np.float32))
    targets = np.stack([blob((9, 8, 7)), blob((7, 9, 8))])[:, None].astype(np.float32)
    return sp, I, targets


def test_lddmm_step_with_the_squared_difference_as_similarity_is_the_default_call(lm):
    """`similarity=sse` runs the very kernels of the default call.  loss and reg come from gathers alone and are compared
    bit for bit.  m and I.grad pass through splats whose float atomics add in arrival order, so the DEFAULT call does not
    repeat its own bits in them on the device (measured here, two default calls with the fluid metric: max difference
    3.0e-8 in m at max|m| 0.2, 6.7e-8 in I.grad; with the Gaussian metric 2.3e-10 between two `similarity` calls): there
    are no "bits of the default call" to hold them to, and they are judged by the project's float32 rule,
    max|a - b| <= 1e-5 max|b|.  The bit-for-bit statement for m and I.grad is made where the step is reproducible, on the
    CPU through the oracle (tests/test_lncc_host.py: test_lddmm_step_takes_a_similarity)."""
    sp, I, targets = _blobs()
    img = dev(targets)
    sse = lambda a, b: torch.nn.functional.mse_loss(a, b, reduction="sum")
    for metric in (lm.FluidMetric([0.1, 0.0, 0.01]), lm.GaussianMetric([1.5, 3.0], weights=[1.0, 0.5])):   # fused and plain step
        res = []
        for sim in (None, sse):
            Ia = I.clone().requires_grad_(True)
            m = 0.05 * normal((2, 3) + sp, 41)
            m, loss, reg = lm.lddmm_step(Ia, m, img, metric, dataset_size=2, integration_steps=3, reg_weight=1e-2,
                                         learning_rate_pose=2e2, similarity=sim)
            res.append((m.detach().clone(), loss.detach().clone(), reg.detach().clone(), Ia.grad.clone()))
        (m0, loss0, reg0, g0), (m1, loss1, reg1, g1) = res
        assert torch.equal(loss0, loss1) and torch.equal(reg0, reg1)
        um, ug = units_of(m1, host(m0), torch.float32), units_of(g1, host(g0), torch.float32)
        print(f"{type(metric).__name__}: m {um:.4f}, I.grad {ug:.4f} x 1e-5 x max|default|")
        assert um <= 1.0 and ug <= 1.0
        assert float(m0.abs().max()) > 0 and float(g0.abs().max()) > 0 and float(loss0) > float(reg0) > 0


def test_lddmm_step_with_lncc_matches_intensity_inverted_targets(lm):
    """Targets 1 - 2 blob: the squared difference cannot match them to the blob atlas, the correlation can.  Two steps
    lower 1 - mean cc of the deformed atlas against the targets."""
    sp, I, targets = _blobs()
    img = dev(1.0 - 2.0 * targets)
    metric = lm.GaussianMetric([1.5, 3.0], weights=[1.0, 0.5])
    sim = lm.LNCCSimilarity(2.0)
    m = torch.zeros((2, 3) + sp, device="cuda")

    def term(mm):
        with torch.no_grad():
            return float(lm.lncc_loss(lm.interp(I, lm.expmap(metric, mm, num_steps=3)), img, 2.0))

    before = term(m)
    kw = dict(dataset_size=2, integration_steps=3, reg_weight=1e-2, learning_rate_pose=2e2, similarity=sim)
    m, loss1, reg1 = lm.lddmm_step(I, m, img, metric, **kw)
    m, loss2, reg2 = lm.lddmm_step(I, m, img, metric, **kw)
    after = term(m)
    img1, img2 = float(loss1) - float(reg1), float(loss2) - float(reg2)
    print(f"1 - mean cc: {before:.6e} at m = 0, first call {img1:.6e}, second call {img2:.6e}; after two steps {after:.6e}")
    assert abs(img1 - before) <= 1e-5 * before          # the step's image term IS (1 - cc).sum() / numel
    assert after < before and img2 < img1
    assert bool(torch.isfinite(m).all()) and float(m.abs().max()) > 0


def test_atlas_builder_takes_a_similarity(lm):
    sp, I, targets = _blobs()
    images = dev(1.0 - 2.0 * targets)
    sim = lm.LNCCSimilarity(2.0)
    b = lm.LDDMMAtlasBuilder(images, batch_size=2, lddmm_integration_steps=2, reg_weight=1e-2, I0=I[0],
                             metric=lm.GaussianMetric([1.5, 3.0], weights=[1.0, 0.5]), similarity=sim)
    assert b.similarity is sim and lm.LDDMMAtlasBuilder(images, batch_size=2).similarity is None
    before = float(lm.lncc_loss(b.I.detach().expand(2, -1, -1, -1, -1).contiguous(), images, 2.0))
    loss, reg = b.iteration(0, last_of_epoch=True)
    assert abs((float(loss) - float(reg)) - before) <= 1e-5 * before
    assert bool(torch.isfinite(b.ms[0]).all()) and float(b.ms[0].abs().max()) > 0 and bool(torch.isfinite(b.I).all())


# ---- 8. production sizes

def _production(lm, shape, sigma, mode, seed):
    I = normal(shape, seed)
    J = 0.8 * I + 0.6 * normal(shape, seed + 1)
    g = normal(shape, seed + 2)
    got = _all(lm, I, J, g, sigma, mode)
    ref = lncc_ref.lncc_with_grads(host(I), host(J), host(g), sigma, mode=mode)
    u = [units_of(a, b, torch.float32) for a, b in zip(got, ref)]
    print(f"{shape} sigma={sigma} {mode}: cc {u[0]:.3f} dI {u[1]:.3f} dJ {u[2]:.3f} x RTOL x max|ref|")
    assert max(u) <= 1.0, u


def test_production_size_128(lm):
    _production(lm, (2, 1, 128, 128, 128), 2.0, "wrap", 51)


def test_production_size_160_192_160(lm):
    _production(lm, (1, 1, 160, 192, 160), 2.0, "zero", 54)
