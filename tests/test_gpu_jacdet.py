"""GPU: jacobian_determinant (csrc/diff.hip: jacdet_fwd_kernel / jacdet_bwd_kernel) against the test-side reference
built from the CPU oracle (tests/jacdet_ref.py).  Forward bit for bit; backward within the project's tolerance
(RTOL x max|reference|, no multipliers, as tests/test_gpu_parity.py) and bit-identical from call to call."""
import functools
import os

import numpy as np
import pytest
import torch

import gpu_util
import jacdet_ref
from gpu_util import DTYPES, SHAPES2, SHAPES3, assert_bits, dev, host, rnd, smooth_field
from oracle import lago_oracle as orc

pytestmark = pytest.mark.gpu
assert_close = functools.partial(gpu_util.assert_close, record=False, show=True)   # prints the units, stays out of LAGO_TOL_REPORT


@pytest.fixture(scope="module")
def lm():
    import lagomorph_amd

    lagomorph_amd.set_debug_mode(True)
    yield lagomorph_amd
    lagomorph_amd.set_debug_mode(False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", SHAPES3 + SHAPES2)
def test_forward_bits_backward_tolerance(lm, dtype, sp):
    ext = lm.lagomorph_ext
    for nn in (1, 2, 3):
        for scale in (0.3, 3.0):
            rng = np.random.default_rng(abs(hash((sp, nn, scale))) % 2**31)
            u = rnd(rng, (nn, len(sp)) + sp, dtype, scale)
            go = rnd(rng, (nn, 1) + sp, dtype)
            for disp in (True, False):
                what = f"{sp} N={nn} scale={scale} displacement={disp}"
                assert_bits(ext.jacobian_determinant_forward(dev(u), disp), jacdet_ref.forward(u, disp), "forward " + what)
                d1 = ext.jacobian_determinant_backward(dev(go), dev(u), disp)
                assert_close(d1, jacdet_ref.backward(go, u, disp), dtype, "backward " + what)
                d2 = ext.jacobian_determinant_backward(dev(go), dev(u), disp)
                assert torch.equal(d1, d2), "backward differs between two calls: " + what


def _oracle_threads():
    return min(os.cpu_count() or 1, 64)


@pytest.mark.parametrize("N,S", [(8, 128), (2, 160)])
def test_production_geometry(lm, N, S):
    """8 x 3 x 128^3 and 2 x 3 x 160^3 float32, a smooth displacement of about 3 voxels amplitude."""
    ext = lm.lagomorph_ext
    u = smooth_field((N, 3, S, S, S), 8.0, 100 + S, 3.0)
    g = torch.Generator(device="cuda").manual_seed(S)
    go = torch.randn((N, 1, S, S, S), device="cuda", generator=g)
    out = ext.jacobian_determinant_forward(u, True)
    d_u = ext.jacobian_determinant_backward(go, u, True)
    assert torch.equal(d_u, ext.jacobian_determinant_backward(go, u, True))
    un, gon = host(u), host(go)
    orc.set_threads(_oracle_threads())
    try:
        want = jacdet_ref.forward(un, True)
        wantb = jacdet_ref.backward(gon, un, True)
    finally:
        orc.set_threads(1)
    assert_bits(out, want, f"forward {N} x 3 x {S}^3")
    assert_close(d_u, wantb, torch.float32, f"backward {N} x 3 x {S}^3")
    assert float(want.min()) < 1.0 < float(want.max())


@pytest.mark.parametrize("disp", [True, False])
@pytest.mark.parametrize("shape", [(1, 2, 4, 5), (2, 3, 3, 4, 3)])
def test_gradcheck(lm, shape, disp):
    g = torch.Generator(device="cuda").manual_seed(7)
    u = torch.randn(shape, device="cuda", dtype=torch.float64, generator=g).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: lm.jacobian_determinant(x, disp), (u,))


def test_autograd_function(lm):
    rng = np.random.default_rng(3)
    u = rnd(rng, (2, 3, 6, 5, 9), torch.float32, 0.5)
    go = rnd(rng, (2, 1, 6, 5, 9), torch.float32)
    ut = dev(u).requires_grad_(True)
    out = lm.jacobian_determinant(ut)   # displacement=True is the default
    assert out.shape == (2, 1, 6, 5, 9)
    assert_bits(out, jacdet_ref.forward(u, True), "jacobian_determinant")
    out.backward(dev(go))
    assert_close(ut.grad, jacdet_ref.backward(go, u, True), torch.float32, "jacobian_determinant backward")
    (lm.jacobian_determinant(ut, False) * dev(go)).sum().backward()   # the flag takes no gradient


def test_zero_field_is_exactly_one(lm):
    for shape in [(2, 3, 9, 10, 11), (2, 2, 12, 13)]:
        for dtype in DTYPES:
            u = torch.zeros(shape, device="cuda", dtype=dtype)
            one = lm.jacobian_determinant(u)
            assert torch.equal(one, torch.ones_like(one))
            assert torch.equal(lm.jacobian_determinant(u, False), torch.zeros_like(one))


def test_noncontiguous_stream_empty_and_errors(lm):
    ext = lm.lagomorph_ext
    rng = np.random.default_rng(4)
    base = rnd(rng, (2, 6, 7, 8, 3), torch.float32, 0.7)
    u_nc = dev(base).permute(0, 4, 1, 2, 3)
    assert not u_nc.is_contiguous()
    un = np.ascontiguousarray(base.transpose(0, 4, 1, 2, 3))
    go = rnd(rng, (2, 1, 6, 7, 8), torch.float32)
    go_nc = dev(go.transpose(0, 1, 4, 3, 2)).permute(0, 1, 4, 3, 2)
    assert not go_nc.is_contiguous()
    assert_bits(ext.jacobian_determinant_forward(u_nc, True), jacdet_ref.forward(un, True), "non-contiguous forward")
    assert_close(ext.jacobian_determinant_backward(go_nc, u_nc, True), jacdet_ref.backward(go, un, True), torch.float32,
                 "non-contiguous backward")
    # a non-default stream
    u, g = dev(un), dev(go)
    ref_f, ref_b = ext.jacobian_determinant_forward(u, True), ext.jacobian_determinant_backward(g, u, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        f = ext.jacobian_determinant_forward(u, True)
        b = ext.jacobian_determinant_backward(g, u, True)
    side.synchronize()
    assert torch.equal(f, ref_f) and torch.equal(b, ref_b)
    # empty batch: no launch, right shapes
    for shape in [(0, 3, 4, 5, 6), (0, 2, 4, 5)]:
        u0 = torch.zeros(shape, device="cuda")
        g0 = torch.zeros((0, 1) + shape[2:], device="cuda")
        assert ext.jacobian_determinant_forward(u0, True).shape == g0.shape
        assert ext.jacobian_determinant_backward(g0, u0, True).shape == u0.shape
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ext.jacobian_determinant_forward(u.cpu(), True)
    with pytest.raises(RuntimeError, match="vector fields"):
        ext.jacobian_determinant_forward(u[:, :2].contiguous(), True)
    with pytest.raises(RuntimeError, match="two- and three-dimensional"):
        ext.jacobian_determinant_forward(u[:, :, 0, 0].contiguous(), True)
    with pytest.raises(RuntimeError, match="grad_out must have shape"):
        ext.jacobian_determinant_backward(u, u, True)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        ext.jacobian_determinant_backward(g.double(), u, True)
    with pytest.raises(RuntimeError, match="float32 and float64"):
        ext.jacobian_determinant_forward(u.half(), True)


@pytest.mark.parametrize("shape", [(3, 3, 20, 18, 33), (2, 2, 40, 37)])
def test_graph_capture(lm, shape):
    """Forward and backward captured on one stream replay the eager call's bits and follow new contents of u."""
    ext = lm.lagomorph_ext
    lm.set_debug_mode(False)   # debug mode synchronises after every launch: not capturable
    try:
        u = smooth_field(shape, 2.0, 21, 2.0)
        go = smooth_field((shape[0], 1) + shape[2:], 1.0, 22, 1.0)

        def fn():
            return ext.jacobian_determinant_forward(u, True), ext.jacobian_determinant_backward(go, u, True)

        ref = fn()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fn()
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
        u2 = smooth_field(shape, 3.0, 23, 1.0)
        ref2 = (ext.jacobian_determinant_forward(u2, True), ext.jacobian_determinant_backward(go, u2, True))
        u.copy_(u2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], ref2[0]) and torch.equal(out[1], ref2[1]) and not torch.equal(ref2[0], ref[0])
        del graph
    finally:
        lm.set_debug_mode(True)


def test_on_a_field_the_library_produced(lm):
    """h = expmap(metric, m0): the operator's bits on h equal the reference module's; the shoot is scaled so that the
    reference finds no folded voxel, and then the kernel finds none either."""
    sp = (24, 20, 36)
    met = lm.FluidMetric([0.1, 0.0, 0.01])
    m = smooth_field((2, 3) + sp, 3.0, 31, 1.0)
    with torch.no_grad():
        m *= 0.5 / met.sharp(m).abs().max()   # initial velocity of at most half a voxel
        h = lm.expmap(met, m, num_steps=10)
        det = lm.jacobian_determinant(h)
    want = jacdet_ref.forward(host(h), True)
    assert float(np.abs(host(h)).max()) > 0.1
    assert want.min() > 0, "the test's momentum folds the map: scale it down"
    assert_bits(det, want, "jacobian_determinant(expmap)")
    assert float(det.min()) > 0
