"""GPU: invert_displacement (csrc/invert.hip: invert_disp_kernel / invert_disp_adjoint_kernel).

Forward: bit for bit the unfused loop `v = -u; v = -interp_forward(u, v, 1.0)` of the library's own operators, and
within the project's tolerance of the test-side reference built from the CPU oracle (tests/invert_ref.py).  Tolerances
are RTOL x max|reference| as in tests/test_gpu_parity.py; where two steps chain, or the iteration runs to its fixed
point on a field with contraction bound L = 0.5, the factor is 2:  e_{k+1} <= L e_k + RTOL max|u|  gives
e <= RTOL max|u| / (1 - L) = 2 RTOL max|u|  (the truncation term 0.5^60 < 1e-18 is below both precisions)."""
import numpy as np
import pytest
import torch

import invert_ref
from gpu_util import DTYPES, NPDT, SHAPES2, SHAPES3, assert_bits, dev, host, rnd, smooth_field, units_of
from parity_rule import rtol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm():
    import lagomorph_amd

    lagomorph_amd.set_debug_mode(True)
    yield lagomorph_amd
    lagomorph_amd.set_debug_mode(False)


def loop(ext, u, iters):
    """The unfused iteration over the existing operators."""
    v = -u
    for _ in range(iters):
        v = -ext.interp_forward(u, v, 1.0)
    return v


# ---- 1. forward bits against the unfused loop

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", SHAPES3 + SHAPES2)
def test_forward_bits_against_the_unfused_loop(lm, dtype, sp):
    """Random fields at scale 0.3 and at scale 3.0 -- the latter far outside the contraction regime: samples land out
    of range and on the clamped border."""
    ext = lm.lagomorph_ext
    for nn in (1, 2, 3):
        for scale in (0.3, 3.0):
            rng = np.random.default_rng(abs(hash((sp, nn, scale))) % 2**31)
            u = dev(rnd(rng, (nn, len(sp)) + sp, dtype, scale))
            for iters in (0, 1, 2, 5):
                got = ext.invert_displacement_forward(u, iters)
                assert_bits(got, loop(ext, u, iters), f"{sp} N={nn} scale={scale} iters={iters}")
    assert_bits(lm.invert_displacement(u, 2), loop(ext, u, 2), "invert_displacement")


def test_forward_bits_production_geometry(lm):
    """2 x 3 x 128^3 float32, 5 steps, a smooth field of amplitude 2: the loop's interp_forward runs its vectorised
    production kernels here."""
    ext = lm.lagomorph_ext
    u = smooth_field((2, 3, 128, 128, 128), 8.0, 228, 2.0)
    got = ext.invert_displacement_forward(u, 5)
    want = loop(ext, u, 5)
    assert torch.equal(got, want), f"not bit-identical: max abs diff {float((got - want).abs().max()):.3e}"
    assert not torch.equal(got, loop(ext, u, 4))   # the fifth step still moves this field: the count is honoured


# ---- 2. forward against the oracle, 3. it is an inverse

@pytest.fixture(scope="module")
def oracle_fields():
    """(dtype, sp) -> (u, v_1, v_60) of the reference on the L = 0.5 field, computed once."""
    cache = {}

    def get(dtype, sp):
        key = (dtype, sp)
        if key not in cache:
            u = invert_ref.field(sp, 2, NPDT[dtype])
            assert invert_ref.lipschitz_bound(u) <= 0.5 + 1e-9
            cache[key] = (u, invert_ref.forward(u, 1), invert_ref.forward(u, 60))
            for a in cache[key]:
                a.setflags(write=False)
        return cache[key]

    return get


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", SHAPES3 + SHAPES2)
def test_forward_against_oracle(lm, oracle_fields, dtype, sp):
    ext = lm.lagomorph_ext
    u, v1, v60 = oracle_fields(dtype, sp)
    e1 = units_of(ext.invert_displacement_forward(dev(u), 1), v1, dtype)
    e60 = units_of(ext.invert_displacement_forward(dev(u), 60), v60, dtype)
    print(f"{sp} {dtype}: iters 1 {e1:.4f} (allowed 1), iters 60 {e60:.4f} (allowed 2) of RTOL x max|ref|")
    assert e1 <= 1.0
    assert e60 <= 2.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", SHAPES3 + SHAPES2)
def test_it_is_an_inverse(lm, oracle_fields, dtype, sp):
    """compose(v, u) = (id + u) o (id + v) - id vanishes to 2 RTOL max|u| at 60 steps -- and does not at 1 step, so
    the check can fail."""
    u = dev(oracle_fields(dtype, sp)[0])
    bound = 2 * rtol(dtype) * float(u.abs().max())
    res60 = float(lm.compose(lm.invert_displacement(u, 60), u).abs().max())
    res1 = float(lm.compose(lm.invert_displacement(u, 1), u).abs().max())
    print(f"{sp} {dtype}: residual at 60 steps {res60 / bound:.3e}, at 1 step {res1 / bound:.3e} of the bound")
    assert res60 <= bound
    assert res1 > bound


# ---- 4. adjoint

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", SHAPES3 + SHAPES2)
def test_adjoint(lm, oracle_fields, dtype, sp):
    """lam against the float64 solve (det M >= (1 - L)^3 = 0.125 on these fields), identical between two calls; d_u
    end to end through the autograd function: two chained operators, each at the project's tolerance."""
    ext = lm.lagomorph_ext
    u, _, v60 = oracle_fields(dtype, sp)
    rng = np.random.default_rng(abs(hash(sp)) % 2**31)
    go = rnd(rng, u.shape, dtype)
    ut, vt, got = dev(u), dev(v60), dev(go)
    l1 = ext.invert_displacement_adjoint(got, ut, vt)
    el = units_of(l1, invert_ref.lam(go, u, v60), dtype)
    assert torch.equal(l1, ext.invert_displacement_adjoint(got, ut, vt)), "lam differs between two calls"
    ug = dev(u).requires_grad_(True)
    v = lm.invert_displacement(ug, 60)
    v.backward(got)
    ed = units_of(ug.grad, invert_ref.d_u(go, u, host(v)), dtype)
    print(f"{sp} {dtype}: lam {el:.4f} (allowed 1), d_u {ed:.4f} (allowed 2) of RTOL x max|ref|")
    assert el <= 1.0
    assert ed <= 2.0


# ---- 5. gradcheck

@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9)])
def test_gradcheck(lm, sp):
    u = dev(invert_ref.field(sp, 2, np.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: lm.invert_displacement(x, 60), (u,), nondet_tol=1e-10)


# ---- 6. behaviour

@pytest.mark.parametrize("sp", [(6, 5, 16), (7, 9)])
def test_noncontiguous_stream_empty_and_errors(lm, sp):
    ext = lm.lagomorph_ext
    d = len(sp)
    rng = np.random.default_rng(4)
    base = rnd(rng, (2,) + sp + (d,), torch.float32, 0.7)
    u_nc = dev(base).permute((0, d + 1) + tuple(range(1, d + 1)))   # channels last in memory
    assert not u_nc.is_contiguous()
    u = u_nc.contiguous()
    go = dev(rnd(rng, u.shape, torch.float32))
    go_nc = go.transpose(2, 3).contiguous().transpose(2, 3)
    assert not go_nc.is_contiguous()
    v = ext.invert_displacement_forward(u, 5)
    lam = ext.invert_displacement_adjoint(go, u, v)
    assert_bits(ext.invert_displacement_forward(u_nc, 5), v, "non-contiguous forward")
    assert_bits(ext.invert_displacement_adjoint(go_nc, u_nc, v), lam, "non-contiguous adjoint")
    assert_bits(lm.invert_displacement(u_nc, 5), v, "non-contiguous invert_displacement")
    # a non-default stream
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        vs = ext.invert_displacement_forward(u, 5)
        ls = ext.invert_displacement_adjoint(go, u, v)
    side.synchronize()
    assert torch.equal(vs, v) and torch.equal(ls, lam)
    # empty batch: no launch, right shapes
    u0 = torch.zeros((0, d) + sp, device="cuda")
    assert ext.invert_displacement_forward(u0, 3).shape == u0.shape
    assert ext.invert_displacement_adjoint(u0, u0, u0).shape == u0.shape
    assert lm.invert_displacement(u0).shape == u0.shape
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ext.invert_displacement_forward(u.cpu(), 3)
    with pytest.raises(RuntimeError, match="vector field"):
        ext.invert_displacement_forward(u[:, :1].contiguous(), 3)
    with pytest.raises(RuntimeError, match="float32 and float64"):
        ext.invert_displacement_forward(u.half(), 3)
    with pytest.raises(RuntimeError, match="iters must not be negative"):
        ext.invert_displacement_forward(u, -1)
    with pytest.raises(RuntimeError, match="shape of u"):
        ext.invert_displacement_adjoint(go[:1], u, v)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        ext.invert_displacement_adjoint(go.double(), u, v)


@pytest.mark.parametrize("sp", [(6, 5, 16), (7, 9)])
def test_graph_capture(lm, sp):
    """Forward and adjoint captured on one stream (no parallel branches) replay the eager call's bits."""
    ext = lm.lagomorph_ext
    lm.set_debug_mode(False)   # debug mode synchronises after every launch: not capturable
    try:
        rng = np.random.default_rng(5)
        u = dev(rnd(rng, (2, len(sp)) + sp, torch.float32, 0.4))
        go = dev(rnd(rng, u.shape, torch.float32))

        def fn():
            v = ext.invert_displacement_forward(u, 5)
            return v, ext.invert_displacement_adjoint(go, u, v)

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
        del graph
    finally:
        lm.set_debug_mode(True)


def test_on_a_field_the_library_produced(lm):
    """h = expmap(metric, m0) in 5 steps at 1 x 3 x 32^3: the default 20 steps leave a smaller residual than 1 step."""
    sp = (32, 32, 32)
    met = lm.FluidMetric([0.1, 0.0, 0.01])
    m = smooth_field((1, 3) + sp, 3.0, 31, 1.0)
    with torch.no_grad():
        m *= 0.5 / met.sharp(m).abs().max()   # initial velocity of at most half a voxel
        h = lm.expmap(met, m, num_steps=5)
        res = float(lm.compose(lm.invert_displacement(h), h).abs().max())
        res1 = float(lm.compose(lm.invert_displacement(h, iters=1), h).abs().max())
    amp = float(h.abs().max())
    print(f"expmap field of amplitude {amp:.3f}: residual {res:.3e} at 20 steps, {res1:.3e} at 1 step")
    assert amp > 0.1
    assert res < res1
