"""GPU: joint_histogram (csrc/mi.hip: mi_hist_kernel; csrc/chunk_table.hpp: table_reduce_kernel), its backward (mi_bwd_kernel),
mutual_information, mi_loss, MISimilarity and the latter as the `similarity` of lddmm_step and LDDMMAtlasBuilder.

P is compared with the numpy reference tests/mi_ref.py (held against central differences and against the kernels' own
header on the CPU, tests/test_mi_host.py) BIT FOR BIT: the histogram is a sum of 64-bit integers.  MI, NMI, dI and dJ are
judged by the project's rule, unchanged: max|got - ref| <= RTOL x max|ref| with RTOL 1e-5 (float32) and 1e-12 (float64).
The cases (shapes, bins, the seven kinds of input) are mi_ref's; their values are float32 numbers, so both precisions
share one reference per case."""
import numpy as np
import pytest
import torch

import mi_ref
from gpu_util import DTYPES, NPDT, dev, host, units_of

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def lm():
    import lagomorph_amd

    lagomorph_amd.set_debug_mode(True)
    yield lagomorph_amd
    lagomorph_amd.set_debug_mode(False)


def case(lead, sp, kind, dtype, grad=True):
    """(I, J, g, range_I, range_J) on the device; J IS I for the kind "same" when no gradient is wanted (with one, the
    two are separate leaves of equal values, so that dI and dJ can be told apart)."""
    Ih, Jh, gh, rI, rJ = mi_ref.inputs(lead, sp, kind)
    I = dev(Ih, dtype).requires_grad_(grad)
    J = I if kind == "same" and not grad else dev(Jh, dtype).requires_grad_(grad)
    return I, J, dev(gh, dtype), rI, rJ


def normal(shape, seed, dtype=torch.float32):
    return torch.randn(shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(seed))


# ---- 1. P equals the reference exactly

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lead,sp", mi_ref.SHAPES)
def test_histogram_equals_the_reference_bit_for_bit(lm, dtype, lead, sp):
    from lagomorph_amd import lagomorph_ext as ext

    nvox, rows = int(np.prod(sp)), lead[0] * lead[1]
    for B in mi_ref.BINS:
        chunks = ext._lib.lago_mi_scratch_tables(B, rows, nvox)
        print(f"{lead} + {sp} B={B}: {chunks} workgroups (partial tables) a row")
        if sp == (33, 40, 41):
            assert chunks >= 4          # 54 120 voxels: a row is shared by several workgroups, each with its replicas
        for kind in mi_ref.KINDS:
            I, J, _, rI, rJ = case(lead, sp, kind, dtype, grad=False)
            assert (J is I) == (kind == "same")
            P = lm.joint_histogram(I, J, bins=B, range_I=rI, range_J=rJ)
            assert P.dtype == torch.float64 and P.shape == lead + (B, B) and P.is_contiguous()
            want = mi_ref.case_reference(lead, sp, kind, B)[0]
            assert torch.equal(P.cpu(), torch.from_numpy(want)), (kind, B, float((P.cpu() - torch.from_numpy(want)).abs().max()))
            if kind == "constant":
                assert int((P != 0).sum()) <= 16 * rows


# ---- 2. MI, NMI, dI and dJ against the reference

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", mi_ref.KINDS)
def test_mi_nmi_and_gradients_against_the_reference(lm, dtype, kind):
    """Every shape, bin count and MI / NMI of one kind of input; the upstream gradient on (N, C) is random.

    The constant pair is the hard one for MI in float64: P is an outer product of two windows, the O(1) entropies cancel
    and MI = 7.657e-10 is what the three eps terms leave, so 1e-12 max|ref| is 7.7e-22 absolute of a sum of O(1) terms.
    No tolerance on the entropies gives that; the same operations in the same order do.  P is exact, and the product and
    the reference both take every sum in one fixed order (similarity._fold_sum, mi_ref.fold_sum), so MI differs only
    where a logarithm of the device differs from the host's in its last bit.  With torch.sum, whose order depends on the
    shape, the pair was 2.2e-16 = 2.9e5 x RTOL x max|ref| off for B in {4, 5, 64}; with the fixed order it is at 0, as are
    five of the other six kinds (0.0045 for "clamp": a last bit of a logarithm; it could show on the constant pair too,
    whose tables hold six distinct values).  dI and dJ of the constant pair are exactly 0 in both: the two lower windows
    are equal and their derivatives opposite."""
    worst = [0.0, 0.0, 0.0]
    failed = []
    for lead, sp in mi_ref.SHAPES:
        I, J, g, rI, rJ = case(lead, sp, kind, dtype)
        for B in mi_ref.BINS:
            for normalized in (False, True):
                _, rmi, rdI, rdJ = mi_ref.case_reference(lead, sp, kind, B, normalized)
                mi = lm.mutual_information(I, J, bins=B, range_I=rI, range_J=rJ, normalized=normalized)
                assert mi.dtype == dtype and mi.shape == lead
                dI, dJ = torch.autograd.grad(mi, (I, J), g)
                u = [units_of(a, b, dtype) for a, b in zip((mi, dI, dJ), (rmi, rdI, rdJ))]
                print(f"{lead}+{sp} {kind} B={B} normalized={normalized} {dtype}: MI {u[0]:.3g} dI {u[1]:.3g} dJ {u[2]:.3g} "
                      f"x RTOL x max|ref|   (max|ref| {np.abs(rmi).max():.3e} {np.abs(rdI).max():.3e} {np.abs(rdJ).max():.3e})")
                worst = [max(a, b) for a, b in zip(worst, u)]
                if not max(u) <= 1.0:
                    failed.append((sp, B, normalized, u))
                if not normalized:   # one gradient alone (the other output is neither computed nor written): the same bits
                    kw = dict(bins=B, range_I=rI, range_J=rJ)
                    (oI,) = torch.autograd.grad(lm.mutual_information(I, J.detach(), **kw), (I,), g)
                    (oJ,) = torch.autograd.grad(lm.mutual_information(I.detach(), J, **kw), (J,), g)
                    assert torch.equal(oI, dI) and torch.equal(oJ, dJ)
    print(f"{kind} {dtype}: worst MI {worst[0]:.3g} dI {worst[1]:.3g} dJ {worst[2]:.3g} of the tolerance")
    assert not failed, failed


@pytest.mark.parametrize("dtype", DTYPES)
def test_need_flags_of_the_shim(lm, dtype):
    """need_I alone and need_J alone: the other output is None, the one computed has the bits of the joint call."""
    from lagomorph_amd import lagomorph_ext as ext

    lead, sp, B = (1, 2), (9, 5, 70), 32
    I, J, _, rI, rJ = case(lead, sp, "clamp", dtype, grad=False)
    G = normal(lead + (B, B), 5, torch.float64)
    dI, dJ = ext.mi_backward(G, I, J, B, rI, rJ, True, True)
    oI, none_J = ext.mi_backward(G, I, J, B, rI, rJ, True, False)
    none_I, oJ = ext.mi_backward(G, I, J, B, rI, rJ, False, True)
    assert none_I is None and none_J is None and torch.equal(oI, dI) and torch.equal(oJ, dJ)
    assert ext.mi_backward(G, I, J, B, rI, rJ, False, False) == (None, None)
    rdI, rdJ = mi_ref.backward(host(G), *mi_ref.inputs(lead, sp, "clamp")[:2], B, rI, rJ)
    assert units_of(dI, rdI, dtype) <= 1.0 and units_of(dJ, rdJ, dtype) <= 1.0


# ---- 3. symmetry

@pytest.mark.parametrize("dtype", DTYPES)
def test_symmetry_bit_for_bit(lm, dtype):
    for lead, sp in mi_ref.SHAPES[:3]:
        for kind in ("noise", "clamp", "nonfinite"):
            I, J, g, rI, rJ = case(lead, sp, kind, dtype)
            for B in (5, 32):
                a = lm.joint_histogram(I, J, bins=B, range_I=rI, range_J=rJ)
                b = lm.joint_histogram(J, I, bins=B, range_I=rJ, range_J=rI)
                assert torch.equal(b, a.transpose(-1, -2))
                G = normal(a.shape, 9, torch.float64)
                aI, aJ = torch.autograd.grad(a, (I, J), G)
                bJ, bI = torch.autograd.grad(b, (J, I), G.transpose(-1, -2).contiguous())
                assert torch.equal(aI, bI) and torch.equal(aJ, bJ)
                assert float(aI.abs().max()) > 0 and float(aJ.abs().max()) > 0


# ---- 4. gradcheck

@pytest.mark.parametrize("sp", [(4, 5, 6), (5, 7)])
def test_gradcheck(lm, sp):
    """Ranges (-4, 4) around values of standard deviation 0.5: no voxel sits within the step of a clamp edge, where the
    derivative jumps.  The function that is differenced is the QUANTISED one, the gradient that of the unquantised one: a
    step h moves each of a voxel's 16 products by a rounding of up to 2^-33, a noise of about 16 x 2^-33 |G| / (2 h nvox)
    in the difference quotient, against a gradient of the order s |G| / nvox with s = (B - 3) / 8.  With h = 1e-3 that is
    1e-6 relative and the truncation error h^2 s^2 / 6 is about as much: rtol 1e-4, atol 1e-7 (entries are 1e-4 to
    1e-2)."""
    I = 0.5 * normal((1, 2) + sp, 31, torch.float64)
    J = torch.cos(3.0 * I) + 0.3 * normal((1, 2) + sp, 32, torch.float64)
    assert float(I.abs().max()) < 3.9 and float(J.abs().max()) < 3.9
    r = (-4.0, 4.0)
    kw = dict(eps=1e-3, atol=1e-7, rtol=1e-4)
    for B in (8, 32):
        for f in (lambda a, b: lm.mutual_information(a, b, bins=B, range_I=r, range_J=r),
                  lambda a, b: lm.mutual_information(a, b, bins=B, range_I=r, range_J=r, normalized=True),
                  lambda a, b: lm.mi_loss(a, b, bins=B, range_I=r, range_J=r, reduction="sum")):
            Ig, Jg = I.clone().requires_grad_(True), J.clone().requires_grad_(True)
            assert torch.autograd.gradcheck(lambda a: f(a, J), (Ig,), **kw)
            assert torch.autograd.gradcheck(lambda b: f(I, b), (Jg,), **kw)
            assert torch.autograd.gradcheck(f, (Ig, Jg), **kw)


# ---- 5. bits and stability

def _all(lm, I, J, g, B, rI, rJ):
    I, J = I.detach().requires_grad_(True), J.detach().requires_grad_(True)
    P = lm.joint_histogram(I, J, bins=B, range_I=rI, range_J=rJ)
    mi = lm.mutual_information(I, J, bins=B, range_I=rI, range_J=rJ)
    return (P.detach(), mi.detach()) + torch.autograd.grad(mi, (I, J), g)


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_on_a_second_call_and_on_a_side_stream(lm, dtype):
    for (lead, sp), B in zip(mi_ref.SHAPES[1:], (32, 5, 64)):
        for kind in ("smooth", "clamp"):
            I, J, g, rI, rJ = case(lead, sp, kind, dtype)
            a = _all(lm, I, J, g, B, rI, rJ)
            b = _all(lm, I, J, g, B, rI, rJ)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                c = _all(lm, I, J, g, B, rI, rJ)
            s.synchronize()
            for x, y, z in zip(a, b, c):
                assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_contiguous_and_misaligned_input(lm, dtype):
    lead, sp, B = (2, 2), (5, 6, 7), 32
    Ih, Jh, gh, _, _ = mi_ref.inputs(lead, sp, "noise")
    Ih, Jh = Ih.astype(NPDT[dtype]), Jh.astype(NPDT[dtype])
    rI, rJ = mi_ref.auto_range(Ih), (-1.0, 1.5)
    I, J, g = dev(Ih), dev(Jh), dev(gh, dtype)
    want = _all(lm, I, J, g, B, rI, rJ)
    pI, pJ = (dev(a.transpose(0, 1, 4, 3, 2)).permute(0, 1, 4, 3, 2) for a in (Ih, Jh))   # permuted views
    assert not pI.is_contiguous() and torch.equal(pI, I)
    got = _all(lm, pI, pJ, g, B, rI, rJ)
    assert all(x.is_contiguous() and torch.equal(x, y) for x, y in zip(got, want))
    sl = _all(lm, I[:, 1:], J[:, 1:], g[:, 1:], B, rI, rJ)                                 # a channel slice
    assert not I[:, 1:].is_contiguous() and all(torch.equal(x, y[:, 1:]) for x, y in zip(sl, want))
    # one element (4 / 8 bytes) off the alignment of the vector loads: both images, and one of them alone
    oI, oJ = (dev(np.concatenate([a.reshape(-1)[:1], a.reshape(-1)]))[1:].reshape(a.shape) for a in (Ih, Jh))
    assert oI.data_ptr() % 16 != 0 and oJ.data_ptr() % 16 != 0
    for a, b in ((oI, oJ), (oI, J), (I, oJ)):
        assert all(torch.equal(x, y) for x, y in zip(_all(lm, a, b, g, B, rI, rJ), want))


# ---- 6. an empty batch

@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_batch(lm, dtype):
    for shape in ((0, 3, 5, 6, 7), (0, 1, 7, 9)):
        I = torch.zeros(shape, dtype=dtype, device="cuda", requires_grad=True)
        J = torch.zeros(shape, dtype=dtype, device="cuda", requires_grad=True)
        P = lm.joint_histogram(I, J, bins=8)
        assert P.shape == shape[:2] + (8, 8) and P.dtype == torch.float64
        mi = lm.mutual_information(I, J)
        assert mi.shape == shape[:2] and mi.dtype == dtype
        dI, dJ = torch.autograd.grad(mi, (I, J), torch.zeros_like(mi))
        assert dI.shape == I.shape and dJ.shape == J.shape
        assert lm.mi_loss(I, J, reduction="none").shape == shape[:2]
        assert float(lm.mi_loss(I.detach(), J.detach(), reduction="sum")) == 0.0


# ---- 7. graph capture

def test_graph_capture_of_forward_and_backward(lm):
    """Forward and backward of two calls with different bin counts (and ranges) in one captured graph, replayed on new
    data: the bits of the eager calls.  The ranges are explicit (a range of None reads the tensor on the host) and travel
    in the captured launches by value."""
    lead, sp, dtype = (1, 2), (9, 5, 70), torch.float32
    calls = ((32, (-2.0, 2.0), (-1.5, 2.5)), (5, (-1.0, 0.75), (-3.0, 3.0)))
    lm.set_debug_mode(False)
    try:
        I, J, g, _, _ = case(lead, sp, "noise", dtype)
        outs = [[torch.empty(lead + (B, B), dtype=torch.float64, device="cuda"), torch.empty(lead, dtype=dtype, device="cuda"),
                 torch.empty_like(I.detach()), torch.empty_like(I.detach())] for B, _, _ in calls]

        def work():
            for (B, rI, rJ), o in zip(calls, outs):
                P = lm.joint_histogram(I, J, bins=B, range_I=rI, range_J=rJ)
                mi = lm.mutual_information(I, J, bins=B, range_I=rI, range_J=rJ)
                dI, dJ = torch.autograd.grad(mi, (I, J), g)
                for dst, src in zip(o, (P.detach(), mi.detach(), dI, dJ)):
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
        for kind in ("smooth", "nonfinite"):
            nI, nJ, ng, _, _ = mi_ref.inputs(lead, sp, kind)
            with torch.no_grad():
                I.copy_(dev(nI, dtype))
                J.copy_(dev(nJ, dtype))
                g.copy_(dev(ng, dtype))
            for o in outs:
                for t in o:
                    t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for (B, rI, rJ), o in zip(calls, outs):
                eager = _all(lm, I, J, g, B, rI, rJ)
                assert all(torch.equal(x, y) for x, y in zip(o, eager))
                P, mi, dI, dJ = mi_ref.reference(nI, nJ, B, rI, rJ, g=ng)
                assert torch.equal(o[0].cpu(), torch.from_numpy(P))
                assert max(units_of(a, b, dtype) for a, b in zip(o[1:], (mi, dI, dJ))) <= 1.0
    finally:
        lm.set_debug_mode(True)


# ---- 8. the matching step

def _blobs():
    sp = (16, 16, 16)
    g = np.indices(sp).astype(np.float64)
    blob = lambda c: np.exp(-sum((g[a] - c[a]) ** 2 for a in range(3)) / (2 * 3.0 ** 2))
    I = dev(blob((8, 8, 8))[None, None].astype(np.float32))
    targets = np.stack([np.cos(3.0 * blob((9, 8, 7))), np.cos(3.0 * blob((7, 9, 8)))])[:, None].astype(np.float32)
    return sp, I, dev(targets)


MI_RANGES = dict(range_I=(0.0, 1.0), range_J=(-1.0, 1.0))   # of the blob atlas and of cos(3 blob)
# The step size, chosen on the device (32 bins, three integration steps, reg_weight 1e-2).  -mean MI at m = 0 is -0.4918;
# after two steps at learning rate 2e2: -0.5048, 1e3: -0.5655 (second call's image term -0.5241), 5e3: -0.7232 with
# max|m| 2.6, 2e4: -0.4396 (overshoots), 1e5: -0.2116.  1e3 moves the term clearly and stays far from the overshoot.
# The squared difference on the same pair: -0.4911, -0.4881, -0.4745 after two steps at 2e2, 1e3, 5e3 (MI falls).
MI_STEP = 1e3


def test_lddmm_step_with_mi_matches_targets_of_another_modality(lm):
    """The blob atlas against targets cos(3 blob(shifted)): the intensity relation is not monotone.  The step's image term
    is minus the mean MI of the deformed atlas against the targets; two steps with MISimilarity lower it (raise MI), two
    steps with the squared difference do not.  Only the sign of each change is asserted; the values are printed."""
    sp, I, img = _blobs()
    metric = lm.GaussianMetric([1.5, 3.0], weights=[1.0, 0.5])
    sim = lm.MISimilarity(**MI_RANGES)

    def term(mm):
        with torch.no_grad():
            return float(lm.mi_loss(lm.interp(I, lm.expmap(metric, mm, num_steps=3)), img, **MI_RANGES))

    kw = dict(dataset_size=2, integration_steps=3, reg_weight=1e-2, learning_rate_pose=MI_STEP)
    m = torch.zeros((2, 3) + sp, device="cuda")
    before = term(m)
    m, loss1, reg1 = lm.lddmm_step(I, m, img, metric, similarity=sim, **kw)
    m, loss2, reg2 = lm.lddmm_step(I, m, img, metric, similarity=sim, **kw)
    after = term(m)
    img1, img2 = float(loss1) - float(reg1), float(loss2) - float(reg2)
    print(f"-mean MI: {before:.6e} at m = 0, first call {img1:.6e}, second call {img2:.6e}; after two steps {after:.6e}")
    assert abs(img1 - before) <= 1e-5 * abs(before)          # the step's image term IS -MI.sum() nvox / numel
    assert after < before and img2 < img1
    assert bool(torch.isfinite(m).all()) and float(m.abs().max()) > 0
    # the squared difference on the same pair, same step size as the LNCC test uses for it
    m = torch.zeros((2, 3) + sp, device="cuda")
    for _ in range(2):
        m, _, _ = lm.lddmm_step(I, m, img, metric, **{**kw, "learning_rate_pose": 2e2})
    after_sse = term(m)
    print(f"-mean MI after two steps of the squared difference: {after_sse:.6e}")
    assert float(m.abs().max()) > 0 and not after_sse < before


def test_atlas_builder_takes_mi_as_similarity(lm):
    sp, I, images = _blobs()
    sim = lm.MISimilarity(**MI_RANGES)
    b = lm.LDDMMAtlasBuilder(images, batch_size=2, lddmm_integration_steps=2, reg_weight=1e-2, I0=I[0],
                             metric=lm.GaussianMetric([1.5, 3.0], weights=[1.0, 0.5]), similarity=sim)
    assert b.similarity is sim
    before = float(lm.mi_loss(b.I.detach().expand(2, -1, -1, -1, -1).contiguous(), images, **MI_RANGES))
    loss, reg = b.iteration(0, last_of_epoch=True)
    assert abs((float(loss) - float(reg)) - before) <= 1e-5 * abs(before)
    assert bool(torch.isfinite(b.ms[0]).all()) and float(b.ms[0].abs().max()) > 0 and bool(torch.isfinite(b.I).all())


def test_loss_reductions_and_similarity(lm):
    lead, sp = (2, 2), (5, 6, 7)
    I, J, _, _, _ = case(lead, sp, "noise", torch.float32, grad=False)
    mi = lm.mutual_information(I, J)
    none = lm.mi_loss(I, J, reduction="none")
    assert torch.equal(none, -mi)
    assert torch.equal(lm.mi_loss(I, J, reduction="sum"), none.sum()) and torch.equal(lm.mi_loss(I, J), none.mean())
    assert torch.equal(lm.MISimilarity()(I, J), none.sum() * 210)
    assert torch.equal(lm.mutual_information(I, J, range_I=mi_ref.auto_range(host(I)), range_J=mi_ref.auto_range(host(J))), mi)
    const = torch.full_like(I, 3.0)                       # a constant image takes the range (lo, lo + 1)
    assert torch.equal(lm.joint_histogram(const, J), lm.joint_histogram(const, J, range_I=(3.0, 4.0)))
    assert not torch.equal(lm.mutual_information(I, J, eps=1e-3), mi)


# ---- 9. production size

def test_production_size_128(lm):
    """2 x 1 x 128^3 float32, 32 bins, ranges taken from the tensors: P exact, dI and dJ within the rule."""
    shape, B = (2, 1, 128, 128, 128), 32
    I = normal(shape, 51).requires_grad_(True)
    J = (torch.cos(3.0 * I.detach()) + 0.3 * normal(shape, 52)).requires_grad_(True)
    g = normal(shape[:2], 53)
    P = lm.joint_histogram(I, J, bins=B)
    mi = lm.mutual_information(I, J, bins=B)
    dI, dJ = torch.autograd.grad(mi, (I, J), g)
    rP, rmi, rdI, rdJ = mi_ref.reference(host(I), host(J), B, g=host(g))
    assert torch.equal(P.cpu(), torch.from_numpy(rP))
    u = [units_of(a, b, torch.float32) for a, b in zip((mi, dI, dJ), (rmi, rdI, rdJ))]
    print(f"{shape} B={B}: MI {u[0]:.3f} dI {u[1]:.3f} dJ {u[2]:.3f} x RTOL x max|ref|")
    assert max(u) <= 1.0, u


# ---- 10. the chunking does not show (csrc/chunk_table.hpp)

_CHUNK_REFS = {}


def _chunk_case(lead, sp, B):
    """(I, J, range_I, range_J, P) of a noise pair in float32 values, the reference computed once for both precisions."""
    key = (lead, sp, B)
    if key not in _CHUNK_REFS:
        rng = np.random.default_rng([B, *sp])
        Ih, Nh = (rng.standard_normal(lead + sp).astype(np.float32) for _ in range(2))
        Jh = (np.float32(0.8) * Ih + np.float32(0.6) * Nh).astype(np.float32)
        rI, rJ = (-2.0, 2.0), (-1.5, 2.5)   # both clamp a few voxels
        P = mi_ref.joint_histogram(Ih.astype(np.float64), Jh.astype(np.float64), B, rI, rJ)
        P.setflags(write=False)
        _CHUNK_REFS[key] = (Ih, Jh, rI, rJ, P)
    return _CHUNK_REFS[key]


def _histogram_with_scratch(I, J, B, rI, rJ, tables):
    """lago_mi_histogram with a scratch of `tables` partial tables a row, as lagomorph_ext.mi_histogram calls it."""
    from lagomorph_amd import lagomorph_ext as ext

    dim, nx, ny, nz = ext._spatial(I)
    rows = I.size(0) * I.size(1)
    P = torch.full((I.size(0), I.size(1), B, B), -1.0, dtype=torch.float64, device=I.device)
    scratch = torch.empty((rows * tables * B * B,), dtype=torch.int64, device=I.device)
    ext._call("lago_mi_histogram", I, ext._ptr(P), ext._ptr(I), ext._ptr(J), ext._ptr(scratch), tables, B, *rI, *rJ, dim,
              rows, nx, ny, nz)
    return P


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [4, 32, 64])
@pytest.mark.parametrize("sp", [(17, 19, 13), (67, 63)], ids=str)
def test_two_ragged_chunks_a_row_equal_one_chunk_a_row(lm, dtype, B, sp):
    """4199 voxels are chunks of 2100 + 2099, 4221 of 2112 + 2109; the rows are odd, so rows 1 and 2 start off the
    16-byte boundary and walk a scalar head, vectors and a scalar tail.  P equals the reference integer for integer,
    and so does the same call with a scratch of ONE table a row (fewer than wanted: one workgroup walks the row)."""
    from lagomorph_amd import lagomorph_ext as ext

    lead, nvox = (1, 3), int(np.prod(sp))
    assert nvox % 2 == 1 and ext._lib.lago_mi_scratch_tables(B, 3, nvox) == 2
    Ih, Jh, rI, rJ, want = _chunk_case(lead, sp, B)
    I, J = dev(Ih, dtype), dev(Jh, dtype)
    P = lm.joint_histogram(I, J, bins=B, range_I=rI, range_J=rJ)
    assert torch.equal(P.cpu(), torch.from_numpy(want))
    assert torch.equal(_histogram_with_scratch(I, J, B, rI, rJ, 1), P)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", [(1, 1), (1, 5), (3, 3, 3), (1, 259)], ids=str)
def test_the_smallest_rows(lm, dtype, sp):
    """Rows below one vector, below one workgroup of lanes, and of a vector count that is no multiple of 256 with a tail."""
    Ih, Jh, rI, rJ, want = _chunk_case((1, 2), sp, 4)
    P = lm.joint_histogram(dev(Ih, dtype), dev(Jh, dtype), bins=4, range_I=rI, range_J=rJ)
    assert torch.equal(P.cpu(), torch.from_numpy(want))
