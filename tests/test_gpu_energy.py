"""GPU: diffusion_energy, bending_energy and energy_operator (csrc/energy.hip) against the numpy reference
tests/energy_ref.py (which tests/test_energy_host.py ties to a torch restatement and to known answers): voxel by voxel
against a bound counted from the kernel's own roundings, bit for bit from call to call, through torch.autograd.gradcheck
and gradgradcheck, composed with ffd_expand, and on tensors that start off the 16-byte alignment.

Shapes (energy_ref.GPU_SHAPES): the host test's list; for every axis of the kernels' tile -- energy_ref.TILE3 = 8 x 8 x 64
voxels, TILE2 = 64 x 64 -- extents of one tile + 1, one tile + 2 and two tiles + 1, so that the two-voxel halo crosses a
tile edge and a ragged last tile occurs on every axis, and (17, 18, 131) with all of that at once; and shapes with an
axis of extent 1 or 2 in 2D and in 3D.  N = 2 with different fields per item, C in {1, 3}, unit spacing and
(1.0, 1.5, 0.7).

float64: energy and operator within 1e-12 max|ref|.  float32 operator, per voxel: |got - ref64| <= K 2^-24 |scale_n|
abs_operator(u)(x), K = 13 (bending) / 8 (diffusion) as energy_stencil.hpp counts them, and within 1e-5 max|ref| on the
random-normal fields; float32 energy within 1e-5 ref.  A field that is affine plus 1e-3 x noise, where A u is small
against u, is held to the per-voxel bound alone (float64: the same bound with 2^-53).  The worst observed fractions of
the bound are printed."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import energy_ref as ref
import offset_views as ov
from gpu_util import dev, host, units_of

pytestmark = pytest.mark.gpu

both_dtypes = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
kinds = pytest.mark.parametrize("kind", ref.KINDS)
UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


@functools.lru_cache(maxsize=None)
def _case(shape, kind, spacing, dtype, C, affine):
    """(u, E, A u, abs_operator(u)) with the reference in float64, computed once and left unchanged."""
    u = ref.field(2, C, shape, np.dtype(dtype), seed=11, affine=affine)
    out = (u, ref.energy(u, kind, spacing), ref.operator(u, kind, spacing), ref.abs_operator(u, kind, spacing))
    for a in out:
        a.setflags(write=False)
    return out


@both_dtypes
@kinds
@pytest.mark.parametrize("shape", ref.GPU_SHAPES, ids=str)
def test_energy_and_operator(shape, kind, dtype):
    import lagomorph_amd as lm

    dt = np.dtype(dtype)
    worst = worst_affine = 0.0
    for spacing in ref.SPACINGS:
        sp = ref.spacing_tuple(spacing, len(shape))
        for C in (1, 3):
            u, want_E, want_A, absop = _case(shape, kind, spacing, dt.name, C, False)
            ud = dev(u)
            E, A = lm.field_energy(ud, kind, sp), lm.energy_operator(ud, kind, sp)
            assert E.shape == (2,) and E.dtype == ud.dtype and A.shape == ud.shape and A.dtype == ud.dtype and A.is_contiguous()
            assert torch.equal(E, (lm.bending_energy if kind == "bending" else lm.diffusion_energy)(ud, spacing if spacing == 1.0 else list(sp)))
            err_E, err_A = np.abs(host(E).astype(np.float64) - want_E), np.abs(host(A).astype(np.float64) - want_A)
            bound = ref.K[kind] * UNIT[dt] * absop
            if dt == np.float64:
                assert units_of(E, want_E, dt, floor=0) <= 1.0, (spacing, C, err_E, want_E)
                assert units_of(A, want_A, dt, floor=0) <= 1.0, (spacing, C)
            else:
                ratio = ref.worst_ratio(err_A, bound)
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"{shape} {kind} {spacing} C {C}: {ratio:.3f} of the per-voxel bound"
                assert units_of(A, want_A, dt, floor=0) <= 1.0, (spacing, C)
                assert (err_E <= 1e-5 * want_E).all(), (spacing, C, err_E, want_E)
            assert torch.equal(ud, dev(u))   # the input is left alone
            # scale: the unscaled result times s[n], inside the same bound; None is ones, bit for bit
            s = np.array([-1.75, 0.3], dtype=dt)
            S = lm.energy_operator(ud, kind, sp, scale=dev(s))
            err_S = np.abs(host(S).astype(np.float64) - want_A * s.astype(np.float64).reshape(2, 1, *([1] * len(shape))))
            if dt == np.float64:
                assert err_S.max() <= 1e-12 * np.abs(want_A).max() * np.abs(s).max()
            else:
                assert ref.worst_ratio(err_S, ref.operator_bound(u, kind, spacing, s)) <= 1.0
            assert torch.equal(lm.energy_operator(ud, kind, sp, scale=torch.ones(2, dtype=ud.dtype, device="cuda")), A)
        # affine plus small noise: the per-voxel bound alone
        u, _, want_A, absop = _case(shape, kind, spacing, dt.name, 3, True)
        A = lm.energy_operator(dev(u), kind, sp)
        ratio = ref.worst_ratio(np.abs(host(A).astype(np.float64) - want_A), ref.K[kind] * UNIT[dt] * absop)
        worst_affine = max(worst_affine, ratio)
        assert ratio <= 1.0, f"{shape} {kind} {spacing} affine: {ratio:.3f} of the per-voxel bound"
    print(f"energy_operator {shape} {kind} {dt.name}: at most {worst:.3f} (random) and {worst_affine:.3f} (affine + noise) of the per-voxel bound")


@both_dtypes
def test_known_answers_on_the_device(dtype):
    import lagomorph_amd as lm

    x = np.meshgrid(*[np.arange(n, dtype=dtype) for n in (6, 7, 8)], indexing="ij")
    const = dev(np.full((1, 2, 6, 7, 8), 3.25, dtype=dtype))
    assert float(lm.diffusion_energy(const)) == 0.0 and not lm.energy_operator(const, "diffusion").any()
    aff = dev((2 * x[0] - 3 * x[1] + x[2] + 4)[None, None])
    assert float(lm.bending_energy(aff)) == 0.0 and not lm.energy_operator(aff, "bending").any()
    assert float(lm.bending_energy(aff, (1.0, 1.5, 0.7))) == 0.0
    quad = dev((x[0] ** 2 + x[0] * x[1])[None, None])
    assert float(lm.bending_energy(quad)) == dtype((4 * 4 * 7 * 8 + 2 * 5 * 6 * 8) / 336)   # small integers: exact sums


@kinds
@pytest.mark.parametrize("shape,spacing", [((5, 6, 7), (1.0, 1.5, 0.7)), ((9, 11), (1.5, 0.7))], ids=str)
def test_gradcheck_and_gradgradcheck(shape, spacing, kind):
    import lagomorph_amd as lm

    u = dev(ref.field(2, 2, shape, np.float64, seed=5)).requires_grad_(True)
    s = torch.tensor([0.7, -1.3], dtype=torch.float64, device="cuda", requires_grad=True)
    # E is quadratic and A u linear in u: central differences are exact at any step, so a large one keeps their rounding
    # (about 1e-16 x |values| / eps) far below the tolerance
    tol = dict(eps=1e-3, atol=1e-7, rtol=1e-7, nondet_tol=0.0)
    f = lambda x: lm.field_energy(x, kind, spacing)   # noqa: E731
    assert torch.autograd.gradcheck(f, (u,), **tol)
    assert torch.autograd.gradgradcheck(f, (u,), **tol)
    g = lambda x, y: lm.energy_operator(x, kind, spacing, scale=y)   # noqa: E731
    assert torch.autograd.gradcheck(g, (u, s), **tol)
    assert torch.autograd.gradgradcheck(g, (u, s), **tol)
    assert torch.autograd.gradcheck(lambda x: lm.energy_operator(x, kind, spacing), (u,), **tol)


@both_dtypes
@kinds
def test_the_gradient_is_the_scaled_operator(kind, dtype):
    import lagomorph_amd as lm

    shape, sp = (9, 10, 70), (1.0, 1.5, 0.7)
    u = dev(ref.field(2, 3, shape, dtype, seed=6)).requires_grad_(True)
    lm.field_energy(u, kind, sp).sum().backward()
    want = (2.0 / float(np.prod(shape))) * lm.energy_operator(u.detach(), kind, sp)
    if dtype == np.float64:
        assert torch.equal(u.grad, want)
    assert (u.grad - want).abs().max() <= 2e-7 * want.abs().max()
    g = dev(np.array([0.5, -2.0], dtype=dtype))
    u.grad = None
    lm.field_energy(u, kind, sp).backward(g)
    want = lm.energy_operator(u.detach(), kind, sp, scale=g * (2.0 / float(np.prod(shape))))
    assert torch.equal(u.grad, want)


def test_a_gradient_nobody_needs_runs_no_kernel(monkeypatch):
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext, regularize

    calls = []
    real = ext._call
    monkeypatch.setattr(regularize._ext, "_call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    u = dev(ref.field(2, 3, (5, 6, 7), np.float32))
    w = torch.ones((), device="cuda", requires_grad=True)
    E = lm.bending_energy(u)
    assert not E.requires_grad and calls == ["lago_field_energy"]
    (E * w).sum().backward()
    assert u.grad is None and w.grad is not None and calls == ["lago_field_energy"]

    class Ctx:
        needs_input_grad = (False, False, False)
        kind, spacing = "bending", 1.0
    assert lm.FieldEnergyFunction.backward(Ctx, torch.ones_like(E)) == (None, None, None) and len(calls) == 1

    class Ctx2:
        needs_input_grad = (False, False, False, False)
        kind, spacing, saved_tensors = "bending", 1.0, (u, None)
    assert lm.EnergyOperatorFunction.backward(Ctx2, torch.ones_like(u)) == (None, None, None, None) and len(calls) == 1
    u.requires_grad_(True)
    lm.bending_energy(u).sum().backward()
    assert calls == ["lago_field_energy", "lago_field_energy", "lago_field_energy_operator"] and u.grad.shape == u.shape


def test_bending_energy_of_an_expanded_lattice():
    import lagomorph_amd as lm

    shape, s = (12, 10, 14), (4, 3, 5)
    m = lm.ffd_grid_shape(shape, s)
    j = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in m], indexing="ij")
    lattice = np.stack([0.5 * j[0] - 1.25 * j[1] + 2.0 * j[2] + 3.0, -j[0] + 0.75 * j[2], 0.25 * j[1] - 4.0])[None]
    E = lm.bending_energy(lm.ffd_expand(dev(lattice), shape, s))
    # the expanded field is affine up to ffd_expand's float64 bound 38 u max|u| <= 2e-13 per voxel (|u| <= 50): a second
    # difference of it is at most 4 x that, and a voxel has 3 squared pure and 3 doubled squared mixed ones
    assert E.shape == (1,) and 0.0 <= float(E) <= 9 * (4 * 2e-13) ** 2
    c = dev(ref.field(2, 3, m, np.float64, seed=8)).requires_grad_(True)
    lm.bending_energy(lm.ffd_expand(c, shape, s), (1.0, 1.5, 0.7)).sum().backward()
    u = lm.ffd_expand(c.detach(), shape, s).requires_grad_(True)
    lm.bending_energy(u, (1.0, 1.5, 0.7)).sum().backward()
    assert torch.equal(c.grad, lm.ffd_restrict(u.grad, s)) and float(c.grad.abs().max()) > 0


@both_dtypes
def test_two_calls_and_a_non_default_stream_give_the_same_bits(dtype):
    import lagomorph_amd as lm

    for shape in ((17, 18, 131), (129, 70)):
        u = dev(ref.field(2, 3, shape, dtype, seed=7))
        sp = ref.spacing_tuple((1.0, 1.5, 0.7), len(shape))
        for kind in ref.KINDS:
            want_E, want_A = lm.field_energy(u, kind, sp), lm.energy_operator(u, kind, sp)
            assert torch.equal(lm.field_energy(u, kind, sp), want_E) and torch.equal(lm.energy_operator(u, kind, sp), want_A)
            torch.cuda.synchronize()
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                got_E, got_A = lm.field_energy(u, kind, sp), lm.energy_operator(u, kind, sp)
            stream.synchronize()
            assert torch.equal(got_E, want_E) and torch.equal(got_A, want_A)


@both_dtypes
@kinds
@pytest.mark.parametrize("shape", [(9, 10, 70), (66, 70)], ids=str)
def test_tensors_off_the_vector_alignment(shape, kind, dtype):
    """u, out, scale, energy and scratch one element past a 16-byte boundary, in buffers with poisoned margins: the
    kernels have one path, so the bits are those of the aligned run, and no margin changes."""
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    d, k = len(shape), ref.KINDS.index(kind)
    sp = ref.spacing_tuple((1.0, 1.5, 0.7), d)
    h = (ctypes.c_double * d)(*sp)
    n = tuple(shape) + (1,) * (3 - d)
    u0 = dev(ref.field(2, 3, shape, dtype, seed=9))
    s0 = dev(np.array([0.75, -1.5], dtype=dtype))
    want_A, want_E = lm.energy_operator(u0, kind, sp, scale=s0), lm.field_energy(u0, kind, sp)
    elems = int(ext._lib.lago_field_energy_scratch_elems(k, d, 2, 3, *n))
    assert elems > 0
    for off in (1, 0):
        (u, ub), (s, sb) = ov.offset_view(u0, off), ov.offset_view(s0, off)
        (out, ob), (E, Eb) = ov.offset_view(torch.zeros_like(u0), off), ov.offset_view(torch.zeros_like(want_E), off)
        scratch, scb = ov.offset_view(torch.zeros(elems, dtype=u0.dtype, device="cuda"), off)
        ext._call("lago_field_energy_operator", u, ext._ptr(out), ext._ptr(u), ext._ptr(s), k, d, 2, 3, *n, h)
        ext._call("lago_field_energy", u, ext._ptr(E), ext._ptr(u), ext._ptr(scratch), elems, k, d, 2, 3, *n, h)
        torch.cuda.synchronize()
        assert torch.equal(out, want_A) and torch.equal(E, want_E), off
        assert ov.poisoned(out) == 0 and ov.poisoned(E) == 0
        for buf, view in ((ub, u), (sb, s), (ob, out), (Eb, E), (scb, scratch)):
            assert ov.margins_intact(buf, view) == [], off
        assert torch.equal(u, u0) and torch.equal(s, s0)
        # ... and through the public functions, which allocate their own outputs
        assert torch.equal(lm.energy_operator(u, kind, sp, scale=s), want_A) and torch.equal(lm.field_energy(u, kind, sp), want_E)


@both_dtypes
def test_empty_problems(dtype, monkeypatch):
    import lagomorph_amd as lm
    from lagomorph_amd import regularize

    calls = []
    monkeypatch.setattr(regularize._ext, "_call", lambda name, *a: calls.append(name))
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    for shape in ((0, 3, 5, 6, 7), (2, 3, 5, 0, 7), (2, 0, 5, 6, 7), (0, 1, 9, 11), (2, 1, 0, 11)):
        u = torch.zeros(shape, dtype=tdt, device="cuda")
        for kind in ref.KINDS:
            E, A = lm.field_energy(u, kind), lm.energy_operator(u, kind, 1.5)
            assert E.shape == (shape[0],) and E.dtype == tdt and not E.any()
            assert A.shape == shape and A.dtype == tdt and A.numel() == 0
    torch.cuda.synchronize()
    assert not calls
