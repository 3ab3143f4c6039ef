"""CPU: the specification of diffusion_energy, bending_energy and energy_operator before any GPU run.

- tests/energy_ref.py, the numpy reference, against an independent pure-torch restatement (slicing differences, the
  operator as torch autograd's gradient of the energy) at 1e-12 in float64, and against known answers: constant, affine
  and quadratic fields, the interior stencils (-Laplacian, the squared 7-point Laplacian), symmetry, E = <u, A u> / V;
- lagomorph_amd/csrc/energy_stencil.hpp, the header the kernels call: tests/native/energy_emul.cpp runs it over the
  same shapes with a plain host compiler; float64 equals the reference at 1e-12, float32 equals the float32 numpy
  restatement of the header's order exactly; the same program once more under -fsanitize=address,undefined;
- the rounding bound of the GPU test without the kernel: the float32 restatement stays inside it;
- the public surface: names, C symbols, header text, the argument errors (raised on CPU tensors, before any device
  call) and the C entry points' validation with pointers that are never dereferenced."""
import ctypes
import itertools
import os
import struct

import numpy as np
import pytest
import torch

import energy_ref as ref
import native_build

HERE = os.path.dirname(os.path.abspath(__file__))
shapes = pytest.mark.parametrize("shape", ref.HOST_SHAPES, ids=str)
kinds = pytest.mark.parametrize("kind", ref.KINDS)
spacings = pytest.mark.parametrize("spacing", ref.SPACINGS, ids=str)


# ---- the reference against a pure-torch restatement

def torch_energy(u, kind, h):
    """E (N,) from slicing differences of a torch tensor u (N, C, *sp): what could be written before the kernels."""
    d = u.dim() - 2

    def fwd(t, a):
        n = t.size(2 + a)
        return (t.narrow(2 + a, 1, n - 1) - t.narrow(2 + a, 0, n - 1)) / h[a] if n > 1 else t.narrow(2 + a, 0, 0)

    def sec(t, a):
        n = t.size(2 + a)
        if n < 3:
            return t.narrow(2 + a, 0, 0)
        return (t.narrow(2 + a, 2, n - 2) - 2 * t.narrow(2 + a, 1, n - 2) + t.narrow(2 + a, 0, n - 2)) / h[a] ** 2

    def ssq(t):
        return t.pow(2).flatten(1).sum(1)

    if kind == "diffusion":
        e = sum(ssq(fwd(u, a)) for a in range(d))
    else:
        e = sum(ssq(sec(u, a)) for a in range(d))
        for a, b in itertools.combinations(range(d), 2):
            e = e + 2 * ssq(fwd(fwd(u, a), b))
    return e / float(np.prod(u.shape[2:]))


@spacings
@kinds
@shapes
def test_reference_equals_the_torch_restatement(shape, kind, spacing):
    h = ref.spacing_tuple(spacing, len(shape))
    u = ref.field(2, 3, shape, np.float64)
    t = torch.from_numpy(u).requires_grad_(True)
    E = torch_energy(t, kind, h)
    want_E = ref.energy(u, kind, spacing)
    assert np.abs(E.detach().numpy() - want_E).max() <= 1e-12 * max(np.abs(want_E).max(), 1e-300)
    g, = torch.autograd.grad(E.sum(), t, allow_unused=True)
    g = np.zeros_like(u) if g is None else g.numpy()
    V = float(np.prod(shape))
    want_A = ref.operator(u, kind, spacing)
    assert np.abs(0.5 * V * g - want_A).max() <= 1e-12 * max(np.abs(want_A).max(), 1e-300)
    if kind == "diffusion" and max(shape) > 1 or kind == "bending" and sorted(shape)[-1] > 2:
        assert want_E.min() > 0 and np.abs(want_A).max() > 0


# ---- known answers

def _grid(shape, dtype=np.float64):
    return np.meshgrid(*[np.arange(n, dtype=dtype) for n in shape], indexing="ij")


def test_constant_and_affine_fields_have_exactly_no_energy():
    for shape in ((4, 5, 6), (7, 9)):
        for dtype in (np.float32, np.float64):
            c = np.full((1, 2) + shape, 3.25, dtype=dtype)
            assert (ref.energy(c, "diffusion") == 0).all() and (ref.density_native(c, "diffusion") == 0).all()
            assert (ref.operator(c, "diffusion") == 0).all() and (ref.operator_native(c, "diffusion") == 0).all()
            x = _grid(shape, dtype)
            aff = (sum((a + 2) * x[a] for a in range(len(shape))) - 3 * x[0] + 4)[None, None].astype(dtype)
            assert (ref.energy(aff, "bending") == 0).all() and (ref.operator(aff, "bending") == 0).all()
            assert aff.dtype == dtype and (ref.density_native(aff, "bending") == 0).all() and (ref.operator_native(aff, "bending") == 0).all()
            assert float(ref.density_native(aff, "bending", (1.0, 1.5, 0.7)).astype(np.float64).sum()) == 0.0


def test_quadratic_and_linear_fields():
    x = _grid((6, 7, 8))
    q = (x[0] ** 2 + x[0] * x[1])[None, None]
    # d_xx = 2 on the 4 interior x planes; d_xy = 1 where x + 1 < 6 and y + 1 < 7
    assert ref.energy(q, "bending")[0] == (4 * 4 * 7 * 8 + 2 * 5 * 6 * 8) / 336
    c = (0.5, -1.25, 2.0)
    lin = (c[0] * x[0] + c[1] * x[1] + c[2] * x[2] + 4.0)[None, None]
    want = sum(ca ** 2 * (n - 1) / n for ca, n in zip(c, (6, 7, 8)))
    assert abs(ref.energy(lin, "diffusion")[0] - want) <= 1e-14 * want
    lin2 = np.concatenate([lin, 2 * lin], axis=1)   # channels add
    assert abs(ref.energy(lin2, "diffusion")[0] - 5 * want) <= 1e-14 * want
    h = (1.0, 1.5, 0.7)
    want_h = sum((ca / ha) ** 2 * (n - 1) / n for ca, ha, n in zip(c, h, (6, 7, 8)))
    assert abs(ref.energy(lin, "diffusion", h)[0] - want_h) <= 1e-14 * want_h


def test_interior_stencils():
    def lap(v, axes):
        r = -2.0 * len(axes) * v
        for a in axes:
            r = r + np.roll(v, 1, a) + np.roll(v, -1, a)
        return r

    for shape in ((9, 8, 10), (9, 11)):
        u = ref.field(1, 1, shape, np.float64, seed=3)
        axes = tuple(range(2, 2 + len(shape)))
        inner = lambda w: (slice(None), slice(None)) + (slice(w, -w),) * len(shape)   # noqa: E731
        A = ref.operator(u, "diffusion")
        assert np.abs(A + lap(u, axes))[inner(1)].max() <= 1e-13
        B = ref.operator(u, "bending")
        assert np.abs(B - lap(lap(u, axes), axes))[inner(2)].max() <= 1e-12
        assert np.abs(B - lap(lap(u, axes), axes))[inner(1)].max() > 1e-3   # ... and not one voxel further out


@spacings
@kinds
@shapes
def test_symmetry_and_the_quadratic_form(shape, kind, spacing):
    u, v = ref.field(2, 2, shape, np.float64, seed=1), ref.field(2, 2, shape, np.float64, seed=2)
    Au, Av = ref.operator(u, kind, spacing), ref.operator(v, kind, spacing)
    scale = (np.abs(v) * ref.abs_operator(u, kind, spacing)).sum()
    assert abs((v * Au).sum() - (u * Av).sum()) <= 1e-13 * max(scale, 1e-300)
    E = ref.energy(u, kind, spacing)
    quad = (u * Au).reshape(2, -1).sum(1) / float(np.prod(shape))
    assert np.abs(E - quad).max() <= 1e-13 * max((np.abs(u) * ref.abs_operator(u, kind, spacing)).sum() / np.prod(shape), 1e-300)
    assert (E >= 0).all() and (ref.abs_operator(u, kind, spacing) >= np.abs(Au) * (1 - 1e-12)).all()


# ---- the header against the reference

def _cases():
    """(kind id, shape, spacing, dtype, plane, whether the plane is affine plus small noise) for every plane the emulation runs."""
    out = []
    for shape in ref.HOST_SHAPES:
        for spacing in ref.SPACINGS:
            for k, kind in enumerate(ref.KINDS):
                for dtype in (np.float32, np.float64):
                    out.append((k, shape, spacing, dtype, ref.field(1, 1, shape, dtype, seed=5), False))
                out.append((k, shape, spacing, np.float32, ref.field(1, 1, shape, np.float32, seed=6, affine=True), True))
    return out


def _run_emul(tmp_path, name, cases, extra=()):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for k, shape, spacing, dtype, u, affine in cases:
            d = len(shape)
            n = (1,) * (3 - d) + tuple(shape)
            h = (1.0,) * (3 - d) + ref.spacing_tuple(spacing, d)
            f.write(struct.pack("<6i3d", k, d, *n, np.dtype(dtype).itemsize, *h))
            f.write(u.tobytes())
    native_build.run(native_build.build(tmp_path, "energy_emul.cpp", extra=extra, name=name), src, dst, quiet=True)
    return open(dst, "rb").read()


def _check_emul(raw, cases):
    at = 0
    for k, shape, spacing, dtype, u, affine in cases:
        kind, nv = ref.KINDS[k], int(np.prod(shape))
        dens = np.frombuffer(raw, dtype=dtype, count=nv, offset=at).reshape(u.shape)
        at += dens.nbytes
        op = np.frombuffer(raw, dtype=dtype, count=nv, offset=at).reshape(u.shape)
        at += op.nbytes
        want_A, want_E = ref.operator(u, kind, spacing), ref.energy(u, kind, spacing)[0]
        if dtype == np.float64:
            assert np.abs(op - want_A).max() <= 1e-12 * max(np.abs(want_A).max(), 1e-300), (kind, shape, spacing)
            assert abs(dens.sum() / nv - want_E) <= 1e-12 * max(want_E, 1e-300), (kind, shape, spacing)
        else:
            assert np.array_equal(dens, ref.density_native(u, kind, spacing)), (kind, shape, spacing)
            assert np.array_equal(op, ref.operator_native(u, kind, spacing)), (kind, shape, spacing)
            if not affine:   # (there the energy is the noise's alone, small against the roundings of the affine part)
                assert abs(dens.astype(np.float64).sum() / nv - want_E) <= 1e-5 * want_E
    assert at == len(raw)


@native_build.needs_cxx
def test_header_emulation_equals_the_reference(tmp_path):
    cases = _cases()
    _check_emul(_run_emul(tmp_path, "energy_emul", cases), cases)


@native_build.needs_cxx
def test_header_emulation_under_the_sanitizers(tmp_path):
    """The same stand-alone host program with AddressSanitizer and UndefinedBehaviorSanitizer."""
    cases = _cases()
    _check_emul(_run_emul(tmp_path, "energy_emul_san", cases, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")), cases)


# ---- the bound, without the kernel

@kinds
@pytest.mark.parametrize("shape", ref.HOST_SHAPES + ref.THIN_SHAPES, ids=str)
def test_float32_restatement_stays_inside_the_bound(shape, kind):
    worst = 0.0
    for spacing in ref.SPACINGS:
        for affine in (False, True):
            u = ref.field(2, 3, shape, np.float32, affine=affine)
            got = ref.operator_native(u, kind, spacing).astype(np.float64)
            want = ref.operator(u, kind, spacing)
            worst = max(worst, ref.worst_ratio(np.abs(got - want), ref.operator_bound(u, kind, spacing)))
            if not affine and np.abs(want).max() > 0:
                assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
            if not affine:
                E = ref.density_native(u, kind, spacing).astype(np.float64).reshape(2, -1).sum(1) / np.prod(shape)
                want_E = ref.energy(u, kind, spacing)
                assert (np.abs(E - want_E) <= 1e-5 * want_E).all()
    print(f"{shape} {kind}: float32 restatement at most {worst:.3f} of the operator bound")
    assert worst <= 1.0


# ---- the public surface

def test_names_symbols_and_abi_version():
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext, regularize

    for name in ("diffusion_energy", "bending_energy", "field_energy", "energy_operator", "FieldEnergyFunction", "EnergyOperatorFunction"):
        assert getattr(lm, name) is getattr(regularize, name) and getattr(lm, name).__doc__
    lib = ctypes.CDLL(ext.LIB_PATH)
    for stem in ("lago_field_energy", "lago_field_energy_operator"):
        for suf in ("_f32", "_f64"):
            assert hasattr(lib, stem + suf) and stem + suf in ext._fn, stem + suf
    assert hasattr(lib, "lago_field_energy_scratch_elems")
    assert lib.lago_abi_version() == ext.ABI_VERSION == 5
    header = open(os.path.join(os.path.dirname(HERE), "include", "lagomorph_hip.h")).read()
    block = header[header.index("#define LAGO_DECLARE(REAL, SUF)"):header.index("LAGO_DECLARE(float, _f32)")]
    for text in ("lago_field_energy##SUF(", "lago_field_energy_operator##SUF("):
        assert text in block, text
    for text in ("long long lago_field_energy_scratch_elems(", "#define LAGO_ABI_VERSION 5", "#define LAGO_ENERGY_DIFFUSION 0",
                 "#define LAGO_ENERGY_BENDING 1"):
        assert text in header and text not in block, text
    for doc in (regularize.__doc__, lm.field_energy.__doc__, lm.energy_operator.__doc__, header):
        assert "call to call" in doc
    public = {n for n, f in vars(ext).items() if callable(f) and getattr(f, "__module__", None) == ext.__name__ and not n.startswith("_")}
    assert not {n for n in public if "energy" in n}   # the shim gained no public function


def test_argument_errors_are_raised_on_cpu_tensors():
    import lagomorph_amd as lm

    u, u2 = torch.zeros((2, 3, 5, 6, 7)), torch.zeros((2, 1, 9, 11))
    calls = ((lambda x, *a, **k: lm.diffusion_energy(x, *a, **k)), (lambda x, *a, **k: lm.bending_energy(x, *a, **k)),
             (lambda x, *a, **k: lm.field_energy(x, "bending", *a, **k)), (lambda x, *a, **k: lm.energy_operator(x, "diffusion", *a, **k)))
    for f in calls:
        for bad in (u.numpy(), None, [1.0]):
            with pytest.raises(TypeError):
                f(bad)
        for bad in (u.half(), u.int(), u.long()):
            with pytest.raises(RuntimeError, match="float32 and float64"):
                f(bad)
        for bad in (torch.zeros((2, 3, 4)), torch.zeros((5,)), torch.zeros((2, 3, 4, 5, 6, 7))):
            with pytest.raises(RuntimeError, match="two or three spatial axes"):
                f(bad)
        for bad in (0, -1.0, float("inf"), float("nan"), (1.0, 2.0), (1.0, 2.0, 3.0, 4.0), (1.0, 0.0, 1.0), "1", None, True, (1.0, "2", 1.0)):
            with pytest.raises(RuntimeError, match="spacing"):
                f(u, bad)
        with pytest.raises(RuntimeError, match="contiguous"):
            f(u.transpose(2, 3).contiguous().transpose(2, 3))
        for args in ((u,), (u.double(), 2), (u.clone().requires_grad_(True), (1.0, 1.5, 0.7)), (u2, [1.0, 2.5]), (u2, np.float32(0.5))):
            with pytest.raises(RuntimeError, match="CUDA tensor"):   # all fine but for the device
                f(*args)
    for bad in ("elastic", 0, None, "Bending"):
        with pytest.raises(RuntimeError, match="kind"):
            lm.field_energy(u, bad)
        with pytest.raises(RuntimeError, match="kind"):
            lm.energy_operator(u, bad)
    with pytest.raises(TypeError):
        lm.energy_operator(u, "bending", scale=[1.0, 1.0])
    for bad in (torch.ones(3), torch.ones(2, 1), torch.ones(2, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="scale"):
            lm.energy_operator(u, "bending", scale=bad)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        lm.energy_operator(u, "bending", scale=torch.ones(2))


def test_c_entry_points_validate_before_any_device_call():
    from lagomorph_amd import lagomorph_ext as ext

    OK, INVALID = 0, -1
    p, q, r = 0x100000, 0x4000000, 0x8000000   # never dereferenced: every call returns before a launch
    err = ext._lib.lago_last_error
    elems = ext._lib.lago_field_energy_scratch_elems
    h = (ctypes.c_double * 3)(1.0, 1.5, 0.7)
    tx, ty, tz = ref.TILE3
    assert elems(1, 3, 2, 3, 5, 6, 7) == 2 * 3 and elems(0, 3, 2, 3, tx + 1, ty, 2 * tz + 1) == 2 * 3 * 2 * 1 * 3
    assert elems(1, 2, 2, 1, ref.TILE2[0] + 1, ref.TILE2[1] + 2, 1) == 2 * 1 * 2 * 2
    assert elems(1, 3, 0, 3, 5, 6, 7) == 0 and elems(1, 3, 2, 0, 5, 6, 7) == 0 and elems(1, 3, 2, 3, 5, 0, 7) == 0
    assert elems(1, 4, 2, 3, 5, 6, 7) == -1 and elems(2, 3, 2, 3, 5, 6, 7) == -1 and elems(1, 3, 2, 3, 5, -6, 7) == -1
    need = elems(1, 3, 2, 3, 5, 6, 7)
    for suf in ("_f32", "_f64"):
        f = ext._fn["lago_field_energy" + suf]
        g = ext._fn["lago_field_energy_operator" + suf]
        tail = (2, 3, 5, 6, 7, h, None)
        for call, what in ((lambda *a: f(p, q, r, need, *a), "energy"), (lambda *a: g(p, q, None, *a), "operator")):
            assert call(1, 4, 2, 3, 5, 6, 7, h, None) == INVALID and b"dimensional" in err(), what
            assert call(1, 1, 2, 3, 5, 6, 7, h, None) == INVALID and b"dimensional" in err()
            for kind in (2, -1):
                assert call(kind, 3, *tail) == INVALID and b"kind" in err()
            assert call(1, 3, 2, 3, 5, -6, 7, h, None) == INVALID and b"negative" in err()
            assert call(0, 3, -2, 3, 5, 6, 7, h, None) == INVALID and b"negative" in err()
            assert call(0, 3, 2, -3, 5, 6, 7, h, None) == INVALID and b"negative" in err()
            assert call(1, 3, 2, 3, 1 << 10, 1 << 10, 1 << 9, h, None) == INVALID and b"2^29" in err()
            assert call(1, 2, 2, 3, 1 << 15, 1 << 14, 1, h, None) == INVALID and b"2^29" in err()
            for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
                assert call(1, 3, 2, 3, 5, 6, 7, (ctypes.c_double * 3)(*bad), None) == INVALID and b"spacing" in err(), bad
            assert call(1, 2, 2, 3, 5, 6, 1, (ctypes.c_double * 2)(1.0, 0.0), None) == INVALID and b"spacing" in err()
            assert call(1, 3, 2, 3, 5, 6, 7, None, None) == INVALID and b"null" in err()
        assert f(None, q, r, need, 1, 3, *tail) == INVALID and b"null" in err()
        assert f(p, None, r, need, 1, 3, *tail) == INVALID and b"null" in err()
        assert f(p, q, None, need, 1, 3, *tail) == INVALID and b"null" in err()
        assert f(p, q, r, need - 1, 1, 3, *tail) == INVALID and b"scratch" in err()
        assert f(p, q, r, 0, 0, 3, *tail) == INVALID and b"scratch" in err()
        assert f(p, q, q + 8, need, 1, 3, *tail) == INVALID and b"overlap" in err()    # scratch / u
        assert f(q + 16, q, r, need, 1, 3, *tail) == INVALID and b"overlap" in err()   # energy / u
        assert g(None, q, None, 1, 3, *tail) == INVALID and b"null" in err()
        assert g(p, None, None, 1, 3, *tail) == INVALID and b"null" in err()
        assert g(p, p, None, 1, 3, *tail) == INVALID and b"overlap" in err()
        assert g(p, p + 64, None, 0, 3, *tail) == INVALID and b"overlap" in err()
        assert g(p, q, p + 8, 0, 3, *tail) == INVALID and b"overlap" in err()          # out / scale
        for ext_ in ((0, 3, 5, 6, 7), (2, 0, 5, 6, 7), (2, 3, 0, 6, 7), (2, 3, 5, 0, 7), (2, 3, 5, 6, 0)):   # empty: nothing to do
            assert f(None, None, None, 0, 1, 3, *ext_, h, None) == OK
            assert g(None, None, None, 0, 3, *ext_, h, None) == OK
        assert f(None, None, None, 0, 1, 2, 2, 3, 5, 0, 0, h, None) == OK
