"""CPU: the specification of ffd_expand and ffd_restrict before any GPU run.

- tests/ffd_ref.py, the numpy reference: its per-axis matrix W against scipy's B-spline basis elements at 2e-16, the
  rows summing to 1, a linear lattice expanding to the same linear function, the unused last control column when
  (n - 1) % s == 0, and <W c, g> = <c, W^T g>;
- lagomorph_amd/csrc/ffd_weights.hpp, the header the kernels call: tests/native/ffd_emul.cpp runs it over every (r, s)
  with a plain host compiler, and t and the weights equal the numpy restatement bit for bit in both precisions; the same
  program once more under -fsanitize=address,undefined;
- the bounds of the GPU test without the kernel: a float32 numpy run of the kernels' own expressions and orders stays
  inside ffd_ref.voxel_bound and ffd_ref.entry_bound on the GPU test's inputs;
- the public surface: names, C symbols, header text, the argument errors (raised on CPU tensors, before any device
  call) and the C entry points' validation with pointers that are never dereferenced."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ffd_ref as ref
import native_build

HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = ((5, 2), (6, 3), (7, 4), (3, 8), (9, 4), (11, 1), (1, 5), (70, 5), (41, 7))


# ---- the reference against scipy and against facts that need no scipy

@pytest.mark.parametrize("n,s", PAIRS, ids=str)
def test_reference_matrix_is_scipys_basis_elements(n, s):
    BSpline = pytest.importorskip("scipy.interpolate").BSpline
    M = ref.W(n, s)
    m = (n - 1) // s + 4
    assert M.shape == (n, m)
    x = np.arange(n, dtype=np.float64)
    for j in range(m):
        knots = np.arange(j - 3, j + 2, dtype=np.float64) * s
        want = np.nan_to_num(BSpline.basis_element(knots, extrapolate=False)(x))
        assert np.abs(M[:, j] - want).max() <= 2e-16, (n, s, j)


@pytest.mark.parametrize("n,s", PAIRS, ids=str)
def test_reference_matrix_facts(n, s):
    M = ref.W(n, s)
    m = M.shape[1]
    assert m == (n - 1) // s + 4 == ref.grid_shape((n,), (s,))[0]
    assert np.abs(M.sum(1) - 1.0).max() <= 4e-16 and (M >= 0).all()
    assert ((M != 0).sum(1) <= 4).all()
    a, b = 0.75, -2.5
    lattice = a * (np.arange(m) - 1.0) * s + b   # control point j at voxel (j - 1) s
    assert np.abs(M @ lattice - (a * np.arange(n) + b)).max() <= 1e-13 * max(1.0, abs(a) * n + abs(b))
    if (n - 1) % s == 0:
        assert (M[:, m - 1] == 0).all()
    else:
        assert (M[:, m - 1] != 0).any()
    assert (M[:, : m - 1] != 0).any(0).all()   # every other column is reached


@pytest.mark.parametrize("shape,spacing", ref.CASES[:5], ids=str)
def test_reference_adjoint_identity(shape, spacing):
    m = ref.grid_shape(shape, spacing)
    c, g = ref.field(2, 2, m, np.float64), ref.field(2, 2, shape, np.float64, seed=1)
    lhs, rhs = (ref.expand(c, shape, spacing) * g).sum(), (c * ref.adjoint(g, spacing)).sum()
    scale = (ref.expand(np.abs(c), shape, spacing) * np.abs(g)).sum()
    assert abs(lhs - rhs) <= 1e-12 * scale
    # the last control plane of an axis with (n - 1) % s == 0 receives exactly nothing
    d_c = ref.adjoint(g, spacing)
    for a, (n, s) in enumerate(zip(shape, ref.spacing_tuple(spacing, len(shape)))):
        if (n - 1) % s == 0:
            assert (np.take(d_c, m[a] - 1, axis=2 + a) == 0).all()


# ---- the header against the reference

def _run_emul(tmp_path, name, extra=()):
    dst = str(tmp_path / "out.bin")
    native_build.run(native_build.build(tmp_path, "ffd_emul.cpp", extra=extra, name=name), dst, quiet=True)
    return open(dst, "rb").read()


def _check_emul(raw):
    at, pairs = 0, sum(range(1, ref.MAX_SPACING + 1))
    for dtype in (np.float32, np.float64):
        got = np.frombuffer(raw, dtype=dtype, count=pairs * 5, offset=at).reshape(-1, 5)
        at += got.nbytes
        bits = np.uint32 if dtype == np.float32 else np.uint64
        row = 0
        for s in range(1, ref.MAX_SPACING + 1):
            t, w = ref.weights_native(np.arange(s), s, dtype)
            assert t.dtype == np.dtype(dtype) and w.dtype == np.dtype(dtype)
            mine = got[row:row + s]
            assert np.array_equal(mine[:, 0].view(bits), t.view(bits)), (dtype, s)
            assert np.array_equal(mine[:, 1:].view(bits), np.ascontiguousarray(w.T).view(bits)), (dtype, s)
            assert mine[0, 0] == 0 and mine[0, 4] == 0 and (mine[:, 0] < 1).all()   # r = 0: t = 0 and w_3 exactly 0
            # ... and these are the reference's weights: within 8 u of the float64 cubic at the same t
            exact = ref.bspline_ref.weights(t, np.longdouble)
            rel = np.abs(w.astype(np.longdouble) - exact)[exact != 0] / exact[exact != 0]
            assert rel.max() <= 8 * ref.UNIT[np.dtype(dtype)] and (w[exact == 0] == 0).all()
            row += s
        assert row == pairs
    m = np.frombuffer(raw, dtype="<i8", count=ref.MAX_SPACING * 200, offset=at).reshape(ref.MAX_SPACING, 200)
    at += m.nbytes
    assert at == len(raw)
    for s in range(1, ref.MAX_SPACING + 1):
        assert np.array_equal(m[s - 1], (np.arange(1, 201) - 1) // s + 4)


@native_build.needs_cxx
def test_header_emulation_equals_the_reference_exactly(tmp_path):
    _check_emul(_run_emul(tmp_path, "ffd_emul"))


@native_build.needs_cxx
def test_header_emulation_under_the_sanitizers(tmp_path):
    """The same stand-alone host program with AddressSanitizer and UndefinedBehaviorSanitizer."""
    _check_emul(_run_emul(tmp_path, "ffd_emul_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")))


# ---- the bounds, without the kernel

@pytest.mark.parametrize("shape,spacing", ref.CASES, ids=str)
def test_float32_restatement_stays_inside_the_bounds(shape, spacing):
    """The kernels' expressions and orders in float32 numpy against the float64 reference: inside voxel_bound
    (forward) and entry_bound (adjoint) on the GPU test's inputs."""
    d, m = len(shape), ref.grid_shape(shape, spacing)
    worst_f = worst_a = 0.0
    for C in sorted({1, d, 4}):
        c = ref.field(2, C, m, np.float32)
        got = ref.expand_native(c, shape, spacing)
        assert got.dtype == np.float32
        worst_f = max(worst_f, ref.worst_ratio(got.astype(np.float64) - ref.expand(c, shape, spacing), ref.voxel_bound(c, shape, spacing, np.float32)))
        g = ref.field(2, C, shape, np.float32, seed=7)
        got = ref.adjoint_native(g, spacing)
        assert got.dtype == np.float32 and got.shape[2:] == m
        worst_a = max(worst_a, ref.worst_ratio(got.astype(np.float64) - ref.adjoint(g, spacing), ref.entry_bound(g, spacing, np.float32)))
    print(f"{shape} / {spacing}: float32 restatement at most {worst_f:.3f} of the voxel bound, {worst_a:.3f} of the entry bound")
    assert 0.0 < worst_f <= 1.0 and 0.0 < worst_a <= 1.0


# ---- the public surface

def test_names_symbols_and_abi_version():
    import lagomorph_amd as lm
    from lagomorph_amd import ffd, lagomorph_ext as ext

    for name in ("ffd_expand", "ffd_restrict", "ffd_grid_shape", "FFDFunction"):
        assert getattr(lm, name) is getattr(ffd, name) and getattr(lm, name).__doc__
    assert callable(ext.ffd_expand) and callable(ext.ffd_expand_adjoint) and callable(ext._check_ffd)
    assert lm.ffd_grid_shape((5, 6, 7), (2, 3, 4)) == (6, 5, 5) and lm.ffd_grid_shape((9, 11), 4) == (6, 6)
    assert lm.ffd_grid_shape(torch.Size((1, 33)), 32) == (4, 5)
    lib = ctypes.CDLL(ext.LIB_PATH)
    for stem in ("lago_ffd_expand", "lago_ffd_expand_adjoint"):
        for suf in ("_f32", "_f64"):
            assert hasattr(lib, stem + suf) and stem + suf in ext._fn, stem + suf
    assert hasattr(lib, "lago_ffd_scratch_elems")
    assert lib.lago_abi_version() == ext.ABI_VERSION == 5
    header = open(os.path.join(os.path.dirname(HERE), "include", "lagomorph_hip.h")).read()
    for text in ("lago_ffd_expand##SUF(", "lago_ffd_expand_adjoint##SUF(", "long long lago_ffd_scratch_elems(", "#define LAGO_ABI_VERSION 5"):
        assert text in header, text
    for doc in (ffd.ffd_expand.__doc__, ffd.ffd_restrict.__doc__, ext.ffd_expand.__doc__, ext.ffd_expand_adjoint.__doc__, header):
        assert "call to call" in doc
    assert "(j - 1) s" in ffd.__doc__ and "voxel" in ffd.__doc__


def test_argument_errors_are_raised_on_cpu_tensors():
    import lagomorph_amd as lm

    shape, sp = (5, 6, 7), (2, 3, 4)
    c = torch.zeros((2, 3) + lm.ffd_grid_shape(shape, sp))
    c2 = torch.zeros((2, 1) + lm.ffd_grid_shape((9, 11), (4, 1)))
    g, g2 = torch.zeros((2, 3) + shape), torch.zeros((2, 1, 9, 11))
    for bad in (c.numpy(), None, [1.0]):
        with pytest.raises(TypeError):
            lm.ffd_expand(bad, shape, sp)
        with pytest.raises(TypeError):
            lm.ffd_restrict(bad, sp)
    for f, x, args in ((lm.ffd_expand, c, (shape, sp)), (lm.ffd_restrict, g, (sp,))):
        for bad in (x.half(), x.int(), x.long()):
            with pytest.raises(RuntimeError, match="float32 and float64"):
                f(bad, *args)
        for bad in (torch.zeros((2, 3, 4)), torch.zeros((5,)), torch.zeros((2, 3, 4, 5, 6, 7))):
            with pytest.raises(RuntimeError, match="two or three spatial axes"):
                f(bad, *args)
        for bad in (0, 33, -1, (2, 3), (2, 3, 4, 5), (2, 3, 0), (2, 3, 33), 2.0, (2, 3, 4.0), "4", None, True):
            with pytest.raises(RuntimeError, match="spacing"):
                f(x, *args[:-1], bad)
        with pytest.raises(RuntimeError, match="contiguous"):
            f(x.transpose(2, 3).contiguous().transpose(2, 3), *args)
        for xx in (x, x.double(), x.clone().requires_grad_(True)):
            with pytest.raises(RuntimeError, match="CUDA tensor"):   # all fine but for the device
                f(xx, *args)
    # control extents against shape and spacing
    for bad_shape, bad_sp in (((5, 6, 9), sp), ((5, 6, 7), (2, 3, 2)), ((5, 6), (2, 3)), ((4, 6, 7), sp), ((5, 6, 7), 1)):
        with pytest.raises(RuntimeError, match="does not match"):
            lm.ffd_expand(c, bad_shape, bad_sp)
    with pytest.raises(RuntimeError, match="does not match"):
        lm.ffd_expand(c[..., :-1].contiguous(), shape, sp)
    with pytest.raises(RuntimeError, match="does not match"):
        lm.ffd_expand(c2, (9, 12), (4, 1))
    for ok in ((c2, (9, 11), (4, 1)), (c2, torch.Size((9, 11)), [4, 1])):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            lm.ffd_expand(*ok)
    for ok in ((g2, (4, 1)), (g2, 32), (g, 1)):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            lm.ffd_restrict(*ok)
    for bad in ((5, 0, 7), (5, 6), (5, -1, 7), 7, (5.0, 6, 7)):
        with pytest.raises(RuntimeError):
            lm.ffd_grid_shape(bad, 2 if bad != (5, 6) else (1, 2, 3))


def test_c_entry_points_validate_before_any_device_call():
    from lagomorph_amd import lagomorph_ext as ext

    OK, INVALID = 0, -1
    p, q, r = 0x100000, 0x4000000, 0x8000000   # never dereferenced: every call returns before a launch
    err = ext._lib.lago_last_error
    elems = ext._lib.lago_ffd_scratch_elems
    need = elems(3, 2, 5, 6, 7, 2, 3, 4)
    assert need == 2 * 1 * ((8 + 0) // 2 + 4) * ((8 + 1) // 3 + 4) * ((64 + 2) // 4 + 4)   # rows x tiles x the box of a tile
    assert elems(2, 1, 97, 70, 1, 32, 7, 1) == 2 * 2 * ((64 + 30) // 32 + 4) * ((64 + 5) // 7 + 4)
    assert elems(3, 0, 5, 6, 7, 2, 3, 4) == 0 and elems(3, 2, 5, 0, 7, 2, 3, 4) == 0
    assert elems(4, 2, 5, 6, 7, 2, 3, 4) == -1 and elems(3, 2, 5, 6, 7, 2, 0, 4) == -1 and elems(3, 2, 5, 6, 7, 2, 3, 33) == -1
    for suf in ("_f32", "_f64"):
        f = ext._fn["lago_ffd_expand" + suf]
        assert f(p, q, 4, 1, 5, 6, 7, 2, 3, 4, None) == INVALID and b"dimensional" in err()
        assert f(p, q, 1, 1, 5, 6, 7, 2, 3, 4, None) == INVALID and b"dimensional" in err()
        assert f(p, q, 3, 1, 5, -6, 7, 2, 3, 4, None) == INVALID and b"negative" in err()
        assert f(p, q, 3, -1, 5, 6, 7, 2, 3, 4, None) == INVALID and b"negative" in err()
        for bad in ((0, 3, 4), (2, 33, 4), (2, 3, -1), (2, 3, 33)):
            assert f(p, q, 3, 1, 5, 6, 7, *bad, None) == INVALID and b"spacing" in err()
        assert f(p, q, 2, 1, 5, 6, 1, 2, 33, 1, None) == INVALID and b"spacing" in err()
        assert f(p, q, 3, 1, 1 << 10, 1 << 10, 1 << 9, 2, 3, 4, None) == INVALID and b"2^29" in err()
        assert f(p, q, 2, 1, 1 << 15, 1 << 14, 1, 2, 3, 1, None) == INVALID and b"2^29" in err()
        assert f(None, q, 3, 1, 5, 6, 7, 2, 3, 4, None) == INVALID and b"null" in err()
        assert f(p, None, 3, 1, 5, 6, 7, 2, 3, 4, None) == INVALID and b"null" in err()
        assert f(p, p, 3, 1, 5, 6, 7, 2, 3, 4, None) == INVALID and b"overlap" in err()
        assert f(p, p + 64, 3, 2, 5, 6, 7, 2, 3, 4, None) == INVALID and b"overlap" in err()
        for ext_ in ((0, 5, 6, 7), (1, 0, 6, 7), (1, 5, 0, 7), (1, 5, 6, 0)):   # empty: nothing to do
            assert f(None, None, 3, *ext_, 2, 3, 4, None) == OK
        assert f(None, None, 2, 1, 5, 0, 0, 2, 3, 0, None) == OK
        h = ext._fn["lago_ffd_expand_adjoint" + suf]
        assert h(p, q, r, need, 0, 2, 5, 6, 7, 2, 3, 4, None) == INVALID and b"dimensional" in err()
        assert h(p, q, r, need, 3, 2, 5, 6, -7, 2, 3, 4, None) == INVALID and b"negative" in err()
        assert h(p, q, r, need, 3, 2, 5, 6, 7, 2, 3, 0, None) == INVALID and b"spacing" in err()
        assert h(p, q, r, need, 3, 2, 1 << 10, 1 << 10, 1 << 9, 2, 3, 4, None) == INVALID and b"2^29" in err()
        assert h(None, q, r, need, 3, 2, 5, 6, 7, 2, 3, 4, None) == INVALID and b"null" in err()
        assert h(p, None, r, need, 3, 2, 5, 6, 7, 2, 3, 4, None) == INVALID and b"null" in err()
        assert h(p, q, None, need, 3, 2, 5, 6, 7, 2, 3, 4, None) == INVALID and b"null" in err()
        assert h(p, q, r, need - 1, 3, 2, 5, 6, 7, 2, 3, 4, None) == INVALID and b"scratch" in err()
        assert h(p, q, r, 0, 3, 2, 5, 6, 7, 2, 3, 4, None) == INVALID and b"scratch" in err()
        assert h(p, p + 8, r, need, 3, 2, 5, 6, 7, 2, 3, 4, None) == INVALID and b"overlap" in err()   # d_ctrl / grad_out
        assert h(p, q, p + 8, need, 3, 2, 5, 6, 7, 2, 3, 4, None) == INVALID and b"overlap" in err()   # d_ctrl / scratch
        assert h(p, q, q + 8, need, 3, 2, 5, 6, 7, 2, 3, 4, None) == INVALID and b"overlap" in err()   # scratch / grad_out
        for ext_ in ((0, 5, 6, 7), (2, 0, 6, 7), (2, 5, 0, 7), (2, 5, 6, 0)):
            assert h(None, None, None, 0, 3, *ext_, 2, 3, 4, None) == OK
