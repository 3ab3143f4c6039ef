"""CPU: the specification of distance_transform, signed_distance and surface_distance before any GPU run.

- tests/edt_ref.py, the numpy reference: its separable recurrence equals the brute-force minimum over all feature voxels
  in exact integers, scipy's distance_transform_edt and binary_erosion where scipy is installed, and the known answers
  (a single feature, two boxes, an item without features, an empty surface);
- lagomorph_amd/csrc/edt_line.hpp, the header the kernels call: tests/native/edt_emul.cpp runs every line of every case
  through its functions in float32 with a plain host compiler; at unit spacing the result equals the reference bit for
  bit, otherwise it is within 8 * 2^-24 relative; the same program is run once more built with
  -fsanitize=address,undefined;
- the public surface: names, the C symbol, and the argument errors (raised on CPU tensors, before any device call)."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import edt_ref as ref
import native_build

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((5, 6, 7), (7, 9), (1, 9), (2, 2, 2))
SPACING = (1.5, 0.7, 2.0)
REL = 8 * 2.0 ** -24   # float32 against the real value: one rounding for s delta, one for the square, one per addition
                       # over three axes, and the spacing's own rounding to float32 (squared)


# ---- the reference against the definition

@pytest.mark.parametrize("sp", SHAPES)
def test_reference_equals_brute_force(sp):
    for kind in ref.KINDS:
        L = ref.labels(kind, 2, sp)
        for where in ref.WHERES:
            f = ref.features(L, where, 1)
            got, want = ref.edt_sq(f), ref.brute(f)
            assert got.dtype == np.int64 and np.array_equal(got, want), (kind, where)
            s = SPACING[-len(sp):]
            got, want = ref.edt_sq(f, s), ref.brute(f, s)
            assert np.array_equal(np.isinf(got), np.isinf(want)), (kind, where)
            fin = np.isfinite(want)
            assert np.allclose(got[fin], want[fin], rtol=1e-14, atol=0), (kind, where)


@pytest.mark.parametrize("sp", SHAPES + ((8, 16, 32), (1, 5, 4), (6, 1, 3)))
def test_reference_equals_scipy(sp):
    ndi = pytest.importorskip("scipy.ndimage")
    for kind in ref.KINDS:
        L = ref.labels(kind, 2, sp)
        for where in ref.WHERES:
            f = ref.features(L, where, 1)
            if where == "surface":
                m = L == 1
                want = np.stack([m[n, 0] & ~ndi.binary_erosion(m[n, 0], border_value=0) for n in range(2)])[:, None]
                assert np.array_equal(f, want), kind
            for n in range(2):
                if not f[n].any():   # scipy has no answer for an input without features
                    assert np.all(ref.edt_sq(f[n:n + 1]) == ref.NO_FEATURE)
                    continue
                d = ndi.distance_transform_edt(~f[n, 0])
                assert np.array_equal(ref.edt_sq(f[n:n + 1])[0, 0], np.rint(d * d).astype(np.int64)), (kind, where)
                s = SPACING[-len(sp):]
                d = ndi.distance_transform_edt(~f[n, 0], sampling=s)
                assert np.allclose(np.sqrt(ref.edt_sq(f[n:n + 1], s)[0, 0]), d, rtol=1e-12, atol=0), (kind, where)


# ---- known answers

@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9)])
def test_single_feature_gives_the_analytic_field(sp):
    L = np.zeros((1, 1) + sp, dtype=np.int32)
    at = tuple(s // 3 for s in sp)
    L[(0, 0) + at] = 5
    grid = np.indices(sp)
    want = sum((grid[a] - at[a]) ** 2 for a in range(len(sp)))
    assert np.array_equal(ref.edt_sq(ref.features(L, "equal", 5))[0, 0], want)
    assert np.array_equal(ref.edt_sq(ref.features(L, "surface", 5))[0, 0], want)   # a lone voxel is its own surface
    assert np.array_equal(ref.distance_transform(L, squared=True)[0, 0], want.astype(np.float32))
    assert np.array_equal(ref.distance_transform(L)[0, 0], np.sqrt(want.astype(np.float32)))
    assert ref.distance_transform(L).dtype == np.float32
    s = SPACING[-len(sp):]
    want = sum((s[a] * (grid[a] - at[a])) ** 2 for a in range(len(sp)))
    assert np.allclose(ref.edt_sq(ref.features(L, "nonzero"), s)[0, 0], want, rtol=1e-15, atol=0)


def test_no_feature_is_inf_and_only_in_that_item():
    L = ref.labels("sparse", 2, (5, 6, 7))
    L[1] = 0
    for s in (1.0, SPACING):
        d = ref.distance_transform(L, spacing=s)
        assert np.all(np.isfinite(d[0])) and np.all(d[1] == np.inf)
    assert np.all(ref.distance_transform(L, "equal", 9) == np.inf)
    assert np.all(ref.distance_transform(ref.labels("all", 2, (7, 9))) == 0)


@pytest.mark.parametrize("d", [2, 3])
def test_boxes_have_their_closed_form_surface_distances(d):
    A, B, hausdorff, assd = ref.concentric_boxes(d)
    r = ref.surface_distance(A, B, [1, 2], float32_distances=False)
    assert r["hausdorff"][0, 0] == hausdorff == np.sqrt((d - 1) * 9 + 16)
    assert abs(r["assd"][0, 0] - assd) <= 1e-12 * assd
    assert r["hausdorff"][0, 0] >= r["hd95"][0, 0] >= r["assd"][0, 0] > 0
    # symmetric, zero against itself, nan for a label without a surface in either map
    r2 = ref.surface_distance(B, A, [1])
    assert abs(r2["hausdorff"][0, 0] - hausdorff) < 1e-6 * hausdorff
    same = ref.surface_distance(A, A, [1])
    assert same["hausdorff"][0, 0] == 0 and same["hd95"][0, 0] == 0 and same["assd"][0, 0] == 0
    assert all(np.isnan(v[0, 1]) for v in r.values())
    onesided = ref.surface_distance(A, np.zeros_like(A), [1])
    assert all(np.isnan(v[0, 0]) for v in onesided.values())
    # twice the spacing, twice every distance
    r3 = ref.surface_distance(A, B, [1], spacing=2.0, float32_distances=False)
    assert abs(r3["hausdorff"][0, 0] - 2 * hausdorff) < 1e-12 and abs(r3["assd"][0, 0] - 2 * assd) < 1e-12


def test_signed_distance_of_a_box():
    L = ref.box((9, 9), (3, 3), (6, 6), label=4)
    for lab, M in ((4, L), (None, L)):
        sd = ref.signed_distance(M, lab)[0, 0]
        assert sd[4, 4] == -2 and sd[3, 4] == -1 and sd[2, 4] == 1 and sd[0, 0] == np.sqrt(18.0)
        assert np.array_equal(sd < 0, L[0, 0] == 4)
    assert np.all(ref.signed_distance(np.zeros_like(L), 4) == np.inf) and np.all(ref.signed_distance(L * 0 + 4, 4) == -np.inf)


# ---- the header against the reference

def _build_emul(tmp_path, name, extra=()):
    return native_build.build(tmp_path, "edt_emul.cpp", extra=extra, name=name)


def _emul_cases(shapes):
    from lagomorph_amd.lagomorph_ext import EDT_WHERE

    for sp in shapes:
        for kind in ref.KINDS:
            L = ref.labels(kind, 2, sp)
            for where in ref.WHERES:
                for s in (1.0, SPACING[-len(sp):]):
                    yield sp, L, where, EDT_WHERE[where], 1, s


def _run_emul(exe, tmp_path, cases):
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        for sp, L, where, code, label, s in cases:
            n = (1,) * (3 - len(sp)) + tuple(sp)
            s3 = (1.0,) * (3 - len(sp)) + ((s,) * len(sp) if np.ndim(s) == 0 else tuple(s))
            f.write(struct.pack("<7i3f", len(sp), L.shape[0], *n, code, label, *s3))
            f.write(np.ascontiguousarray(L, dtype="<i4").tobytes())
    native_build.run(exe, src, dst, quiet=True)
    raw, at = open(dst, "rb").read(), 0
    for sp, L, where, code, label, s in cases:
        feat = np.frombuffer(raw, dtype="<i4", count=L.size, offset=at).reshape(L.shape)
        sq = np.frombuffer(raw, dtype="<f4", count=L.size, offset=at + 4 * L.size).reshape(L.shape)
        at += 8 * L.size
        yield feat, sq
    assert at == len(raw)


def _check_emul(cases, results):
    exact = 0
    for (sp, L, where, code, label, s), (feat, sq) in zip(cases, results):
        what = (sp, where, s)
        f = ref.features(L, where, label)
        assert np.array_equal(feat != 0, f), what
        want = ref.as_float(ref.edt_sq(f, s))
        if np.ndim(s) == 0:
            assert np.array_equal(sq.view(np.uint32), want.astype(np.float32).view(np.uint32)), what
            exact += 1
        else:
            assert np.array_equal(np.isinf(sq), np.isinf(want)), what
            fin = np.isfinite(want)
            assert np.all(np.abs(sq[fin].astype(np.float64) - want[fin]) <= REL * want[fin]), what
    return exact


@native_build.needs_cxx
def test_header_emulation_equals_the_reference(tmp_path):
    cases = list(_emul_cases(SHAPES + ((8, 16, 32), (1, 5, 4), (6, 1, 3), (33, 9, 10), (3, 70))))
    assert len(cases) > 400
    exact = _check_emul(cases, _run_emul(_build_emul(tmp_path, "edt_emul"), tmp_path, cases))
    assert exact == len(cases) // 2


@native_build.needs_cxx
def test_header_emulation_under_the_sanitizers(tmp_path):
    """The same stand-alone host program with AddressSanitizer and UndefinedBehaviorSanitizer: the clamped neighbour
    indices of the surface stencil stay inside the label map at every border, thin extents included."""
    cases = list(_emul_cases(SHAPES + ((1, 5, 4), (6, 1, 3))))
    exe = _build_emul(tmp_path, "edt_emul_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    _check_emul(cases, _run_emul(exe, tmp_path, cases))


# ---- the public surface

def test_names_symbol_and_header():
    import lagomorph_amd as lm
    from lagomorph_amd import distance, lagomorph_ext as ext

    assert distance.__all__ == ["distance_transform", "signed_distance", "surface_mask", "surface_distance"]
    for name in distance.__all__:
        assert callable(getattr(lm, name)) and getattr(lm, name) is getattr(distance, name)
        assert getattr(lm, name).__doc__
    assert callable(ext.distance_transform)
    assert ext.EDT_WHERE == {"nonzero": 0, "equal": 1, "not_equal": 2, "surface": 3} and ext.EDT_MAX_EXTENT == 1024
    lib = ctypes.CDLL(ext.LIB_PATH)
    assert hasattr(lib, "lago_distance_transform")
    assert lib.lago_abi_version() == ext.ABI_VERSION == 5
    header = open(os.path.join(os.path.dirname(HERE), "include", "lagomorph_hip.h")).read()
    for text in ("#define LAGO_EDT_NONZERO 0", "#define LAGO_EDT_EQUAL 1", "#define LAGO_EDT_NOT_EQUAL 2",
                 "#define LAGO_EDT_SURFACE 3", "#define LAGO_EDT_MAX_EXTENT 1024", "int lago_distance_transform("):
        assert text in header, text
    assert "differentiable" in distance.distance_transform.__doc__
    assert "synchronises" in distance.surface_distance.__doc__
    assert "inf" in distance.signed_distance.__doc__


def test_argument_errors_are_raised_on_cpu_tensors():
    import lagomorph_amd as lm

    L = torch.zeros((2, 1, 4, 5, 6), dtype=torch.int32)
    for where in ("inside", "", None, 3, "Surface"):
        with pytest.raises(ValueError, match="where"):
            lm.distance_transform(L, where)
    for s in (0.0, -1.0, float("nan"), float("inf"), (1.0, 2.0), (1.0, 0.0, 1.0), (1.0, 1.0, 1.0, 1.0), "x", None):
        with pytest.raises(ValueError, match="spacing"):
            lm.distance_transform(L, spacing=s)
        with pytest.raises(ValueError, match="spacing"):
            lm.signed_distance(L, 1, spacing=s)
        with pytest.raises(ValueError, match="spacing"):
            lm.surface_distance(L, L, [1], spacing=s)
    for lab in (2 ** 31, 1.5, "1", None, True):
        with pytest.raises(ValueError, match="label"):
            lm.distance_transform(L, "equal", lab)
    for bad in (L.float(), L.double(), L.half()):
        with pytest.raises(RuntimeError, match="integer labels"):
            lm.distance_transform(bad)
    for bad in (torch.zeros((2, 2, 4, 5, 6), dtype=torch.int32), torch.zeros((2, 1, 4), dtype=torch.int32),
                torch.zeros((2, 1, 4, 5, 6, 7), dtype=torch.int32), torch.zeros((2, 2, 5, 6), dtype=torch.bool)):
        with pytest.raises(RuntimeError, match="label map of shape"):
            lm.distance_transform(bad)
    for sp in ((1025, 2, 2), (2, 1025, 2), (2, 2, 1025), (1025, 2), (2, 1025)):
        with pytest.raises(RuntimeError, match="extents up to 1024"):
            lm.distance_transform(torch.zeros((1, 1) + sp, dtype=torch.uint8))
    with pytest.raises(TypeError):
        lm.distance_transform(L.numpy())
    with pytest.raises(TypeError):
        lm.signed_distance(L.numpy())
    with pytest.raises(RuntimeError, match="same shape"):
        lm.surface_distance(L, L[..., :5], [1])
    for dt in (torch.uint8, torch.int16, torch.int32, torch.int64, torch.bool):   # all fine but for the device
        for where in ("nonzero", "equal", "not_equal", "surface"):
            with pytest.raises(RuntimeError, match="CUDA tensor"):
                lm.distance_transform(L.to(dt), where, 1, (1.5, 0.7, 2.0), squared=True)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            lm.signed_distance(L.to(dt))
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            lm.surface_distance(L.to(dt), L.to(dt), [1, 2])
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            lm.surface_mask(L.to(dt)[:, :, 0], 1)


def test_c_entry_point_validates_before_any_device_call():
    from lagomorph_amd import lagomorph_ext as ext

    OK, INVALID = 0, -1
    f = ext._lib.lago_distance_transform
    p, q = 0x10000, 0x80000000   # never dereferenced: every call below returns before a launch
    one = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    assert f(p, q, 0, 0, one, 0, 5, 1, 4, 4, 4, None) == INVALID and b"dimensional" in ext._lib.lago_last_error()
    for where in (4, -1):
        assert f(p, q, where, 0, one, 0, 3, 1, 4, 4, 4, None) == INVALID and b"where" in ext._lib.lago_last_error()
    for bad in ((0.0, 1.0, 1.0), (1.0, -2.0, 1.0), (1.0, 1.0, float("nan")), (1e-60, 1.0, 1.0), (1.0, 1e60, 1.0)):
        assert f(p, q, 0, 0, (ctypes.c_double * 3)(*bad), 0, 3, 1, 4, 4, 4, None) == INVALID and b"spacing" in ext._lib.lago_last_error()
    assert f(p, q, 0, 0, None, 0, 3, 1, 4, 4, 4, None) == INVALID
    for sp in ((1025, 4, 4), (4, 1025, 4), (4, 4, 1025)):
        assert f(p, q, 0, 0, one, 0, 3, 1, *sp, None) == INVALID and b"extent" in ext._lib.lago_last_error()
    assert f(p, q, 0, 0, one, 0, 2, 1, 4, 1025, 0, None) == INVALID
    assert f(p, q, 0, 0, one, 0, 3, 1, 4, -1, 4, None) == INVALID
    assert f(p, q, 0, 0, one, 0, 3, 3, 1024, 1024, 1024, None) == INVALID and b"2^31" in ext._lib.lago_last_error()
    assert f(p, p + 16, 3, 0, one, 0, 3, 1, 4, 4, 4, None) == INVALID and b"overlap" in ext._lib.lago_last_error()
    assert f(None, q, 0, 0, one, 0, 3, 1, 4, 4, 4, None) == INVALID
    for ext_ in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0)):   # empty: nothing to do
        assert f(None, None, 0, 0, one, 0, 3, *ext_, None) == OK
