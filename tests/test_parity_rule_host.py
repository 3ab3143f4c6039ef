"""CPU: tests/parity_rule.py, the one statement of the project's acceptance rule, at its edges; and the wrappers of
tests/gpu_util.py on CPU tensors.

The bound is RTOL * max(scale, floor) with scale = max|want| unless given.  An error of exactly the bound passes, the
next float64 above it does not; anything that is not a number fails; floor=0 is "RTOL * max|want| exactly"."""
import sys

import numpy as np
import pytest

import parity_rule as pr

F32, F64 = np.float32, np.float64
BOTH = pytest.mark.parametrize("dtype,rtol", [(F32, 1e-5), (F64, 1e-12)])


def _fails(got, want, dtype, **kw):
    """True when the rule rejects; the raising and the fail-list forms of `close` must agree."""
    fails = []
    pr.close(got, want, dtype, "x", fails=fails, **kw)
    if fails:
        with pytest.raises(AssertionError):
            pr.close(got, want, dtype, "x", **kw)
    else:
        pr.close(got, want, dtype, "x", **kw)
    return bool(fails)


@BOTH
@pytest.mark.parametrize("scale", [1.0, 3.7, 1e-3, 123456.789])
def test_exactly_the_bound_passes_and_the_next_float_fails(dtype, rtol, scale):
    want = np.array([scale, -0.25 * scale, 0.0])
    tol = rtol * scale
    up = np.nextafter(tol, np.inf)
    assert pr.units(want + [0, 0, tol], want, dtype) == 1.0
    assert not _fails(want + [0, 0, tol], want, dtype) and not _fails(want - [0, 0, tol], want, dtype)
    assert pr.units(want + [0, 0, up], want, dtype) > 1.0
    assert _fails(want + [0, 0, up], want, dtype) and _fails(want - [0, 0, up], want, dtype)


@BOTH
def test_not_a_number_fails(dtype, rtol):
    want = np.array([1.0, 2.0, 3.0])
    for bad in (np.nan, np.inf, -np.inf):
        got = want.copy()
        got[1] = bad
        assert not pr.units(got, want, dtype) <= 1.0
        assert _fails(got, want, dtype) and _fails(got, want, dtype, floor=0) and _fails(got, want, dtype, scale=1e300)
    assert _fails(np.array([1.0, np.nan]), np.array([1.0, np.nan]), dtype)   # NaN in both arrays at the same place
    assert _fails(np.array([np.inf]), np.array([np.inf]), dtype)
    assert _fails(np.array([np.nan]), np.zeros(1), dtype, floor=0)


@BOTH
def test_empty_arrays_and_shapes(dtype, rtol):
    assert pr.units(np.zeros((0, 3)), np.zeros((0, 3)), dtype) == 0.0
    assert pr.units(np.zeros(0), np.zeros(0), dtype, floor=0) == 0.0
    assert not _fails(np.zeros((2, 0)), np.zeros((2, 0)), dtype)
    for other in ((3, 2), (3,), (6,)):                      # (no broadcasting)
        with pytest.raises(AssertionError, match="shape"):
            pr.units(np.zeros((2, 3)), np.zeros(other), dtype)
        assert _fails(np.zeros((2, 3)), np.zeros(other), dtype)


@BOTH
def test_scale_overrides_the_reference_maximum(dtype, rtol):
    want = np.array([1.0, -2.0])
    got = want + [0.0, 10 * rtol]                           # 5 units of max|want| = 2
    assert _fails(got, want, dtype) and not _fails(got, want, dtype, scale=20.0) and _fails(got, want, dtype, scale=9.0)
    assert pr.units(got, want, dtype) == pytest.approx(5.0) and pr.units(got, want, dtype, scale=20.0) == pytest.approx(1.0 / 2)
    assert type(pr.units(got, want, dtype, scale=np.float32(20.0))) is float      # (LAGO_TOL_REPORT is written as JSON)


@BOTH
def test_floor_zero_is_the_bound_exactly(dtype, rtol):
    zero, tiny = np.zeros(4), np.array([0, 0, 5e-324, 0])
    assert pr.units(zero, zero, dtype, floor=0) == 0.0 and not _fails(zero, zero, dtype, floor=0)
    assert pr.units(tiny, zero, dtype, floor=0) == np.inf and _fails(tiny, zero, dtype, floor=0)
    want = np.array([0.0, 8.0])
    tol = rtol * 8.0
    assert not _fails(want + [tol, 0], want, dtype, floor=0) and _fails(want + [np.nextafter(tol, 1), 0], want, dtype, floor=0)


def test_default_floor_under_a_zero_reference():
    zero = np.zeros(3)                # float32: the bound is 1e-5 * 1e-300 = 1e-305;  float64: 1e-12 * 1e-300 = 1e-312
    assert not _fails(zero + 1e-310, zero, F32) and _fails(zero + 1e-304, zero, F32)
    assert not _fails(zero + 1e-313, zero, F64) and _fails(zero + 1e-311, zero, F64)
    assert not _fails(zero, zero, F32) and not _fails(zero, zero, F64)
    assert not _fails(zero + 1e-36, zero, F32, floor=1e-30) and _fails(zero + 1e-36, zero, F32)   # an explicit floor


def test_every_spelling_of_a_dtype():
    import torch

    for name, want in (("float32", 1e-5), ("float64", 1e-12)):
        npt = getattr(np, name)
        for spelling in (getattr(torch, name), npt, np.dtype(npt), name, np.dtype(name).str, npt(0).dtype):
            assert pr.rtol(spelling) == want == pr.RTOL[np.dtype(name)], spelling
    for other in (torch.float16, np.int32, "complex64"):
        with pytest.raises(KeyError):
            pr.rtol(other)


def test_bits_tells_dtype_shape_and_the_first_differing_index():
    a = np.arange(24, dtype=F32).reshape(2, 3, 4)
    pr.bits(a, a.copy(), "same")
    with pytest.raises(AssertionError, match="float32 vs .*float64"):
        pr.bits(a, a.astype(F64), "dtype")
    pr.bits(a, a.astype(F64), "dtype", check_dtype=False)
    with pytest.raises(AssertionError, match=r"\(2, 3, 4\) .* vs \(6, 4\)"):
        pr.bits(a, a.reshape(6, 4), "shape", check_dtype=False)
    b = a.copy()
    b[1, 0, 2] += 1
    b[1, 2, 3] = np.nan
    with pytest.raises(AssertionError, match=r"2 of 24 entries, first at \(1, 0, 2\)"):
        pr.bits(b, a, "values")
    fails = []
    pr.bits(b, a, "values", fails=fails), pr.bits(a, a.copy(), "same", fails=fails)
    assert len(fails) == 1 and "first at (1, 0, 2)" in fails[0]
    n = np.array([np.nan, 1.0])
    with pytest.raises(AssertionError):         # NaN is not bit-identical to NaN here, as in every copy this replaced
        pr.bits(n, n.copy(), "nan")


def test_close_keeps_the_worst_and_names_the_place():
    (worst, fails), want = ({}, []), np.array([[1.0, 2.0], [3.0, 4.0]])
    pr.close(want + [[0, 0], [2e-5, 0]], want, F32, "a", fails=fails, worst=worst)
    pr.close(want + [[0, 8e-5], [0, 0]], want, F32, "a", fails=fails, worst=worst)
    pr.close(want, want, F32, "a", fails=fails, worst=worst)
    assert worst["a"] == pytest.approx(2.0) and len(fails) == 1 and "at (0, 1)" in fails[0]


def test_imports_without_torch(monkeypatch):
    """A fresh copy of the module, loaded while `import torch` fails."""
    import importlib.util

    monkeypatch.setitem(sys.modules, "torch", None)
    with pytest.raises(ImportError):
        import torch  # noqa: F401
    spec = importlib.util.spec_from_file_location("parity_rule_without_torch", pr.__file__)
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert fresh.rtol("float32") == 1e-5 and fresh.units(np.ones(2), np.ones(2), "float64") == 0.0
    assert {k for k, v in vars(fresh).items() if isinstance(v, type(sys))} == {"np"}


def test_gpu_util_wrappers_on_cpu_tensors():
    import torch

    import gpu_util

    want = np.array([1.0, -4.0], dtype=F32)
    got = torch.tensor([1.0, -4.0 + 2e-5], dtype=torch.float32)
    before = dict(gpu_util.OBSERVED)
    try:
        u = gpu_util.assert_close(got, want, torch.float32, "helper check (case 1) [x]")
        assert 0.4 < u < 0.6 and gpu_util.OBSERVED["helper check f32"] == u
        assert gpu_util.units_of(got, want, torch.float32) == u
        with pytest.raises(AssertionError, match="helper check"):
            gpu_util.assert_close(got + 1e-3, want, torch.float32, "helper check (case 2)")
        assert gpu_util.OBSERVED["helper check f32"] > 1.0          # recorded before the assertion, as it always was
        gpu_util.assert_close(got.double(), want, torch.float64, "unrecorded", scale=1e8, record=False)
        assert "unrecorded f64" not in gpu_util.OBSERVED
    finally:
        gpu_util.OBSERVED.clear()
        gpu_util.OBSERVED.update(before)
    gpu_util.assert_bits(got, got.clone(), "tensor against tensor")
    gpu_util.assert_bits(got, gpu_util.host(got).astype(F64), "dtype", check_dtype=False)
    with pytest.raises(AssertionError):
        gpu_util.assert_bits(got, gpu_util.host(got).astype(F64), "dtype")
