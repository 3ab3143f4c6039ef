"""CPU: the test-side reference of invert_displacement (tests/invert_ref.py) against an independent pure-numpy
restatement and against known answers; the test fields' contraction bound; the operator's public surface, C symbols
and argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import invert_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(5, 6, 7), (8, 8, 8), (3, 4, 1), (2, 2, 2), (9, 5, 70), (6, 5, 16), (3, 4, 128), (7, 9), (16, 16), (2, 2), (5, 1),
          (3, 130)]


@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9)])
def test_reference_agrees_with_numpy_restatement(sp):
    """float64, within 1e-12 x max|ref| (the restatement sums the corner products in another order): a contraction
    field at 1, 5 and 60 steps, and a random field of 3 voxels amplitude whose samples leave the grid."""
    rng = np.random.default_rng(len(sp))
    for u, what in ((invert_ref.field(sp, 2, np.float64), "L = 0.5"), (3.0 * rng.standard_normal((2, len(sp)) + sp), "random 3.0")):
        for iters in (0, 1, 5, 60):
            got, want = invert_ref.forward(u, iters), invert_ref.np_forward(u, iters)
            assert got.dtype == np.float64 and got.shape == u.shape
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"{sp} {what} iters {iters}: {err:.3e} of max|ref|")
            if what == "L = 0.5" or iters <= 1:
                assert err <= 1e-12
            # (outside the contraction regime the iteration amplifies rounding differences: no bound is claimed there)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sp", SHAPES)
def test_fields_are_contractions_and_the_reference_converges(sp, dtype):
    """The bound is 0.5 on the array the tests use, and the step v_k - v_{k+1} then shrinks to the rounding level: one
    step's rounding is about 10 roundings of the lerp plus the rounding of the sample position (half an ulp of an
    index below 2^8, times a slope of at most 2 pi / n x max|u|), under 32 eps x max|u| together, and a contraction at
    0.5 doubles it: 64 eps x max|u|."""
    u = invert_ref.field(sp, 2, dtype)
    assert u.dtype == dtype and u.shape == (2, len(sp)) + sp
    L = invert_ref.lipschitz_bound(u)
    assert 0.49 <= L <= 0.5 + 1e-9, L
    v1, v60 = invert_ref.forward(u, 1), invert_ref.forward(u, 60)
    scale = np.abs(u).max()
    res60 = np.abs(v60 - invert_ref.forward(u, 61)).max()
    res1 = np.abs(v1 - invert_ref.forward(u, 2)).max()
    eps = np.finfo(dtype).eps
    print(f"{sp} {np.dtype(dtype).name}: L {L:.6f}, |v1 - v2| {res1 / scale:.3e}, |v60 - v61| {res60 / scale:.3e} of max|u|")
    assert res60 <= 64 * eps * scale
    assert invert_ref.min_det(u, v60) >= 0.125   # (1 - L)^3: no fold at the fixed point


@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9)])
def test_reference_gradient_is_the_derivative_of_the_converged_inverse(sp):
    """<d_u, delta> against the central difference of <go, v(u + e delta)> in float64 (v by the numpy restatement,
    60 steps): the implicit-function-theorem gradient the kernels are held to is the right one."""
    rng = np.random.default_rng(7)
    u = invert_ref.field(sp, 2, np.float64)
    go = rng.standard_normal(u.shape)
    v = invert_ref.forward(u, 60)
    du = invert_ref.d_u(go, u, v)
    for trial in range(3):
        delta = rng.standard_normal(u.shape)
        e = 1e-6
        fd = (np.sum(go * invert_ref.np_forward(u + e * delta, 60)) - np.sum(go * invert_ref.np_forward(u - e * delta, 60))) / (2 * e)
        an = np.sum(du * delta)
        print(f"{sp} trial {trial}: analytic {an:.9e}, central difference {fd:.9e}")
        assert abs(an - fd) <= 1e-6 * max(abs(an), np.abs(du).max())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9), (3, 4, 1)])
def test_known_answers(sp, dtype):
    d = len(sp)
    zero = np.zeros((2, d) + sp, dtype=dtype)
    for iters in (0, 1, 7):
        v = invert_ref.forward(zero, iters)
        assert v.dtype == dtype and np.array_equal(v, zero)
    # a field constant in space: v = -c after one step.  Dyadic components, so that every weight (1 - t, t) and every
    # product of the interpolation is exact and the answer holds bit for bit.
    c = np.array([0.25, -0.5, 0.375][:d], dtype=dtype)
    u = np.broadcast_to(c.reshape((1, d) + (1,) * d), (2, d) + sp).copy()
    inner = (slice(None), slice(None)) + tuple(slice(1, -1) if n > 2 else slice(None) for n in sp)
    for iters in (1, 2, 9):
        assert np.array_equal(invert_ref.forward(u, iters)[inner], -u[inner])
    # iters = 0 is -u
    rng = np.random.default_rng(0)
    u = rng.standard_normal((2, d) + sp).astype(dtype)
    assert np.array_equal(invert_ref.forward(u, 0), -u)


def test_public_surface():
    import lagomorph_amd as lm

    assert callable(lm.invert_displacement)
    assert issubclass(lm.InvertDisplacementFunction, torch.autograd.Function)
    assert callable(lm.lagomorph_ext.invert_displacement_forward)
    assert callable(lm.lagomorph_ext.invert_displacement_adjoint)
    doc = lm.invert_displacement.__doc__
    assert "v_{k+1}(x) = -u(x + v_k(x))" in doc and "contraction" in doc and "compose(v, u)" in doc


def test_header_declares_and_library_exports_the_entry_points():
    import lagomorph_amd

    text = open(os.path.join(ROOT, "include", "lagomorph_hip.h")).read()
    block = text[text.index("#define LAGO_DECLARE(REAL, SUF)"):text.index("LAGO_DECLARE(float, _f32)")]
    for name in ("lago_invert_disp_forward", "lago_invert_disp_adjoint"):
        assert re.search(rf"\bint {name}##SUF\s*\(", block), f"{name} is not declared inside the ##SUF block"
    lib = ctypes.CDLL(lagomorph_amd.lagomorph_ext.LIB_PATH)
    for name in ("lago_invert_disp_forward_f32", "lago_invert_disp_forward_f64", "lago_invert_disp_adjoint_f32",
                 "lago_invert_disp_adjoint_f64"):
        assert hasattr(lib, name), name
    assert lib.lago_abi_version() == 5


def test_c_entry_points_reject_bad_arguments_before_touching_the_gpu():
    """iters < 0, a dim outside {2, 3} and out aliasing u are LAGO_ERR_INVALID; nn == 0 is a successful no-op.  None
    of these reaches a launch, so the calls are made here with host addresses that are never dereferenced."""
    import lagomorph_amd

    ext = lagomorph_amd.lagomorph_ext
    lib = ctypes.CDLL(ext.LIB_PATH)
    lib.lago_last_error.restype = ctypes.c_char_p
    a = np.zeros(2 * 3 * 64, dtype=np.float32)
    b = np.zeros_like(a)
    i64 = ctypes.c_int64
    for suf in ("_f32", "_f64"):
        f = getattr(lib, "lago_invert_disp_forward" + suf)
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, i64, i64, i64, i64, ctypes.c_void_p]
        f.restype = ctypes.c_int
        assert f(a.ctypes.data, b.ctypes.data, -1, 3, 2, 4, 4, 4, None) != 0
        assert b"iters" in lib.lago_last_error()
        assert f(a.ctypes.data, b.ctypes.data, 3, 4, 2, 4, 4, 4, None) != 0
        assert f(a.ctypes.data, b.ctypes.data, 3, 1, 2, 4, 4, 4, None) != 0
        assert f(a.ctypes.data, a.ctypes.data, 3, 3, 1, 4, 4, 4, None) != 0
        assert b"alias" in lib.lago_last_error()
        assert f(a.ctypes.data, b.ctypes.data, 3, 3, 0, 4, 4, 4, None) == 0
        assert f(a.ctypes.data, b.ctypes.data, 3, 2, 0, 4, 4, 1, None) == 0
        g = getattr(lib, "lago_invert_disp_adjoint" + suf)
        g.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, i64, i64, i64, i64, ctypes.c_void_p]
        g.restype = ctypes.c_int
        assert g(a.ctypes.data, b.ctypes.data, b.ctypes.data, b.ctypes.data, 5, 1, 4, 4, 4, None) != 0
        assert g(a.ctypes.data, b.ctypes.data, b.ctypes.data, b.ctypes.data, 3, 0, 4, 4, 4, None) == 0


def test_shim_argument_checks():
    import lagomorph_amd as lm

    ext = lm.lagomorph_ext
    u = torch.zeros((1, 3, 4, 4, 4))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        lm.invert_displacement(u)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ext.invert_displacement_forward(u, 3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ext.invert_displacement_adjoint(u, u, u)
    with pytest.raises(RuntimeError, match="vector field"):       # wrong channel count
        ext.invert_displacement_forward(torch.zeros((1, 2, 4, 4, 4)), 3)
    with pytest.raises(RuntimeError, match="vector field"):
        ext.invert_displacement_forward(torch.zeros((1, 3, 4, 4)), 3)
    with pytest.raises(RuntimeError, match="two- and three-dimensional"):
        ext.invert_displacement_forward(torch.zeros((1, 1, 4)), 3)
    with pytest.raises(RuntimeError, match="float32 and float64"):  # integer dtype
        ext.invert_displacement_forward(torch.zeros((1, 3, 4, 4, 4), dtype=torch.int32), 3)
    with pytest.raises(RuntimeError, match="iters must not be negative"):
        ext.invert_displacement_forward(u, -1)
    with pytest.raises(RuntimeError, match="iters must not be negative"):
        lm.invert_displacement(u, iters=-2)
