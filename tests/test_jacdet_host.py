"""CPU: the test-side reference of jacobian_determinant (tests/jacdet_ref.py) against an independent pure-torch
restatement and against known answers; the operator's public surface, C symbols and CPU-tensor behaviour."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import jacdet_ref
from oracle import lago_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(5, 6, 7), (2, 2, 2), (3, 4, 1), (9, 5, 70), (7, 9), (2, 2), (5, 1), (24, 20, 36)]


@pytest.mark.parametrize("displacement", [True, False])
@pytest.mark.parametrize("scale", [0.3, 3.0])
@pytest.mark.parametrize("sp", SHAPES)
def test_reference_agrees_with_torch_restatement(sp, scale, displacement):
    """float64: forward equal bit for bit, backward within 1e-12 x max|ref| (fold-free fields at scale 0.3, about
    half of the voxels folded at scale 3)."""
    rng = np.random.default_rng(abs(hash((sp, scale))) % 2**31)
    u = scale * rng.standard_normal((2, len(sp)) + sp)
    go = rng.standard_normal((2, 1) + sp)
    fwd = jacdet_ref.forward(u, displacement)
    assert fwd.shape == (2, 1) + sp and fwd.dtype == np.float64
    assert np.array_equal(fwd, jacdet_ref.torch_forward(u, displacement))
    bwd, want = jacdet_ref.backward(go, u, displacement), jacdet_ref.torch_backward(go, u, displacement)
    err = np.abs(bwd - want).max()
    print(f"backward {sp} scale {scale}: {err / max(np.abs(want).max(), 1e-300):.3e} of max|ref|")
    assert err <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9), (3, 4, 1)])
def test_zero_field(sp, dtype):
    u = np.zeros((2, len(sp)) + sp, dtype=dtype)
    one = jacdet_ref.forward(u, True)
    assert one.dtype == dtype and np.array_equal(one, np.ones_like(one))
    assert np.array_equal(jacdet_ref.forward(u, False), np.zeros_like(one))


@pytest.mark.parametrize("sp", [(6, 7, 8), (7, 8)])
def test_linear_map_has_constant_determinant(sp):
    """u(x) = (A - I) x: central differences are exact on a linear field, so det(I + Du) = det A at every interior
    voxel (the one-sided half difference of the border voxels takes half the slope)."""
    d = len(sp)
    rng = np.random.default_rng(d)
    A = np.eye(d) + rng.uniform(-0.5, 0.5, (d, d))
    x = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sp], indexing="ij"))
    u = np.tensordot(A - np.eye(d), x, axes=1)[None]
    got = jacdet_ref.forward(u, True)[0, 0][(slice(1, -1),) * d]
    want = np.linalg.det(A)
    err = np.abs(got - want).max() / abs(want)
    print(f"linear map {sp}: {err:.3e} |det A|")
    assert err <= 1e-12
    # displacement=False on the map itself: det of D(Ax) = det A
    got = jacdet_ref.forward(np.tensordot(A, x, axes=1)[None], False)[0, 0][(slice(1, -1),) * d]
    assert np.abs(got - want).max() <= 1e-12 * abs(want)


def test_float32_reference_error_is_far_inside_the_tolerance():
    """The float32 reference against the float64 one on the same float32 inputs, in units of the project's float32
    tolerance 1e-5 x max|ref|: what the GPU comparison's bound has to spare.  Bound 0.1: a determinant (a d_u element)
    is about 15 roundings of terms no larger than the maximum, each at most 2^-24 = 6e-8 relative: 1e-6 = 0.1 units."""
    rng = np.random.default_rng(5)
    for sp in [(9, 5, 70), (24, 20, 36), (7, 9)]:
        for scale in (0.3, 3.0):
            u = (scale * rng.standard_normal((2, len(sp)) + sp)).astype(np.float32)
            go = rng.standard_normal((2, 1) + sp).astype(np.float32)
            f64, b64 = jacdet_ref.forward(u.astype(np.float64)), jacdet_ref.backward(go.astype(np.float64), u.astype(np.float64))
            ef = np.abs(jacdet_ref.forward(u) - f64).max() / (1e-5 * np.abs(f64).max())
            eb = np.abs(jacdet_ref.backward(go, u) - b64).max() / (1e-5 * np.abs(b64).max())
            print(f"{sp} scale {scale}: forward {ef:.4f}, backward {eb:.4f} of 1e-5 x max|ref|")
            assert ef <= 0.1 and eb <= 0.1


def test_public_surface():
    import lagomorph_amd as lm

    assert callable(lm.jacobian_determinant)
    assert issubclass(lm.JacobianDeterminantFunction, torch.autograd.Function)
    assert callable(lm.lagomorph_ext.jacobian_determinant_forward)
    assert callable(lm.lagomorph_ext.jacobian_determinant_backward)


def test_header_declares_and_library_exports_the_entry_points():
    import lagomorph_amd

    text = open(os.path.join(ROOT, "include", "lagomorph_hip.h")).read()
    block = text[text.index("#define LAGO_DECLARE(REAL, SUF)"):text.index("LAGO_DECLARE(float, _f32)")]
    for name in ("lago_jacdet_forward", "lago_jacdet_backward"):
        assert re.search(rf"\bint {name}##SUF\s*\(", block), f"{name} is not declared inside the ##SUF block"
    lib = ctypes.CDLL(lagomorph_amd.lagomorph_ext.LIB_PATH)
    for name in ("lago_jacdet_forward_f32", "lago_jacdet_forward_f64", "lago_jacdet_backward_f32",
                 "lago_jacdet_backward_f64"):
        assert hasattr(lib, name), name
    assert lib.lago_abi_version() == 5


def test_no_cpu_fallback():
    import lagomorph_amd as lm

    u = torch.zeros((1, 3, 4, 4, 4))
    go = torch.zeros((1, 1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        lm.jacobian_determinant(u)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        lm.lagomorph_ext.jacobian_determinant_forward(u, True)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        lm.lagomorph_ext.jacobian_determinant_backward(go, u, True)


def test_oracle_is_what_the_reference_module_uses():
    """J built through the oracle is the rounded clamped difference itself: 0.5 * (u[+1] - u[-1]) with index clamp."""
    rng = np.random.default_rng(1)
    u = rng.standard_normal((1, 2, 5, 6)).astype(np.float32)
    J = jacdet_ref.jacobian(u, False)
    up = np.concatenate([u[:, :, 1:], u[:, :, -1:]], axis=2)
    um = np.concatenate([u[:, :, :1], u[:, :, :-1]], axis=2)
    assert np.array_equal(J[1][0], (np.float32(0.5) * (up - um))[:, 1])
    assert orc.jacobian_times_vectorfield_forward(u, u, True, False).dtype == np.float32
