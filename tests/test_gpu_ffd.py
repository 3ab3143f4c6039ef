"""GPU: ffd_expand and ffd_restrict (csrc/ffd.hip) against the numpy reference tests/ffd_ref.py (which
tests/test_ffd_host.py ties to scipy's B-spline basis and to known answers): voxel by voxel and control point by
control point against bounds counted from the kernels' own roundings, bit for bit from call to call, through
torch.autograd.gradcheck / gradgradcheck, and composed with `interp`.

Shapes (ffd_ref.CASES) are the smallest that reach every path: general 3D and 2D (one axis at s = 1), s > n (one
cell), an extent of 1, (n - 1) % s == 0 (the last control plane unused), a wave's edge on the contiguous axis (63, 64,
65), s = 1 on every axis of a 3D field (the largest LDS box, above 64 KB in float64), and two tile-boundary shapes.
The kernels' tiles are 8 x 8 x 64 voxels (2D: 64 x 64), larger than the issue's (70, 37, 41) and (33, 70) on one axis
each: that axis is enlarged, to (70, 37, 75) and (97, 70), so that every axis has at least two tiles and a partial one.
N in {1, 2}, C in {1, d, 4}.

Forward: |got - ref| <= ffd_ref.voxel_bound = K u sum_taps w |ctrl| per voxel, K = 12 d + 2 (38 / 26, under the caps 96
and 40), against a reference with exact sums from the same t (float64 sums for float32 results, long double for
float64), and the project's parity criterion 1e-5 max|ref| (float32), 1e-12 max|ref| (float64).
Adjoint: float64 1e-12 max|ref|; float32 per control point ffd_ref.entry_bound = (T_j + 32) u sum_x W[x, j] |g[x]|.
The worst observed ratios are printed."""
import functools

import numpy as np
import pytest
import torch

import ffd_ref as ref
from gpu_util import dev, host
from parity_rule import rtol, units

pytestmark = pytest.mark.gpu

both_dtypes = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
cases = pytest.mark.parametrize("shape,spacing", ref.CASES, ids=str)


def _batches(d):
    """(N, C): N in {1, 2}, C in {1, d, 4}."""
    return [(1 if C == 1 else 2, C) for C in sorted({1, d, 4})]


@functools.lru_cache(maxsize=None)
def _forward_case(shape, spacing, dtype, N, C):
    """(ctrl, reference in float64, voxel bound); the reference's sums in long double for float64 results."""
    dtype = np.dtype(dtype)
    c = ref.field(N, C, ref.grid_shape(shape, spacing), dtype)
    work = np.longdouble if dtype == np.float64 else np.float64
    want = ref.expand(c, shape, spacing, work=work)
    out = (c, want, ref.voxel_bound(c, shape, spacing, dtype))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _adjoint_case(shape, spacing, dtype, N, C):
    dtype = np.dtype(dtype)
    g = ref.field(N, C, shape, dtype, seed=7)
    out = (g, ref.adjoint(g, spacing), ref.entry_bound(g, spacing, dtype))
    for a in out:
        a.setflags(write=False)
    return out


@both_dtypes
@cases
def test_forward(shape, spacing, dtype):
    import lagomorph_amd as lm

    worst = 0.0
    for N, C in _batches(len(shape)):
        c, want, bound = _forward_case(shape, spacing, np.dtype(dtype).name, N, C)
        cd = dev(c)
        got = lm.ffd_expand(cd, shape, spacing)
        assert got.shape == (N, C) + tuple(shape) and got.dtype == cd.dtype and got.is_contiguous()
        h = host(got)
        err = np.abs(h.astype(want.dtype) - want).astype(np.float64)
        ratio = ref.worst_ratio(err, bound)
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{shape} / {spacing} N {N} C {C}: {ratio:.3f} of the voxel bound"
        assert err.max() <= rtol(dtype) * float(np.abs(want).max())
        assert torch.equal(got, lm.ffd_expand(cd, shape, spacing))   # no atomics: the same bits
        assert torch.equal(cd, dev(c))                              # the input is left alone
    print(f"ffd_expand {shape} / {spacing} {np.dtype(dtype).name}: at most {worst:.3f} of the voxel bound")


@both_dtypes
@cases
def test_adjoint(shape, spacing, dtype):
    import lagomorph_amd as lm

    worst = 0.0
    sp = ref.spacing_tuple(spacing, len(shape))
    m = ref.grid_shape(shape, sp)
    for N, C in _batches(len(shape)):
        g, want, bound = _adjoint_case(shape, spacing, np.dtype(dtype).name, N, C)
        gd = dev(g)
        got = lm.ffd_restrict(gd, spacing)
        assert got.shape == (N, C) + m and got.dtype == gd.dtype and got.is_contiguous()
        h = host(got).astype(np.float64)
        err = np.abs(h - want)
        if dtype == np.float64:
            assert units(h, want, dtype, floor=0) <= 1.0
        else:
            ratio = ref.worst_ratio(err, bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{shape} / {spacing} N {N} C {C}: {ratio:.3f} of the entry bound"
        assert torch.equal(got, lm.ffd_restrict(gd, spacing))   # no atomic on memory: the same bits
        assert torch.equal(gd, dev(g))
        unused = 0
        for a, (n, s) in enumerate(zip(shape, sp)):   # entries that no voxel reaches with a weight: exactly 0
            if (n - 1) % s == 0:
                assert (np.take(h, m[a] - 1, axis=2 + a) == 0).all()
                unused += 1
        assert unused == sum((n - 1) % s == 0 for n, s in zip(shape, sp))
    if dtype == np.float32:
        print(f"ffd_restrict {shape} / {spacing}: at most {worst:.3f} of the entry bound")


@cases
def test_adjoint_identity_float64(shape, spacing):
    import lagomorph_amd as lm

    c = dev(ref.field(2, 2, ref.grid_shape(shape, spacing), np.float64, seed=3))
    g = dev(ref.field(2, 2, shape, np.float64, seed=4))
    lhs = float((lm.ffd_expand(c, shape, spacing) * g).sum())
    rhs = float((c * lm.ffd_restrict(g, spacing)).sum())
    scale = float((lm.ffd_expand(c.abs(), shape, spacing) * g.abs()).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs, scale)


def test_unused_control_plane_is_exactly_zero_and_linear_lattices_expand_to_lines():
    import lagomorph_amd as lm

    shape, s = (9, 9, 9), 4
    g = torch.ones((1, 1) + shape, device="cuda")
    d = lm.ffd_restrict(g, s)
    assert (d[:, :, -1] == 0).all() and (d[:, :, :, -1] == 0).all() and (d[..., -1] == 0).all()
    assert (d[:, :, :-1, :-1, :-1] > 0).all()
    assert abs(float(d.sum()) - 9 ** 3) <= 1e-3   # the weights of a voxel sum to 1
    j = torch.arange(6, dtype=torch.float64, device="cuda")
    lattice = (0.5 * (j - 1) * s - 2.0)[None, None, :, None, None].expand(1, 1, 6, 6, 6).contiguous()
    want = (0.5 * torch.arange(9, dtype=torch.float64, device="cuda") - 2.0)[None, None, :, None, None].expand(1, 1, 9, 9, 9)
    assert (lm.ffd_expand(lattice, shape, s) - want).abs().max() <= 1e-13


@pytest.mark.parametrize("shape,spacing", [((5, 6, 7), (2, 3, 4)), ((9, 11), (4, 1))], ids=str)
def test_gradcheck_and_gradgradcheck(shape, spacing):
    import lagomorph_amd as lm

    c = dev(ref.field(1, 2, ref.grid_shape(shape, spacing), np.float64, seed=5)).requires_grad_(True)
    f = lambda x: lm.ffd_expand(x, shape, spacing)   # noqa: E731
    assert torch.autograd.gradcheck(f, (c,), eps=1e-6, atol=1e-8, rtol=1e-8, nondet_tol=0.0)
    assert torch.autograd.gradgradcheck(f, (c,), eps=1e-6, atol=1e-8, rtol=1e-8, nondet_tol=0.0)
    g = dev(ref.field(1, 2, shape, np.float64, seed=6)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: lm.ffd_restrict(x, spacing), (g,), eps=1e-6, atol=1e-8, rtol=1e-8, nondet_tol=0.0)


def test_a_gradient_nobody_needs_runs_no_kernel(monkeypatch):
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    calls = []
    real = ext.ffd_expand_adjoint
    monkeypatch.setattr(ext, "ffd_expand_adjoint", lambda *a: (calls.append(1), real(*a))[1])
    shape, spacing = (5, 6, 7), (2, 3, 4)
    c = dev(ref.field(1, 3, ref.grid_shape(shape, spacing), np.float32))
    w = torch.ones((), device="cuda", requires_grad=True)
    out = lm.ffd_expand(c, shape, spacing)
    assert not out.requires_grad
    (out * w).sum().backward()
    assert c.grad is None and w.grad is not None and not calls

    class Ctx:
        needs_input_grad = (False, False, False, False)
        adjoint = False
    Ctx.shape, Ctx.spacing = shape, spacing
    assert lm.FFDFunction.backward(Ctx, torch.ones_like(out)) == (None, None, None, None) and not calls
    c.requires_grad_(True)
    lm.ffd_expand(c, shape, spacing).sum().backward()
    assert len(calls) == 1 and c.grad.shape == c.shape


def test_gradient_through_interp_is_the_restriction_of_d_u():
    import lagomorph_amd as lm

    shape, spacing = (12, 10, 14), (4, 3, 5)
    I = dev(ref.field(2, 1, shape, np.float32, seed=8))
    go = dev(ref.field(2, 1, shape, np.float32, seed=9))
    c = (0.7 * dev(ref.field(2, 3, ref.grid_shape(shape, spacing), np.float32, seed=10))).requires_grad_(True)
    (lm.interp(I, lm.ffd_expand(c, shape, spacing)) * go).sum().backward()
    u = lm.ffd_expand(c.detach(), shape, spacing).requires_grad_(True)
    (lm.interp(I, u) * go).sum().backward()
    assert torch.equal(c.grad, lm.ffd_restrict(u.grad, spacing))
    assert float(c.grad.abs().max()) > 0


def test_adam_on_the_lattice_reduces_the_squared_difference():
    import lagomorph_amd as lm

    shape, s = (24, 20, 22), 4
    ax = [torch.arange(n, dtype=torch.float32, device="cuda") for n in shape]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")

    def blob(cx):
        return torch.exp(-((X - cx) ** 2 + (Y - 9.5) ** 2 + (Z - 10.5) ** 2) / (2 * 3.0 ** 2))[None, None].contiguous()

    I, J = blob(11.5), blob(12.5)   # the same blob one voxel further along x
    c = torch.zeros((1, 3) + lm.ffd_grid_shape(shape, s), device="cuda", requires_grad=True)
    opt = torch.optim.Adam([c], lr=0.05)   # at most one voxel of motion in 20 steps: no overshoot past the target
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = ((lm.interp(I, lm.ffd_expand(c, shape, s)) - J) ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    final = float(((lm.interp(I, lm.ffd_expand(c.detach(), shape, s)) - J) ** 2).sum())
    print(f"squared difference {losses[0]:.4f} -> {final:.4f} in 20 Adam steps")
    assert final < losses[0]


@both_dtypes
def test_non_default_stream_gives_the_same_bits(dtype):
    import lagomorph_amd as lm

    for shape, spacing in (((70, 37, 75), (5, 3, 7)), ((97, 70), (32, 7))):
        c = dev(ref.field(2, 2, ref.grid_shape(shape, spacing), dtype))
        g = dev(ref.field(2, 2, shape, dtype, seed=7))
        want_f, want_a = lm.ffd_expand(c, shape, spacing), lm.ffd_restrict(g, spacing)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            got_f, got_a = lm.ffd_expand(c, shape, spacing), lm.ffd_restrict(g, spacing)
        stream.synchronize()
        assert torch.equal(got_f, want_f) and torch.equal(got_a, want_a)


@both_dtypes
def test_empty_problems(dtype):
    import lagomorph_amd as lm

    tdt = torch.float32 if dtype == np.float32 else torch.float64
    for shape, spacing in (((5, 6, 7), (2, 3, 4)), ((9, 11), (4, 1))):
        m = lm.ffd_grid_shape(shape, spacing)
        for N, C in ((0, 3), (2, 0), (0, 0)):
            out = lm.ffd_expand(torch.zeros((N, C) + m, dtype=tdt, device="cuda"), shape, spacing)
            assert out.shape == (N, C) + tuple(shape) and out.dtype == tdt and out.numel() == 0
            d = lm.ffd_restrict(torch.zeros((N, C) + tuple(shape), dtype=tdt, device="cuda"), spacing)
            assert d.shape == (N, C) + m and d.dtype == tdt and d.numel() == 0
    torch.cuda.synchronize()
