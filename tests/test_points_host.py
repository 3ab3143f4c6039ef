"""CPU: the specification of interp_points, deform_points and landmark_distance before any GPU run.

- tests/points_ref.py, the numpy reference, against torch.nn.functional.grid_sample on the CPU in float64 (values,
  position gradient, and the wide scatter against the gradient on F), and against known answers;
- landmark_distance against a hand computation;
- the public surface: names, docstrings, C symbols, header text, the argument errors (raised on CPU tensors, before any
  device call) and the C entry points' validation."""
import ctypes
import os

import numpy as np
import pytest
import torch

import points_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the reference against grid_sample

def _grid_sample(F, x):
    """(values (N, C, P), d values . g / d x (N, d, P), d values . g / d F, g) through grid_sample in float64:
    bilinear, border padding, align_corners, the normalised grid g_a = 2 x_a / (n_a - 1) - 1 with the axes reversed."""
    sp, d = F.shape[2:], F.ndim - 2
    N, P = x.shape[0], x.shape[2]
    Ft = torch.from_numpy(F.astype(np.float64)).requires_grad_(True)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    scale = torch.tensor([2.0 / (n - 1) for n in sp], dtype=torch.float64).view(1, d, 1)
    grid = (xt * scale - 1.0).flip(1).permute(0, 2, 1).reshape((N,) + (1,) * (d - 1) + (P, d))
    out = torch.nn.functional.grid_sample(Ft.expand((N,) + F.shape[1:]), grid, mode="bilinear", padding_mode="border",
                                          align_corners=True).reshape(N, F.shape[1], P)
    g = torch.from_numpy(ref.upstream(N, F.shape[1], P, np.float64, seed=7))
    out.backward(g)
    return out.detach().numpy(), xt.grad.numpy(), Ft.grad.numpy(), g.numpy()


@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9), (2, 2, 2)])
@pytest.mark.parametrize("NF", [2, 1])
def test_reference_equals_grid_sample(sp, NF):
    N, C, P = 2, 3, 400
    F = ref.field(NF, C, sp, np.float64)
    x, first = ref.scattered(N, sp, P, np.float64)
    assert ref.outside(x, sp).mean() > 0.3          # a large share of the points leaves the grid
    want, want_dx, want_dF, g = _grid_sample(F, x)
    val, grad = ref.sample(F, x)
    dx = (g[:, :, None, :] * grad).sum(1)
    s, sabs, count = ref.scatter_wide(g, x, sp, NF)
    errs = (np.abs(val - want).max(), np.abs(dx - want_dx).max(), np.abs(s.astype(np.float64) - want_dF).max())
    print(f"{sp} NF {NF}: values {errs[0]:.3e}, d_x {errs[1]:.3e}, d_F {errs[2]:.3e}")
    assert errs[0] <= 1e-12 and errs[1] <= 1e-12 and errs[2] <= 1e-12
    assert count.sum() == N * C * P * 2 ** len(sp) and np.all((count == 0) <= (s == 0))


# ---- known answers

@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9), (1, 5, 4), (1, 9)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_known_answers(sp, dtype):
    N, C, d = 2, 2, len(sp)
    F = ref.field(N, C, sp, dtype)
    # integer positions return the voxel
    x = ref.identity_points(N, sp, dtype)
    val, _ = ref.sample(F, x)
    assert np.array_equal(val, F.reshape(N, C, -1).astype(np.float64))
    # outside the grid: the border value, and a zero gradient on that axis
    for a, n in enumerate(sp):
        for far, edge in ((-1.75, 0), (n + 0.5, n - 1), (-1e6, 0), (1e6, n - 1)):
            xo = x.copy()
            xo[:, a] = far
            xe = x.copy()
            xe[:, a] = edge
            val, grad = ref.sample(F, xo)
            assert np.abs(val - ref.sample(F, xe)[0]).max() <= 1e-13, (a, far)   # ((1 - t) c + t c rounds)
            assert np.all(grad[:, :, a] == 0), (a, far)


@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9)])
def test_reference_reproduces_an_affine_field_and_is_adjoint(sp):
    N, C, d, P = 2, 3, len(sp), 300
    rng = np.random.default_rng(5)
    A, b = rng.standard_normal((C, d)), rng.standard_normal(C)
    idx = np.indices(sp).astype(np.float64)
    F = np.broadcast_to(np.tensordot(A, idx, 1) + b.reshape((C,) + (1,) * d), (N, C) + sp)
    x = ref.interior(N, sp, P, np.float64)
    val, grad = ref.sample(F, x)
    want = np.einsum("ca,nap->ncp", A, x) + b.reshape(1, C, 1)
    assert np.abs(val - want).max() <= 1e-13
    assert np.abs(grad - A.reshape(1, C, d, 1)).max() <= 1e-13
    # <sample(F, x), g> = <F, scatter(g)>, also for points that leave the grid and for a broadcast F
    for NF in (N, 1):
        F = ref.field(NF, C, sp, np.float64)
        x, _ = ref.scattered(N, sp, P, np.float64, seed=1)
        g = ref.upstream(N, C, P, np.float64)
        val, _ = ref.sample(F, x)
        s, _, _ = ref.scatter_wide(g, x, sp, NF)
        lhs, rhs = float((val * g).sum()), float((F * s.astype(np.float64)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (lhs, rhs)


# ---- landmark_distance

def test_landmark_distance_by_hand():
    import lagomorph_amd as lm

    x = torch.tensor([[[0.0, 1.0], [0.0, 2.0], [0.0, 3.0]], [[1.0, 5.0], [1.0, 5.0], [1.0, 5.0]]], dtype=torch.float64)
    y = torch.tensor([[[3.0, 1.0], [4.0, 0.0], [0.0, 3.0]]], dtype=torch.float64)             # (1, 3, 2): broadcast
    # item 0: (-3, -4, 0) and (0, 2, 0); item 1: (-2, -3, 1) and (4, 5, 2)
    assert torch.equal(lm.landmark_distance(x, y), torch.tensor([[5.0, 2.0], [14.0 ** 0.5, 45.0 ** 0.5]], dtype=torch.float64))
    assert torch.equal(lm.landmark_distance(x, y, squared=True), torch.tensor([[25.0, 4.0], [14.0, 45.0]], dtype=torch.float64))
    sp = (2.0, 0.5, 3.0)
    assert torch.equal(lm.landmark_distance(x, y, sp, squared=True),
                       torch.tensor([[36.0 + 4.0, 1.0], [16.0 + 2.25 + 9.0, 64.0 + 6.25 + 36.0]], dtype=torch.float64))
    assert torch.equal(lm.landmark_distance(x, y, sp), lm.landmark_distance(x, y, sp, squared=True).sqrt())
    assert torch.equal(lm.landmark_distance(x, x[:1] + 0.0)[0], torch.zeros(2, dtype=torch.float64))
    # 2D, float32, and the squared form's gradient at zero distance
    a = torch.tensor([[[1.0, 2.0], [3.0, 4.0]]], requires_grad=True)
    lm.landmark_distance(a, a.detach().clone(), squared=True).sum().backward()
    assert torch.equal(a.grad, torch.zeros_like(a))
    assert torch.equal(lm.landmark_distance(a.detach(), a.detach() + torch.tensor([3.0, 4.0]).view(1, 2, 1)), torch.full((1, 2), 5.0))
    with pytest.raises(RuntimeError, match="spacing"):
        lm.landmark_distance(x, y, (1.0, 2.0))
    with pytest.raises(RuntimeError, match="landmark_distance"):
        lm.landmark_distance(x, y[:, :2])
    with pytest.raises(TypeError):
        lm.landmark_distance(x.numpy(), y)


# ---- the public surface

def test_names_symbols_and_abi_version():
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext, points

    for name in ("interp_points", "deform_points", "landmark_distance", "InterpPointsFunction"):
        assert getattr(lm, name) is getattr(points, name) and getattr(lm, name).__doc__
    assert issubclass(lm.InterpPointsFunction, torch.autograd.Function)
    assert callable(ext.interp_points_forward) and callable(ext.interp_points_backward)
    lib = ctypes.CDLL(ext.LIB_PATH)
    for sym in ("lago_interp_points_f32", "lago_interp_points_f64", "lago_interp_points_backward_f32",
                "lago_interp_points_backward_f64"):
        assert hasattr(lib, sym) and sym in ext._fn, sym
    assert lib.lago_abi_version() == ext.ABI_VERSION == 5
    header = open(os.path.join(os.path.dirname(HERE), "include", "lagomorph_hip.h")).read()
    for text in ("#define LAGO_ABI_VERSION 5", "int lago_interp_points##SUF(REAL *out, const REAL *F, const REAL *x, int dim,",
                 "int lago_interp_points_backward##SUF(REAL *d_F, REAL *d_x, const REAL *grad_out, const REAL *F,",
                 "arrival order", "2^30"):
        assert text in header, text
    doc = lm.interp_points.__doc__
    for text in ("clamped border", "2^30", "NaN", "arrival order", "exactly 0"):
        assert text in doc, text
    doc = lm.deform_points.__doc__
    for text in ("interp(I, h)(y) = I(y + h(y))", "invert_displacement(h)", "landmark_distance("):
        assert text in doc, text


def test_argument_errors_are_raised_on_cpu_tensors():
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    F = torch.zeros((2, 3, 4, 5, 6))
    x = torch.zeros((2, 3, 10))
    g = torch.zeros((2, 3, 10))
    for f in (lm.interp_points, ext.interp_points_forward):
        with pytest.raises(TypeError):
            f(F.numpy(), x)
        with pytest.raises(TypeError):
            f(F, [[0.0]])
        with pytest.raises(RuntimeError, match="float32 and float64"):
            f(F.half(), x.half())
        with pytest.raises(RuntimeError, match="float32 and float64"):
            f(F, x.long())
        with pytest.raises(RuntimeError, match="dtype mismatch"):
            f(F, x.double())
        for bad in (torch.zeros((2, 3, 4)), torch.zeros((2, 3, 4, 5, 6, 7)), torch.zeros((4,))):
            with pytest.raises(RuntimeError, match="two or three spatial axes"):
                f(bad, x)
        for bad in (torch.zeros((2, 2, 10)), torch.zeros((2, 3, 10, 1)), torch.zeros((2, 3))):
            with pytest.raises(RuntimeError, match="point set of shape"):
                f(F, bad)
        with pytest.raises(RuntimeError, match="point set of shape"):
            f(torch.zeros((2, 3, 5, 6)), x)                        # a 2D field takes (N, 2, P)
        with pytest.raises(RuntimeError, match="batch sizes"):
            f(torch.zeros((3, 3, 4, 5, 6)), x)
        with pytest.raises(RuntimeError, match="batch sizes"):
            f(F, x[:1])
        with pytest.raises(RuntimeError, match="x must be contiguous"):
            f(F, torch.zeros((2, 10, 3)).transpose(1, 2))
        with pytest.raises(RuntimeError, match="F must be contiguous"):
            f(torch.zeros((2, 3, 4, 6, 5)).transpose(3, 4), x)
        for FF, xx in ((F, x), (F[:1], x), (F.double(), x.double()), (torch.zeros((2, 1, 5, 6)), torch.zeros((2, 2, 0)))):
            with pytest.raises(RuntimeError, match="CUDA tensor"):   # all fine but for the device
                f(FF, xx)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        lm.interp_points(F.requires_grad_(True), x.clone().requires_grad_(True))
    F = F.detach()
    for bad in (torch.zeros((2, 3, 9)), torch.zeros((2, 2, 10)), torch.zeros((1, 3, 10)), torch.zeros((2, 3, 10, 1))):
        with pytest.raises(RuntimeError, match="grad_out of shape"):
            ext.interp_points_backward(bad, F, x, True, True)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        ext.interp_points_backward(g.double(), F, x, True, True)
    with pytest.raises(TypeError):
        ext.interp_points_backward(None, F, x, True, True)
    with pytest.raises(RuntimeError, match="grad_out must be contiguous"):
        ext.interp_points_backward(torch.zeros((2, 10, 3)).transpose(1, 2), F, x, True, True)
    for need in ((True, True), (True, False), (False, True)):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            ext.interp_points_backward(g, F, x, *need)
    # deform_points: the field must have d channels
    with pytest.raises(RuntimeError, match="displacement field"):
        lm.deform_points(x, torch.zeros((2, 2, 4, 5, 6)))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        lm.deform_points(x, F)
    with pytest.raises(TypeError):
        lm.deform_points(x, F.numpy())


def test_c_entry_points_validate_before_any_device_call():
    from lagomorph_amd import lagomorph_ext as ext

    OK, INVALID = 0, -1
    err = ext._lib.lago_last_error
    p, q, r, s, t = 0x100000, 0x200000, 0x400000, 0x800000, 0x1000000   # never dereferenced: every call returns before a launch
    for suf, elem in (("_f32", 4), ("_f64", 8)):
        f = ext._fn["lago_interp_points" + suf]
        b = ext._fn["lago_interp_points_backward" + suf]

        def both(dim, nn, nc, np_, nx, ny, nz, bc=0):
            """The codes of the forward and of the backward (both gradients wanted) for one problem."""
            return (f(p, q, r, dim, nn, nc, np_, nx, ny, nz, bc, None),
                    b(s, t, p, q, r, dim, nn, nc, np_, nx, ny, nz, bc, 1, 1, None))

        for dim in (1, 4, 0, -3):
            assert both(dim, 1, 1, 8, 4, 4, 4) == (INVALID, INVALID) and b"dimensional" in err()
        for bad in ((-1, 1, 8, 4, 4, 4), (1, -1, 8, 4, 4, 4), (1, 1, -8, 4, 4, 4), (1, 1, 8, -4, 4, 4), (1, 1, 8, 4, -4, 4),
                    (1, 1, 8, 4, 4, -4)):
            assert both(3, *bad) == (INVALID, INVALID) and b"negative" in err(), bad
        assert both(2, 1, 1, 8, 4, -4, 1) == (INVALID, INVALID)
        # a channel plane of 2^32 bytes or more
        big = (1 << 32) // elem
        assert both(3, 1, 1, 8, big // 2048, 1024, 2) == (INVALID, INVALID) and b"2^32 bytes" in err()
        assert both(2, 1, 1, 8, big // 1024, 1024, 1) == (INVALID, INVALID) and b"2^32 bytes" in err()
        assert both(3, 1, 1, 8, 1 << 31, 1 << 31, 1 << 31) == (INVALID, INVALID)
        assert both(3, 1, 1, 8, 1 << 40, 1 << 40, 1 << 40) == (INVALID, INVALID)
        # np >= 2^31
        assert both(3, 1, 1, 1 << 31, 4, 4, 4) == (INVALID, INVALID) and b"2^31 points" in err()
        # an output overlapping an input
        assert f(p, p, r, 3, 1, 1, 8, 4, 4, 4, 0, None) == INVALID and b"overlap" in err()
        assert f(p, q, p + 16, 3, 1, 1, 8, 4, 4, 4, 0, None) == INVALID and b"overlap" in err()
        assert f(p, q, p + 16, 2, 2, 1, 8, 4, 4, 0, 1, None) == INVALID and b"overlap" in err()
        for args in ((s, t, p, s, r), (s, t, s, q, r), (s, t, p, q, s + 8), (s, t, t, q, r), (s, t, p, t, r), (s, t, p, q, t),
                     (s, s, p, q, r)):
            assert b(*args, 3, 1, 1, 8, 4, 4, 4, 0, 1, 1, None) == INVALID and b"overlap" in err(), args
        # an output that is not needed may be null -- and is then not judged for overlap either
        assert b(None, t, p, q, t, 3, 1, 1, 8, 4, 4, 4, 0, 0, 1, None) == INVALID and b"overlap" in err()
        assert b(s, None, s, q, r, 3, 1, 1, 8, 4, 4, 4, 0, 1, 0, None) == INVALID and b"overlap" in err()
        assert b(None, t, p, q, r, 3, 1, 1, 8, 4, 4, 4, 0, 1, 1, None) == INVALID and b"null" in err()
        assert b(s, None, p, q, r, 3, 1, 1, 8, 4, 4, 4, 0, 1, 1, None) == INVALID and b"null" in err()
        assert f(None, q, r, 3, 1, 1, 8, 4, 4, 4, 0, None) == INVALID and b"null" in err()
        assert b(None, None, p, q, r, 3, 1, 1, 8, 4, 4, 4, 0, 0, 0, None) == OK          # neither wanted: nothing to do
        # empty problems: nothing to do
        for empty in ((0, 1, 8, 4, 4, 4), (1, 0, 8, 4, 4, 4), (1, 1, 0, 4, 4, 4), (1, 1, 8, 0, 4, 4), (1, 1, 8, 4, 0, 4),
                      (1, 1, 8, 4, 4, 0)):
            assert f(None, None, None, 3, *empty, 0, None) == OK, empty
            assert b(None, None, None, None, None, 3, *empty, 0, 1, 1, None) == OK, empty
        assert f(None, None, None, 2, 1, 1, 8, 4, 0, 0, 0, None) == OK
        assert b(None, None, None, None, None, 2, 1, 1, 0, 4, 4, 1, 1, 1, 1, None) == OK
