"""Image pyramids by a factor of two: the anti-aliased reduce R, the linear expand E and their exact transposes, the
two small linear operators every coarse-to-fine registration loop is built from (Burt and Adelson 1983 for the
1 4 6 4 1 reduce; the prolongation of a multigrid cycle for the expand).

Per spatial axis with fine extent n >= 1 the coarse extent is m = (n + 1) // 2 and coarse voxel j sits at fine voxel
2 j.  Everything is separable and the only border rule is the clamp:

    (R a)[j]     = sum_{k=-2..2} w_k a[clamp(2 j + k, 0, n - 1)],   w = (1, 4, 6, 4, 1) / 16
    (E c)[2 j]   = c[j]
    (E c)[2 j+1] = (c[j] + c[min(j + 1, m - 1)]) / 2

Both preserve constants; E reproduces a linear ramp, R reproduces it away from the border.  Both n = 2 m and
n = 2 m - 1 are fine extents of a coarse extent m, which is why the operators that go up take the fine `shape`.  R^T
and E^T are operators of their own: 2 R^T is not E (it does not preserve constants at the border).

The coarse-to-fine loop:

    pI, pJ = image_pyramid(I), image_pyramid(J)                 # finest first: [I, R I, R R I, ...]
    u = torch.zeros(N, d, *pI[-1].shape[2:], device=I.device)   # a displacement in voxel units (or an ffd lattice)
    for level in reversed(range(len(pI))):
        u = optimise(pI[level], pJ[level], u)                   # interp, a similarity, a regulariser, a few steps
        if level:
            u = pyramid_expand(u, pI[level - 1].shape[2:], scale=2.0)   # voxel units double with the grid

Fields are channel-first (N, C, *sp) with two or three spatial axes, float32 or float64, contiguous, on the GPU; C is
free.  Every result has a fixed evaluation order and no atomics: the bits repeat from call to call, and integer-valued
inputs up to 512 in magnitude give exact results.  Label maps do not belong here (`warp_labels`).  No counterpart in
the reference; no CPU path.
"""
import math

import torch

from . import lagomorph_ext as _ext

__all__ = ["PyramidFunction", "image_pyramid", "pyramid_expand", "pyramid_expand_adjoint", "pyramid_reduce",
           "pyramid_restrict_adjoint", "pyramid_shape"]

PYRAMID_REDUCE, PYRAMID_EXPAND = 0, 1   # LAGO_PYRAMID_* of include/lagomorph_hip.h: which per-axis matrix


def pyramid_shape(shape):
    """Coarse extents for a field of spatial `shape` (two or three extents >= 1): (n + 1) // 2 per axis."""
    try:
        shape = tuple(shape)
        ok = len(shape) in (2, 3) and all(isinstance(n, int) and not isinstance(n, bool) and n >= 1 for n in shape)
    except TypeError:
        ok = False
    if not ok:
        raise RuntimeError(f"pyramid: shape must give two or three spatial axes with extents >= 1, got {shape!r}")
    return tuple((n + 1) // 2 for n in shape)


def _check(x, name, up, shape, scale, what):
    """A coarse field x (N, C, *m) with the fine grid's spatial `shape` (`up`: the two operators that go up), or a fine
    field x (N, C, *sp), `shape` ignored (the two that go down); returns (dim, fine shape, scale).  In the shim's order for
    the newer families: type, dtype, shape (and scale), layout, device last -- so every other error shows on a CPU
    tensor too."""
    _ext._check_types(((name, x),))
    dim = _ext._spatial_frame(x, f"{what}: {name} must be a field of shape (N, C, *spatial) with two or three spatial axes, "
                                 f"got shape {tuple(x.shape)}")[0]
    if min(x.shape[2:]) < 1:
        raise RuntimeError(f"{what}: {name} of shape {tuple(x.shape)} has an empty spatial axis")
    if not up:
        shape = tuple(x.shape[2:])
    else:
        coarse = pyramid_shape(shape)
        shape = tuple(shape)
        if coarse != tuple(x.shape[2:]):
            raise RuntimeError(f"{what}: a coarse field of shape {tuple(x.shape)} does not match the fine grid {shape}: its "
                               f"spatial extents must be {coarse}")
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale):
        raise RuntimeError(f"{what}: scale must be a finite number, got {scale!r}")
    _ext._check_layout(((name, x),))
    return dim, shape, float(scale)


def _launch(entry, op, x, out_shape, dim, shape, scale):
    out = torch.empty(tuple(x.shape[:2]) + tuple(out_shape), dtype=x.dtype, device=x.device)
    _ext._call(entry, x, _ext._ptr(out), _ext._ptr(x), op, dim, x.size(0) * x.size(1), *_ext._pad(shape, 1), scale)
    return out


def _down(x, op, scale, what):
    """scale R x (op PYRAMID_REDUCE) or scale E^T x (PYRAMID_EXPAND) for a fine field x: lago_pyramid_down of
    include/lagomorph_hip.h (csrc/pyramid.hip: pyramid_down_kernel)."""
    dim, shape, scale = _check(x, "x" if op == PYRAMID_REDUCE else "g", False, None, scale, what)
    return _launch("lago_pyramid_down", op, x, pyramid_shape(shape), dim, shape, scale)


def _up(c, shape, op, scale, what):
    """scale E c (op PYRAMID_EXPAND) or scale R^T c (PYRAMID_REDUCE) on the fine grid `shape`: lago_pyramid_up
    (pyramid_up_kernel)."""
    dim, shape, scale = _check(c, "c" if op == PYRAMID_EXPAND else "g", True, shape, scale, what)
    return _launch("lago_pyramid_up", op, c, shape, dim, shape, scale)


class PyramidFunction(torch.autograd.Function):
    """x -> scale M x for one of the four matrices: `expand` False: R (adjoint False, fine -> coarse) or R^T (adjoint
    True, coarse -> fine of spatial `shape`); `expand` True: E (coarse -> fine of spatial `shape`) or E^T.  The
    operators are linear, so the backward is the same function with `adjoint` flipped: all four are differentiable to
    any order."""

    @staticmethod
    def forward(ctx, x, shape, scale, expand, adjoint):
        ctx.expand, ctx.adjoint, ctx.scale = bool(expand), bool(adjoint), scale
        op = PYRAMID_EXPAND if ctx.expand else PYRAMID_REDUCE
        what = (("pyramid_reduce", "pyramid_restrict_adjoint"), ("pyramid_expand", "pyramid_expand_adjoint"))[ctx.expand][ctx.adjoint]
        if ctx.expand != ctx.adjoint:   # E, R^T: up to the fine grid `shape`
            out = _up(x, shape, op, scale, what)
            ctx.shape = tuple(out.shape[2:])
        else:                           # R, E^T: down from x's own grid
            out = _down(x, op, scale, what)
            ctx.shape = tuple(x.shape[2:])
        return out

    @staticmethod
    def backward(ctx, gradout):
        if not ctx.needs_input_grad[0]:   # no kernel runs for a gradient nobody needs
            return None, None, None, None, None
        return PyramidFunction.apply(gradout.contiguous(), ctx.shape, ctx.scale, ctx.expand, not ctx.adjoint), None, None, None, None


def pyramid_reduce(I):
    """out (N, C, *pyramid_shape(sp)) = R I: the next coarser level of I (N, C, *sp), every second voxel of the field
    smoothed with (1 4 6 4 1) / 16 along each axis, the border clamped.  Equal to a strided convolution of the
    replicate-padded field with the binomial kernel; constants are preserved.

    One streaming read of I and one write of an eighth of it.  Differentiable in I to any order (its backward is
    `pyramid_restrict_adjoint`).

    RuntimeError for dtypes or shapes that do not fit, an empty spatial axis, non-contiguous or CPU tensors; TypeError
    for anything that is not a tensor."""
    return PyramidFunction.apply(I, None, 1.0, False, False)


def pyramid_restrict_adjoint(g, shape):
    """out (N, C, *shape) = R^T g for g (N, C, *pyramid_shape(shape)): the exact transpose of `pyramid_reduce`, what
    its backward runs, as a public function.  Not an interpolation: use `pyramid_expand` to carry a field to the finer
    grid.  Differentiable in g to any order.  Errors as for `pyramid_expand`."""
    return PyramidFunction.apply(g, shape, 1.0, False, True)


def pyramid_expand(c, shape, scale=1.0):
    """out (N, C, *shape) = scale E c: the coarse field c (N, C, *pyramid_shape(shape)) carried to the fine grid of
    spatial `shape` by linear prolongation -- even voxels copy their coarse voxel, odd ones average their two
    neighbours.  `scale` multiplies the result: 2.0 for a displacement in voxel units.  Equal to
    F.interpolate(mode="bi/trilinear", align_corners=True) when every fine extent is odd.

    One streaming write of the field.  Differentiable in c to any order (its backward is `pyramid_expand_adjoint`).

    RuntimeError for dtypes or shapes that do not fit -- `shape` must be a fine grid of c's: pyramid_shape(shape) ==
    c.shape[2:] --, a scale that is not finite, non-contiguous or CPU tensors; TypeError for anything that is not a
    tensor."""
    return PyramidFunction.apply(c, shape, scale, True, False)


def pyramid_expand_adjoint(g, scale=1.0):
    """out (N, C, *pyramid_shape(sp)) = scale E^T g for g (N, C, *sp): the exact transpose of `pyramid_expand` (the
    gradient with respect to a coarse field from the gradient with respect to its expansion).  Differentiable in g to
    any order.  Errors as for `pyramid_reduce`."""
    return PyramidFunction.apply(g, None, scale, True, True)


def image_pyramid(I, levels=None, min_size=8):
    """[I, R I, R R I, ...]: the levels of I (N, C, *sp), the finest first.  It stops after `levels` entries (an
    integer >= 1), or -- with levels None, and earlier with both -- before any spatial extent above 1 would drop under
    `min_size` (an integer >= 1).  Differentiable in I.  ValueError for a `levels` or `min_size` that is not such an
    integer; the errors of `pyramid_reduce` for I."""
    for name, v in (("levels", levels), ("min_size", min_size)):
        if not (v is None and name == "levels") and (isinstance(v, bool) or not isinstance(v, int) or v < 1):
            raise ValueError(f"image_pyramid: {name} must be an integer >= 1{' or None' if name == 'levels' else ''}, got {v!r}")
    if not isinstance(I, torch.Tensor):
        raise TypeError("I must be a torch.Tensor")
    out = [I]
    while levels is None or len(out) < levels:
        x = out[-1]
        if isinstance(x, torch.Tensor) and x.dim() in (4, 5) and min(x.shape[2:]) >= 1:
            shape = tuple(x.shape[2:])
            coarse = pyramid_shape(shape)
            if coarse == shape or any(n > 1 and m < min_size for n, m in zip(shape, coarse)):
                break   # (a grid of single voxels has no coarser level)
        out.append(pyramid_reduce(x))   # (anything that is not a field raises here)
    return out
