"""Free-form deformations (FFD): a coarse lattice of control points whose uniform cubic B-spline is the dense field
(Rueckert et al. 1999; NiftyReg, elastix, ITK's BSplineTransform), and the adjoint that takes a dense gradient back to
the lattice.  It is the low-dimensional counterpart of the dense displacement the other operators work on, and the usual
model of a smooth multiplicative bias field.

    u = ffd_expand(c, I.shape[2:], spacing)        # (N, d, *sp), voxel units
    J = interp(I, u)                                # or interp_cubic; penalise folding with jacobian_determinant(u)
    R = bending_energy(u)                           # Rueckert's smoothness penalty on the dense field (regularize.py)

Lattice convention, per spatial axis with extent n and integer spacing s (in voxels, 1..32): the lattice has
m = (n - 1) // s + 4 control points and point j sits at voxel (j - 1) s -- one point before the grid and at least two
at or beyond its last voxel, so that every voxel x has its four taps i ... i + 3, i = x // s, inside the lattice:
nothing is folded, mirrored or clamped.  The taps weigh ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6 at
t = (x % s) / s.  A lattice with c[j] = a (j - 1) s + b expands to a x + b; a constant lattice to that constant.  When
(n - 1) % s == 0 the last control point of the axis weighs 0 everywhere.

Fields are channel-first (N, C, *sp) with two or three spatial axes, float32 or float64, contiguous, on the GPU; C is
free (d channels for a displacement, in voxel units as `interp` takes it; 1 for a scalar field).  No counterpart in the
reference; no CPU path.  `bending_energy(ffd_expand(c, shape, s))` penalises the dense field's second derivatives; its
gradient reaches the lattice through `ffd_restrict`.
"""
import torch

from . import lagomorph_ext
from .lagomorph_ext import ffd_grid_shape

__all__ = ["FFDFunction", "ffd_expand", "ffd_grid_shape", "ffd_restrict"]


class FFDFunction(torch.autograd.Function):
    """x -> W x (adjoint False: lattice -> field of spatial `shape`) or x -> W^T x (adjoint True: field -> lattice).
    The operator is linear, so the backward is the same function with `adjoint` flipped: both directions are
    differentiable to any order."""

    @staticmethod
    def forward(ctx, x, shape, spacing, adjoint):
        ctx.adjoint = bool(adjoint)
        ctx.spacing = spacing
        if ctx.adjoint:
            out = lagomorph_ext.ffd_expand_adjoint(x, spacing)
            ctx.shape = tuple(x.shape[2:])
        else:
            out = lagomorph_ext.ffd_expand(x, shape, spacing)
            ctx.shape = tuple(out.shape[2:])
        return out

    @staticmethod
    def backward(ctx, gradout):
        if not ctx.needs_input_grad[0]:   # no kernel runs for a gradient nobody needs
            return None, None, None, None
        return FFDFunction.apply(gradout.contiguous(), ctx.shape, ctx.spacing, not ctx.adjoint), None, None, None


def ffd_expand(ctrl, shape, spacing):
    """out (N, C, *shape): the dense field of the control lattice ctrl (N, C, *ffd_grid_shape(shape, spacing)),
    out[n, k, x, y, z] = sum_{a, b, c} Wx[x, a] Wy[y, b] Wz[z, c] ctrl[n, k, a, b, c] with the banded per-axis matrices
    of the module docstring (2D: two axes).  `shape`: the field's spatial extents, each >= 1; `spacing`: one integer in
    1..32 for every axis, or one per axis, in voxels.  Values are in whatever units ctrl is in: for a displacement fed
    to `interp`, voxels.

    One streaming write of the field; the lattice is read from cache.  The sum has a fixed order (x innermost, then y,
    then z; four taps ascending) and uses no atomics: the bits repeat from call to call, on any stream.  float32
    results are within about 40 ulp-sized units of sum_taps w |ctrl| of the exact sum.

    Differentiable in ctrl to any order (the operator is linear; its backward is `ffd_restrict`).

    RuntimeError for dtypes, shapes or spacings that do not fit, non-contiguous or CPU tensors; TypeError for anything
    that is not a tensor."""
    return FFDFunction.apply(ctrl, shape, spacing, False)


def ffd_restrict(g, spacing):
    """d_ctrl (N, C, *ffd_grid_shape(g.shape[2:], spacing)): the adjoint of `ffd_expand` applied to the field
    g (N, C, *sp), d_ctrl[n, k, a, b, c] = sum_{x, y, z} Wx[x, a] Wy[y, b] Wz[z, c] g[n, k, x, y, z] -- what the backward
    of `ffd_expand` runs, as a public function (the gradient of a loss with respect to the lattice from its gradient
    with respect to the dense field; also the normal equations' right-hand side of a lattice fit).

    One streaming read of g: workgroups reduce voxel tiles in on-chip memory and a second small kernel adds the
    tiles' partial sums in a fixed order.  No atomic touches memory, so the bits repeat from call to call, and a
    control point that no voxel reaches -- the last one of an axis with (n - 1) % s == 0 -- holds exactly 0.

    Differentiable in g to any order.  Errors as for `ffd_expand`."""
    return FFDFunction.apply(g, None, spacing, True)
