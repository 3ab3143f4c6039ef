"""Cubic B-spline interpolation: the prefilter that turns samples into coefficients, the 4^d-tap evaluation at
i + dt u(i), and `interp_cubic`, their composition -- the sharp counterpart of the multilinear `interp`.

Multilinear interpolation blurs, and by an amount that varies with the sub-voxel phase; its gradient in the position
jumps at the cell faces.  The cubic B-spline interpolates exactly at the grid points, reproduces cubics and is C^2 in the
position (ITK, elastix, NiftyReg, scipy's `order=3`).  Use it for the final resampling of an image through a recovered
deformation and wherever a similarity's gradient should be continuous in the displacement; inside the shooting loop the
multilinear operators remain the right choice (8 taps instead of 64).

Fields are channel-first (N, C, *sp) with two or three spatial axes, float32 or float64, contiguous, on the GPU.  The
border is a whole-sample mirror (scipy's mode='mirror'); a position outside the grid is clamped to the grid's box first,
so the result there is the border value, as `interp` gives.  No counterpart in the reference; no CPU path.
"""
import torch
from torch.autograd.function import once_differentiable

from . import lagomorph_ext

__all__ = ["BsplinePrefilterFunction", "InterpBsplineFunction", "bspline_prefilter", "interp_bspline", "interp_cubic"]


class BsplinePrefilterFunction(torch.autograd.Function):
    """C = B^-1 I along every spatial axis (adjoint: B^-T); the backward is the same function with `adjoint` flipped."""

    @staticmethod
    def forward(ctx, I, adjoint):
        ctx.adjoint = bool(adjoint)
        return lagomorph_ext.bspline_prefilter(I, ctx.adjoint)

    @staticmethod
    @once_differentiable
    def backward(ctx, gradout):
        if not ctx.needs_input_grad[0]:
            return None, None
        return lagomorph_ext.bspline_prefilter(gradout.contiguous(), not ctx.adjoint), None


class InterpBsplineFunction(torch.autograd.Function):
    """out[n, k, i] = the spline with coefficients C[n or 0, k] at i + dt u[n, :, i]; backward = scatter of grad onto
    the 4^d folded taps (d_C) + the position gradient (d_u), one kernel (csrc/bspline.hip).  A gradient that is not
    needed is not computed and comes back as None."""

    @staticmethod
    def forward(ctx, C, u, dt):
        out = lagomorph_ext.interp_bspline_forward(C, u, dt)   # (first: it raises for what is not a pair of tensors)
        ctx.dt = float(dt)
        ctx.save_for_backward(C, u)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gradout):
        C, u = ctx.saved_tensors
        d_C, d_u = lagomorph_ext.interp_bspline_backward(gradout.contiguous(), C, u, ctx.dt, *ctx.needs_input_grad[:2])
        return d_C, d_u, None


def bspline_prefilter(I, adjoint=False):
    """Cubic B-spline coefficients C (N, C, *sp) of the samples I (N, C, *sp): the spline through C takes the values I at
    the grid points.

    Per spatial axis of extent n, axes in order; n = 1 is the identity.  Otherwise c solves B c = f, B the (1, 4, 1) / 6
    tridiagonal with a MIRROR border (whole-sample reflection of period 2n - 2: first row (4, 2) / 6, last row
    (2, 4) / 6) -- scipy's `spline_filter(order=3, mode='mirror')`.  A causal and an anticausal first-order recursion
    per line with pole sqrt(3) - 2 and gain 6; ||B^-1||_inf = 3 per axis, so the coefficients are at most 3^d times the
    samples.  float32 results are within about 1e-6 max|I| of the float64 ones.  No atomics: the bits repeat from call
    to call.

    adjoint=True applies B^-T instead (B is not symmetric: its end rows differ); it is what the backward of
    adjoint=False runs, and the reverse.  Differentiable in I (once).

    RuntimeError for shapes or dtypes that do not fit, non-contiguous or CPU tensors; TypeError for anything that is
    not a tensor."""
    return BsplinePrefilterFunction.apply(I, adjoint)


def interp_bspline(C, u, dt=1.0):
    """out (N, K, *sp): the cubic B-spline with coefficients C (N or 1, K, *sp) evaluated at i + dt u(i) for every
    voxel i; u (N, d, *sp) in voxel units.  A leading 1 broadcasts one coefficient field to every item of u.

    Per axis with extent n: the position -- formed as `interp` forms it -- is CLAMPED to [0, n - 1] first; then
    f = min(floor(x), n - 2), t = x - f, the taps f - 1 ... f + 2 weigh
    ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6 and are folded once into the grid (k -> |k|, then
    k -> 2 (n - 1) - k if k > n - 1; for n = 1 every tap is index 0).  Consequences:

    - `interp_bspline(bspline_prefilter(I), 0)` returns I (to rounding), and the result equals scipy's
      `map_coordinates(order=3, mode='mirror', prefilter=False)` at the clamped positions;
    - a position outside the grid gives the value at the nearest point of the grid's box, +-inf included, and no
      `2^30` domain limit applies; no position addresses outside C;
    - a NaN coordinate gives NaN for that voxel (all K channels) and for no other.

    The sum has a fixed order (z innermost, then y, then x): the bits repeat from call to call.

    Differentiable in C and in u (once: the backward is not itself differentiable).

    - d_u[n, a, i] = dt sum_k g[n, k, i] dS_k/dx_a with the derivative weights
      (-(1-t)^2, 3t^2 - 4t, -3t^2 + 2t + 1, t^2) / 2 along axis a.  It is continuous in u -- the point of the cubic
      spline -- and exactly zero along an axis on which the position was clamped (continuously so: the mirror makes the
      derivative vanish at both borders).  A voxel with a NaN coordinate gets NaN in every component.  No atomics:
      the bits repeat from call to call.
    - d_C is shaped like C, summed over the items when C is broadcast.  Every voxel adds w g to its 4^d folded taps,
      w = (w_x w_y) w_z in C's precision (w_y w_z in 2D); a voxel with a NaN coordinate adds nothing.  The adds are
      hardware float atomics on memory, so the LAST BITS of d_C depend on their arrival order and are not reproducible
      from call to call, as for `interp`'s d_I and `interp_points`' d_F.  Cells that receive nothing hold exactly 0.

    RuntimeError for shapes, dtypes or batch sizes that do not fit, non-contiguous or CPU tensors; TypeError for
    anything that is not a tensor."""
    return InterpBsplineFunction.apply(C, u, dt)


def interp_cubic(I, u, dt=1.0):
    """out (N, C, *sp): the image I (N or 1, C, *sp) resampled with cubic B-spline interpolation at i + dt u(i) --
    `interp_bspline(bspline_prefilter(I), u, dt)`, the drop-in for `interp(I, u, dt)` where sharpness or a continuous
    gradient matters.  `interp_cubic(I, 0)` is I.  To resample one image through several displacements, prefilter
    once and call `interp_bspline`.  Differentiable in I and u; d_I = B^-T d_C carries the call-to-call variation of
    d_C's last bits (see `interp_bspline`)."""
    lagomorph_ext._check_bspline(I, u, "interp_cubic")   # both arguments, before the prefilter runs
    return interp_bspline(bspline_prefilter(I), u, dt)
