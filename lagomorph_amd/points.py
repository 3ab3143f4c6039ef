"""Point sets: sampling an image or a deformation at a list of positions, carrying landmarks through a deformation, and
the distance between two landmark sets (target registration error).

`interp`, `compose`, `warp_labels` and `Ad_star` evaluate at i + dt u(i) for EVERY voxel i of the grid.  The operators
here evaluate at positions that the caller lists: landmarks, fiducials, mesh vertices.  A point set is a tensor x of
shape (N, d, P), channel-first like every field of this library, d = len(sp) in {2, 3}, in voxel-index units along the
spatial axes in order -- the coordinates `identity()` gives -- so a field (N, d, *sp) reshaped to (N, d, -1) already is
a point set.  Tensors are float32 or float64, contiguous, on the GPU.  No counterpart in the reference; no CPU path.
"""
import torch
from torch.autograd.function import once_differentiable

from . import lagomorph_ext

__all__ = ["InterpPointsFunction", "interp_points", "deform_points", "landmark_distance"]


class InterpPointsFunction(torch.autograd.Function):
    """out[n, c, p] = F[n or 0, c] at x[n, :, p]; backward = scatter of grad onto the 2^d corners (d_F) + the position
    gradient of the multilinear value (d_x), one kernel each way (csrc/points.hip).  A gradient that is not needed is
    not computed and comes back as None."""

    @staticmethod
    def forward(ctx, F, x):
        out = lagomorph_ext.interp_points_forward(F, x)   # (first: it raises for what is not a pair of tensors)
        ctx.save_for_backward(F, x)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gradout):
        F, x = ctx.saved_tensors
        d_F, d_x = lagomorph_ext.interp_points_backward(gradout.contiguous(), F, x, *ctx.needs_input_grad[:2])
        return d_F, d_x


def interp_points(F, x):
    """out (N, C, P) with out[n, c, p] = F[n or 0, c] sampled multilinearly at the position x[n, :, p].

    F (N or 1, C, *sp): a leading 1 broadcasts one image to every item of x, as `interp` broadcasts I.  x (N, d, P) in
    voxel-index units.  The arithmetic is `interp`'s at the same position, expression for expression: with
    x = (identity + u).reshape(N, d, -1) the result is `interp(F, u).reshape(N, C, -1)` bit for bit.  Per axis with
    extent n: f = floor(x), t = x - f, corners clamp(f, 0, n - 1) and clamp(f + 1, 0, n - 1).  Consequences:

    - a position outside the grid reads the clamped border (the value at the nearest point of the grid's box);
    - the domain is |x| < 2^30 (the floor saturates there);
    - a coordinate that is not finite gives NaN for that point and never an access outside F: every corner index is
      clamped before it is used.

    Differentiable in F and in x (once: the backward is not itself differentiable).

    - d_x[n, a, p] = sum_c g[n, c, p] dF_c/dx_a, with c ascending from the c = 0 term.  It is the one-sided derivative
      of the cell floor(x) -- the function is piecewise multilinear, its gradient jumps at the cell faces -- and zero
      along an axis on which both clamped corners coincide (outside the grid, or an extent of 1).  No atomics: the
      bits repeat from call to call.
    - d_F is shaped like F, summed over the items when F is broadcast.  Every point adds w_q g to its 2^d clamped
      corners, w_q = (a_x a_y) a_z in F's precision (a = 1 - t for the lower corner, t for the upper; a_y a_z in 2D).
      The adds are hardware float atomics on memory, so the LAST BITS of d_F depend on their arrival order and are
      not reproducible from call to call, as for `interp`'s d_I.  Cells that receive nothing hold exactly 0.

    RuntimeError for shapes, dtypes or batch sizes that do not fit, non-contiguous or CPU tensors; TypeError for
    anything that is not a tensor."""
    return InterpPointsFunction.apply(F, x)


def deform_points(x, u, dt=1.0):
    """x + dt u(x): the points x (N, d, P) moved by the displacement field u (N or 1, d, *sp), (N, d, P).

    Direction.  `interp(I, h)(y) = I(y + h(y))`: the deformed image at y shows I at y + h(y).  So
    `deform_points(x, h)` takes points given in the frame of the DEFORMED image `interp(I, h)` into the frame of I --
    the direction in which h itself points, opposite to the one in which the image content moves.  In the atlas step
    the atlas I is deformed onto each subject, `interp(I, h)` against the subject's image, so with the h that `expmap`
    returns landmarks picked on the subject go to the atlas.  Carrying points the other way, from the frame of I into
    the frame of the deformed image, needs the inverse: `deform_points(x, invert_displacement(h))`.

    Target registration error is `landmark_distance(deform_points(x_subject, h), x_atlas, spacing)` for corresponding
    landmarks x_subject (in the frame of the deformed image) and x_atlas (in the frame of I).

    Composed in Python, not fused: `x + dt * interp_points(u, x)` (for dt = 1 the multiplication, which changes no
    bit, is left out), differentiable in x and u through `interp_points`.  The elementwise passes stream 12 to 20 bytes
    per point and coordinate beside the 8 d gathered values; their measured share is in profiles/points_timing.md."""
    if isinstance(u, torch.Tensor) and isinstance(x, torch.Tensor) and u.dim() >= 2 and x.dim() == 3 and u.size(1) != x.size(1):
        raise RuntimeError(f"deform_points: u must be a displacement field with {x.size(1)} channels for points of "
                           f"shape {tuple(x.shape)}, got shape {tuple(u.shape)}")
    v = interp_points(u, x)
    return x + v if dt == 1.0 else x + dt * v


def landmark_distance(x, y, spacing=None, squared=False):
    """(N, P): the Euclidean distance sqrt(sum_a (spacing_a (x_a - y_a))^2) between corresponding points of x (N, d, P)
    and y (N or 1, d, P).  `spacing`: a length-d sequence of voxel sizes (all ones by default), so that the result is in
    physical units.  squared=True leaves the root out, for use as a loss: its gradient is finite at zero distance.
    Plain torch, on any device, differentiable."""
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise TypeError("landmark_distance: x and y must be torch.Tensors")
    if x.dim() != 3 or y.dim() != 3 or y.size(1) != x.size(1) or y.size(2) != x.size(2) or y.size(0) not in (1, x.size(0)):
        raise RuntimeError(f"landmark_distance: x {tuple(x.shape)} must be (N, d, P) and y {tuple(y.shape)} (N or 1, d, P)")
    diff = x - y
    if spacing is not None:
        sp = [float(s) for s in spacing]
        if len(sp) != x.size(1):
            raise RuntimeError(f"landmark_distance: spacing must have {x.size(1)} entries, got {len(sp)}")
        diff = diff * torch.tensor(sp, dtype=diff.dtype, device=diff.device).view(1, -1, 1)
    d2 = (diff * diff).sum(1)
    return d2 if squared else d2.sqrt()
