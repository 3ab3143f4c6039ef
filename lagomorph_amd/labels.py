"""Label maps: carrying a segmentation through a deformation, and the overlap of two segmentations.

`interp` blends values, which for labels makes values that do not exist, and K one-hot volumes cost K times the memory
and traffic of one label volume.  `warp_labels` reads the 2^d corner labels of every sample from ONE int32 volume and
picks one of them; `label_overlap` counts two label maps against each other in one pass, and `dice` is plain torch on
that tiny table.  No counterpart in the reference; no CPU path.
"""
import torch

from . import lagomorph_ext

__all__ = ["warp_labels", "label_overlap", "dice"]


def warp_labels(L, u, dt=1.0, mode="vote"):
    """out(x) = the label of L at x + dt u(x).

    L (N or 1, 1, *sp) holds integer labels (uint8, int16, int32 or int64); a leading 1 broadcasts one segmentation to
    every item of u, as `interp` broadcasts I.  u (N, d, *sp), d = len(sp) in {2, 3}, float32 or float64, on the GPU.
    The result is (N, 1, *sp) in L's dtype.  Labels are VALUES, not indices: any int32 pattern is legal (2035,
    -2**31).  The kernels take int32; other dtypes are converted for the call and converted back.  Values of an int64
    tensor outside the int32 range are the caller's error: they are not checked, which would synchronise with the host.

    Per axis with extent n and voxel index i, in u's precision:

        p = i + dt u            the position `interp` samples at, bit for bit
        p = fmin(fmax(p, -1), n)
        f = floor(p), t = p - f
        corners clamp(f, 0, n - 1) and clamp(f + 1, 0, n - 1)

    The clamp of p changes no in-range position; out-of-range, infinite and saturated positions fall on the border
    voxel, a NaN position on the first voxel of its axis.

    mode "nearest": per axis the upper corner where t > 0.5, else the lower (a tie at exactly 0.5 goes to the lower).
    mode "vote" (the default): the 2^d corners, first spatial axis slowest, weigh w_q = (a_x a_y) a_z in float64 (a is
    1 - t for the lower corner and t for the upper; a_y a_z in 2D).  A label's score is the sum of w_q over the corners
    that carry it, in ascending q from 0.0 (clamped corners that coincide each add); the label with the largest score
    wins, the smallest label value among equal scores.  This is the argmax over labels of a trilinearly interpolated
    one-hot encoding, without the K volumes.

    Nothing here is differentiable: the result carries no graph whatever u.requires_grad says.  The same bits from call
    to call.  ValueError for an unknown mode; RuntimeError for shapes or dtypes that do not fit and for CPU tensors.
    """
    with torch.no_grad():
        return lagomorph_ext.warp_labels(L, u.detach() if isinstance(u, torch.Tensor) else u, dt, mode)


def label_overlap(A, B, num_labels):
    """int64 counts (N, K, 3), K = num_labels, of two label maps A and B (N, 1, *sp) of one integer dtype and shape on
    the GPU: per item and label k in [0, K)

        [#(A == k), #(B == k), #(A == k and B == k)]

    A voxel whose label is outside [0, K) counts in nothing for that image.  1 <= K <= 4096 (ValueError otherwise).
    Integer sums without an atomic on memory: the same bits from call to call.  int64 labels outside the int32 range
    are the caller's error (see `warp_labels`)."""
    with torch.no_grad():
        return lagomorph_ext.label_overlap(A, B, num_labels)


def dice(A, B, num_labels, empty=float("nan")):
    """The Dice coefficient 2 #(A == k and B == k) / (#(A == k) + #(B == k)) per item and label, (N, K) float64, from
    `label_overlap`; `empty` where a label occurs in neither image."""
    c = label_overlap(A, B, num_labels)
    both = c[..., 0] + c[..., 1]
    d = 2.0 * c[..., 2].to(torch.float64) / both.to(torch.float64)
    return torch.where(both == 0, torch.full_like(d, float(empty)), d)
