"""Distances between segmentations: the exact Euclidean distance transform of a label map, the signed distance map of a
structure, and the surface distances (Hausdorff, its 95th percentile, average symmetric surface distance) of two label
maps.

`label_overlap` says how much two structures share; it does not see a boundary that is a centimetre off along one side.
The surface distances do, and they rest on the distance transform, which is also what turns a segmentation into the
smooth shape image (a signed distance map) that `lddmm_step` or `lncc` can register.  `distance_transform` runs one
kernel pass per axis on ONE int32 volume; the rest is plain torch on its results.  No counterpart in the reference; no
CPU path.
"""
import torch

from . import lagomorph_ext

__all__ = ["distance_transform", "signed_distance", "surface_mask", "surface_distance"]


def distance_transform(L, where="nonzero", label=0, spacing=1.0, squared=False):
    """The Euclidean distance from every voxel centre to the nearest FEATURE voxel of the same batch item, float32
    (N, 1, *sp); 0 on features, +inf everywhere in an item that has none.

    L (N, 1, *sp) holds integer labels (uint8, int16, int32, int64 or bool; converted to int32 for the call, as
    `warp_labels` does), two or three spatial axes, each extent in 1..1024, contiguous, on the GPU.  `where` chooses
    the features:

        "nonzero"     L != 0
        "equal"       L == label
        "not_equal"   L != label
        "surface"     L == label with at least one of the 2 d face neighbours != label; a neighbour outside the volume
                      counts as different.  This is m & ~scipy.ndimage.binary_erosion(m) with the default structure
                      and border_value=0, evaluated as the first pass loads its lines: no mask volume is written.

    spacing is one positive float or one per axis; the squared distance is sum_a (s_a delta_a)^2.  The transform is
    separable and exact: one pass per axis, each per line out[i] = min_j g[j] + (s (i - j))^2 in float32 with nothing
    fused.  With unit spacing every value is an integer below 2^24, so squared=True returns the exact squared distance
    and squared=False its correctly rounded square root.  With other spacings no term is negative, nothing cancels,
    and the squared distance is within 8 * 2^-24 relative of the real value.

    Not differentiable: the result carries no graph.  The same bits from call to call.  ValueError for an unknown
    `where`, a non-positive spacing or a label outside int32; RuntimeError for shapes, dtypes, extents above 1024,
    non-contiguous and CPU tensors; TypeError for a non-tensor.
    """
    with torch.no_grad():
        return lagomorph_ext.distance_transform(L, where, label, spacing, squared)


def signed_distance(L, label=None, spacing=1.0):
    """The signed distance map of a structure, float32 (N, 1, *sp): negative inside, positive outside.

    Outside the structure it is the distance to its nearest voxel, inside minus the distance to the nearest voxel
    that is not part of it: distance_transform(where="equal") - distance_transform(where="not_equal") for a `label`,
    and for label=None the structure is L != 0 (the second transform is taken of L == 0).  Both are distances between
    voxel CENTRES, so the map steps from -1 to +1 (times the spacing) across a face of the structure and is never 0.

    Where one side is empty the result is the other side's infinity: -inf everywhere in an item that the structure
    fills, +inf everywhere in an item it does not occur in.  Not differentiable.
    """
    if label is None:
        outside = distance_transform(L, "nonzero", 0, spacing)
        inside = distance_transform(L == 0 if isinstance(L, torch.Tensor) else L, "nonzero", 0, spacing)
    else:
        outside = distance_transform(L, "equal", label, spacing)
        inside = distance_transform(L, "not_equal", label, spacing)
    return outside - inside   # one of the two is 0 at every voxel: never inf - inf


def surface_mask(L, label):
    """bool (N, 1, *sp): the surface voxels of the structure L == label, by the predicate of
    distance_transform(where="surface") itself -- the voxels where that transform is 0 -- so that there is no second
    implementation of the stencil to keep in step with the kernel's."""
    return distance_transform(L, "surface", label, 1.0, squared=True) == 0


def _quantile(x, q):
    """numpy's default (linear) percentile of a sorted float64 vector with at least one element."""
    pos = q * (x.numel() - 1)
    lo = int(pos)
    hi = min(lo + 1, x.numel() - 1)
    return x[lo] + (x[hi] - x[lo]) * (pos - lo)


def surface_distance(A, B, labels, spacing=1.0):
    """The surface distances of two label maps A, B (N, 1, *sp) per item and per label of `labels` (K integers): a dict
    of float64 (N, K) tensors on A's device.

    With d_AB the values of distance_transform(B, "surface", k, spacing) at the surface voxels of A == k, and d_BA the
    same the other way round (both float32 distances, widened to float64 for what follows):

        "hausdorff"   max(max d_AB, max d_BA)
        "hd95"        max(q(d_AB), q(d_BA)), q the 0.95 quantile with linear interpolation (numpy's default percentile)
        "assd"        (sum d_AB + sum d_BA) / (|d_AB| + |d_BA|)

    nan where either surface is empty.  The surface voxels are selected with `surface_mask`, the kernel's own
    predicate.  Every voxel counts once; there is no surfel-area weighting.

    The boolean selection synchronises with the host, per item and label: this is an evaluation metric, not a loop
    body.
    """
    if isinstance(A, torch.Tensor) and isinstance(B, torch.Tensor) and A.shape != B.shape:
        raise RuntimeError(f"surface_distance: A {tuple(A.shape)} and B {tuple(B.shape)} must have the same shape")
    labels = [int(k) for k in labels]
    res = None
    for c, k in enumerate(labels):
        dA, dB = distance_transform(A, "surface", k, spacing), distance_transform(B, "surface", k, spacing)
        sA, sB = surface_mask(A, k), surface_mask(B, k)
        if res is None:
            res = {name: torch.full((A.size(0), len(labels)), float("nan"), dtype=torch.float64, device=A.device)
                   for name in ("hausdorff", "hd95", "assd")}
        for n in range(A.size(0)):
            d_ab = dB[n][sA[n]].to(torch.float64).sort().values
            d_ba = dA[n][sB[n]].to(torch.float64).sort().values
            if d_ab.numel() == 0 or d_ba.numel() == 0:
                continue
            res["hausdorff"][n, c] = torch.maximum(d_ab[-1], d_ba[-1])
            res["hd95"][n, c] = torch.maximum(_quantile(d_ab, 0.95), _quantile(d_ba, 0.95))
            res["assd"][n, c] = (d_ab.sum() + d_ba.sum()) / (d_ab.numel() + d_ba.numel())
    if res is None:   # no labels: the argument checks still run
        lagomorph_ext.distance_transform(A, "surface", 0, spacing, True)
        lagomorph_ext.distance_transform(B, "surface", 0, spacing, True)
        res = {name: torch.empty((A.size(0), 0), dtype=torch.float64, device=A.device) for name in ("hausdorff", "hd95", "assd")}
    return res
