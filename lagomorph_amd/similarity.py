"""Image similarity beyond the squared difference: Gaussian-windowed local normalised cross-correlation for a locally
affine change of contrast (``csrc/lncc.hip``), and mutual information over a Parzen-window joint histogram for two
modalities (``csrc/mi.hip``).  Not in the reference, whose only image term is the squared difference.
"""
import math

import torch

from . import lagomorph_ext
from .smooth import _plan

REDUCTIONS = ("mean", "sum", "none")


def _pair(I, J, what):
    """The image pair of the similarity `what`: two tensors of one shape and dtype, wherever they live.  The binding's own
    pair checks (lagomorph_ext: _check_lncc_pair, _check_mi) go on to the dtype's kind, the axes and the device."""
    lagomorph_ext._check_tensors((("I", I), ("J", J)))
    lagomorph_ext._check_same_shape(I, J, what)
    if J.dtype != I.dtype:
        raise RuntimeError(f"{what}: dtype mismatch ({I.dtype} vs {J.dtype})")


def _lncc_eps(eps):
    if not float(eps) >= 0.0:
        raise ValueError(f"lncc: eps must not be negative (got {eps})")
    return float(eps)


def _check(I, J, sigma, truncate, mode, eps):
    """(radii, taps) after the argument checks that need no device."""
    _pair(I, J, "lncc")
    _lncc_eps(eps)
    return _plan(I, sigma, truncate, mode)


class LNCCFunction(torch.autograd.Function):
    """cc = sX^2 / (sI sJ + eps) with a hand-written backward (csrc/lncc.hip).

    Memory: the forward saves I, J and the FIVE windowed moments (G I, G J, G(I I), G(I J), G(J J)) -- five extra
    volumes per (n, c) field beside the inputs -- so that the backward starts from them instead of filtering again.  The
    backward forms the three (one input) or five (both) coefficient fields in one pointwise kernel, filters them with
    one stacked call of the gaussian_smooth passes, and combines them with I and J in one more pointwise kernel, for the
    inputs that need a gradient only.  It is not itself differentiable (once_differentiable)."""

    @staticmethod
    def forward(ctx, I, J, sigma, truncate, mode, eps):
        radii, taps = _plan(I, sigma, truncate, mode)
        I, J = I.contiguous(), J.contiguous()
        mom = lagomorph_ext.lncc_moments(I, J, radii, taps, mode)
        ctx.save_for_backward(I, J, mom)
        ctx.args = (radii, taps, mode, eps)
        return lagomorph_ext.lncc_cc(mom, eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gradout):
        I, J, mom = ctx.saved_tensors
        radii, taps, mode, eps = ctx.args
        d_I, d_J = lagomorph_ext.lncc_backward(gradout.contiguous(), I, J, mom, radii, taps, mode, eps,
                                               need_I=ctx.needs_input_grad[0], need_J=ctx.needs_input_grad[1])
        return d_I, d_J, None, None, None, None


def lncc(I, J, sigma, truncate=4.0, mode="wrap", eps=1e-5):
    """The map of local normalised cross-correlations of I and J (N, C, *sp), len(sp) in {2, 3}, float32 or float64, on
    the GPU:

        A = G I,  B = G J,  C = G(I I),  D = G(I J),  E = G(J J)
        sI = C - A^2,  sJ = E - B^2,  sX = D - A B,   cc = sX^2 / (sI sJ + eps)

    with G the operator of `gaussian_smooth(., sigma, truncate, mode)`: the same per-axis sigma and truncate rule, the
    same modes "wrap" and "zero", the same radius cap (ValueError above 32 taps a side).  Nothing is clamped: cc lies in
    [0, 1] up to rounding where the window variances are well resolved; eps >= 0 only guards flat regions.  cc is
    invariant to an affine change of contrast of either image (for eps = 0, mode "wrap") and symmetric in (I, J) bit for
    bit.  With mode "zero" the windows near the border hold less than the full weight: there C - A^2 is not a variance,
    an offset of an image does not cancel (a scaling still does); subtract the mean first.

    Accuracy in float32: the variances are differences of windowed means, C - A^2, so their rounding error is relative
    to the local mean SQUARE, not to the variance.  Where a window holds few samples (a sigma of 0.5, an extent of 2
    or a singleton axis under a per-axis sigma) and the local variance is small against the local mean square (an image
    with a large offset), float32 loses digits that no kernel can give back -- a property of the formula.  The float32
    results are held to 1e-5 of max|cc| on zero-mean or moderately offset images with windows of a voxel or more; images
    with a singleton spatial axis and strongly offset images under sub-voxel windows are outside what is tested.
    Subtract the mean or use float64 there.

    Differentiable once with respect to I and J (`LNCCFunction`: five extra volumes are kept for the backward).
    Non-contiguous input is made contiguous; an empty batch returns an empty tensor.  Deterministic (no atomics)."""
    _check(I, J, sigma, truncate, mode, eps)   # argument errors before autograd records anything
    return LNCCFunction.apply(I, J, sigma, float(truncate), mode, float(eps))


def lncc_loss(I, J, sigma, truncate=4.0, mode="wrap", eps=1e-5, reduction="mean"):
    """1 - lncc(I, J, ...) reduced by "mean", "sum" or "none" (the map itself)."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"lncc_loss: unknown reduction {reduction!r} (one of {list(REDUCTIONS)})")
    d = 1.0 - lncc(I, J, sigma, truncate=truncate, mode=mode, eps=eps)
    if reduction == "none":
        return d
    return d.mean() if reduction == "mean" else d.sum()


class LNCCSimilarity:
    """The image term `(Idef, img) -> (1 - cc).sum()` for `lddmm_step(..., similarity=...)`: the counterpart of
    `mse_loss(Idef, img, reduction="sum")`, which the step divides by the number of voxels."""

    def __init__(self, sigma, truncate=4.0, mode="wrap", eps=1e-5):
        self.sigma, self.truncate, self.mode, self.eps = sigma, float(truncate), mode, float(eps)
        lagomorph_ext._gauss_mode("LNCCSimilarity", mode)
        _lncc_eps(eps)

    def __call__(self, Idef, img):
        return lncc_loss(Idef, img, self.sigma, truncate=self.truncate, mode=self.mode, eps=self.eps, reduction="sum")


# ---- mutual information

def _auto_range(x, name):
    """(min, max) of x, detached; (lo, lo + 1) for a constant image.  A host synchronisation."""
    if x.numel() == 0:
        return 0.0, 1.0
    lo, hi = (float(v) for v in torch.aminmax(x.detach()))
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"mutual_information: {name} holds NaN or inf voxels, its range cannot be taken from it: "
                         f"pass {name} explicitly")
    return (lo, hi) if lo < hi else (lo, lo + 1.0)


def _mi_check(I, J, bins, range_I, range_J):
    """(bins, range_I, range_J) after the argument checks; a range of None is taken from the tensor."""
    _pair(I, J, "mutual_information")
    bins = lagomorph_ext.mi_bins(bins)
    range_I = _auto_range(I, "range_I") if range_I is None else lagomorph_ext.mi_range(range_I, "range_I")
    range_J = _auto_range(J, "range_J") if range_J is None else lagomorph_ext.mi_range(range_J, "range_J")
    return bins, range_I, range_J


def _mi_eps(eps):
    eps = float(eps)
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError(f"mutual_information: eps must be positive (got {eps}): an empty bin would give log 0")
    return eps


class JointHistogramFunction(torch.autograd.Function):
    """P = joint_histogram(I, J) with a hand-written backward (csrc/mi.hip).  Only I and J are saved: the backward reads
    the upstream gradient on the (N, C, B, B) table and gathers from it per voxel, for the inputs that need a gradient
    only.  It is not itself differentiable (once_differentiable)."""

    @staticmethod
    def forward(ctx, I, J, bins, range_I, range_J):
        I, J = I.contiguous(), J.contiguous()
        ctx.save_for_backward(I, J)
        ctx.args = (bins, range_I, range_J)
        return lagomorph_ext.mi_histogram(I, J, bins, range_I, range_J)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        I, J = ctx.saved_tensors
        d_I, d_J = lagomorph_ext.mi_backward(G.contiguous(), I, J, *ctx.args, need_I=ctx.needs_input_grad[0],
                                             need_J=ctx.needs_input_grad[1])
        return d_I, d_J, None, None, None


def _fold_sum(x):
    """The sum over the last axis in a FIXED order: padded with zeros to a power of two, then the upper half added onto
    the lower half until one entry is left.  torch.sum picks its reduction tree by shape and device; with this the bits of
    the entropies follow from P alone, as P's own bits follow from the images alone.  It matters where MI is small against
    the entropies it is the difference of: there a last-bit difference of an entropy is a large relative one of MI.
    A level is written as the sum over an axis of extent two -- one addition per entry, whatever the tree -- which
    autograd differentiates with one expand (two slices would cost a zero-fill and a copy each)."""
    n = 1
    while n < x.shape[-1]:
        n *= 2
    if n != x.shape[-1]:
        x = torch.nn.functional.pad(x, (0, n - x.shape[-1]))
    while n > 1:
        n //= 2
        x = x.unflatten(-1, (2, n)).sum(-2)
    return x[..., 0]


def joint_histogram(I, J, bins=32, range_I=None, range_J=None):
    """The Parzen-window joint histogram P (N, C, bins, bins), float64, of I and J (N, C, *sp), len(sp) in {2, 3},
    float32 or float64, on the GPU: each of the N C scalar fields gets its own table, 4 <= bins <= 64.  With the range
    (lo, hi) of an image and B = bins, per voxel in double,

        c = (min(max(v, lo), hi) - lo) (B - 3) / (hi - lo) + 1,  k = floor(c) - 1 (in [0, B - 4]),  t = c - (k + 1)

    and the four cubic B-spline weights of t go to bins k..k+3 of that image's axis; P sums the products of the two
    images' weights over the voxels, divided by their number.  Values outside a range are clamped to it, a NaN voxel
    counts as lo.  The sum is taken in 64-bit fixed point (32 fraction bits): P has the same bits from call to call, on
    any stream, and P of (J, I) is the transpose of P of (I, J) bit for bit.  Every row and column of P sums to the
    marginal of one image, all of P to 1 (up to the 2^-33 a product is rounded by).

    A range of None is `torch.aminmax` of that tensor (of the whole tensor, detached; a constant image gets
    (lo, lo + 1)): a host synchronisation, so such a call cannot be captured in a graph -- pass the ranges for that.
    An explicit range needs finite bounds lo < hi (ValueError).

    Differentiable once with respect to I and J (`JointHistogramFunction`), with the derivative of the window where
    lo <= v <= hi and 0 for clamped, infinite and NaN voxels.  Non-contiguous input is made contiguous; an empty batch
    returns an empty tensor."""
    bins, range_I, range_J = _mi_check(I, J, bins, range_I, range_J)   # argument errors before autograd records anything
    return JointHistogramFunction.apply(I, J, bins, range_I, range_J)


def mutual_information(I, J, bins=32, range_I=None, range_J=None, normalized=False, eps=1e-10):
    """The mutual information of I and J (N, C, *sp) per scalar field, (N, C) in I.dtype, from P = `joint_histogram`:

        a = P.sum(-1),  b = P.sum(-2)
        H_I = -sum a log(a + eps),  H_J = -sum b log(b + eps),  H_IJ = -sum P log(P + eps)
        MI = H_I + H_J - H_IJ,      or (H_I + H_J) / H_IJ with normalized=True

    in float64 on the tiny tables, by plain torch operations.  Every sum is taken in one fixed order (`_fold_sum`: the
    upper half of the zero-padded axis onto the lower, repeatedly; the last axis of P first in H_IJ), so MI has the same
    bits from call to call whatever reduction torch would choose.  eps > 0 is required: a bin whose every product rounds to
    0 still has a derivative, and log 0 would reach the voxels' gradients."""
    eps = _mi_eps(eps)
    P = joint_histogram(I, J, bins=bins, range_I=range_I, range_J=range_J)
    a, b = _fold_sum(P), _fold_sum(P.transpose(-1, -2))
    h_i = -_fold_sum(a * torch.log(a + eps))
    h_j = -_fold_sum(b * torch.log(b + eps))
    h_ij = -_fold_sum(_fold_sum(P * torch.log(P + eps)))
    mi = (h_i + h_j) / h_ij if normalized else h_i + h_j - h_ij
    return mi.to(I.dtype)


def mi_loss(I, J, bins=32, range_I=None, range_J=None, normalized=False, eps=1e-10, reduction="mean"):
    """-mutual_information(I, J, ...) reduced by "mean", "sum" or "none" (the (N, C) values themselves)."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"mi_loss: unknown reduction {reduction!r} (one of {list(REDUCTIONS)})")
    d = -mutual_information(I, J, bins=bins, range_I=range_I, range_J=range_J, normalized=normalized, eps=eps)
    if reduction == "none":
        return d
    return d.mean() if reduction == "mean" else d.sum()


class MISimilarity:
    """The image term `(Idef, img) -> -(MI summed over the fields) x voxels per field` for
    `lddmm_step(..., similarity=...)`: the step divides by the number of elements, which leaves minus the mean mutual
    information.  With a range of None every call synchronises with the host (`joint_histogram`)."""

    def __init__(self, bins=32, range_I=None, range_J=None, normalized=False, eps=1e-10):
        self.bins = lagomorph_ext.mi_bins(bins)
        self.range_I = None if range_I is None else lagomorph_ext.mi_range(range_I, "range_I")
        self.range_J = None if range_J is None else lagomorph_ext.mi_range(range_J, "range_J")
        self.normalized, self.eps = bool(normalized), _mi_eps(eps)

    def __call__(self, Idef, img):
        nvox = math.prod(Idef.shape[2:])
        return mi_loss(Idef, img, bins=self.bins, range_I=self.range_I, range_J=self.range_J, normalized=self.normalized,
                       eps=self.eps, reduction="sum") * nvox
