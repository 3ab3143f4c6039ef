"""Contrast-invariant image similarity: Gaussian-windowed local normalised cross-correlation (``csrc/lncc.hip``).  Not in
the reference, whose only image term is the squared difference.
"""
import torch

from . import lagomorph_ext
from .smooth import _plan

REDUCTIONS = ("mean", "sum", "none")


def _check(I, J, sigma, truncate, mode, eps):
    """(radii, taps) after the argument checks that need no device."""
    for x, nm in ((I, "I"), (J, "J")):
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{nm} must be a torch.Tensor")
    if J.shape != I.shape:
        raise RuntimeError(f"lncc: I {tuple(I.shape)} and J {tuple(J.shape)} must have the same shape")
    if J.dtype != I.dtype:
        raise RuntimeError(f"lncc: dtype mismatch ({I.dtype} vs {J.dtype})")
    if not float(eps) >= 0.0:
        raise ValueError(f"lncc: eps must not be negative (got {eps})")
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
        if mode not in lagomorph_ext.GAUSS_MODES:
            raise ValueError(f"LNCCSimilarity: unknown mode {mode!r} (one of {sorted(lagomorph_ext.GAUSS_MODES)})")
        if not self.eps >= 0.0:
            raise ValueError(f"lncc: eps must not be negative (got {eps})")

    def __call__(self, Idef, img):
        return lncc_loss(Idef, img, self.sigma, truncate=self.truncate, mode=self.mode, eps=self.eps, reduction="sum")
