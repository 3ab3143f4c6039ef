"""Spatial Gaussian smoothing (``csrc/gauss.hip``).  Not in the reference, whose only smoothing operator is the fluid
metric's FFT kernel; a separable filter with a few taps per axis is the cheaper tool for narrow kernels, and the
building block of windowed statistics.
"""
import numbers

import numpy as np
import torch

from . import lagomorph_ext

MAX_RADIUS = lagomorph_ext.GAUSS_MAX_RADIUS


def _radius(sigma, truncate):
    return int(truncate * sigma + 0.5) if sigma > 0 else 0


def gaussian_taps(sigma, truncate=4.0):
    """The 2 r + 1 float64 taps w_k = exp(-k^2 / (2 sigma^2)), k = -r..r, divided by their sum, with
    r = int(truncate * sigma + 0.5): the rule of scipy.ndimage.gaussian_filter.  sigma <= 0 (or r == 0) gives [1.]."""
    sigma = float(sigma)
    r = _radius(sigma, float(truncate))
    if r == 0:
        return np.ones(1, dtype=np.float64)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / w.sum()


def _per_axis(sigma, dim):
    if isinstance(sigma, numbers.Real):
        return [float(sigma)] * dim
    sigma = [float(s) for s in sigma]
    if len(sigma) != dim:
        raise ValueError(f"gaussian_smooth: sigma must be a number or {dim} numbers, one per spatial axis "
                         f"(got {len(sigma)})")
    return sigma


def _plan(x, sigma, truncate, mode):
    """(radii, taps) per spatial axis after the argument checks that need no device."""
    lagomorph_ext._gauss_mode("gaussian_smooth", mode)
    dim = lagomorph_ext._spatial_frame(x, lagomorph_ext._GAUSS_DIMS)[0]
    sig = _per_axis(sigma, dim)
    radii = [_radius(s, float(truncate)) for s in sig]
    for s, r in zip(sig, radii):
        if r > MAX_RADIUS:
            raise ValueError(f"gaussian_smooth: sigma {s} with truncate {truncate} needs {r} taps on each side, above "
                             f"the separable kernels' {MAX_RADIUS}; the FFT operator (FluidMetric, or a Gaussian "
                             "multiplier on torch.fft) is the tool for that width")
    return radii, [gaussian_taps(s, truncate) for s in sig]


class GaussianSmoothFunction(torch.autograd.Function):
    """alpha * G x.  G is self-adjoint in both border modes (symmetric taps, symmetric border rule), so the backward
    is the same operator on the gradient -- a call of the public function, which keeps double backward working."""

    @staticmethod
    def forward(ctx, x, sigma, truncate, mode, alpha):
        ctx.args = (sigma, truncate, mode, alpha)
        radii, taps = _plan(x, sigma, truncate, mode)
        return lagomorph_ext.gaussian_smooth_forward(x, radii, taps, mode, alpha=alpha)

    @staticmethod
    def backward(ctx, gradout):
        sigma, truncate, mode, alpha = ctx.args
        return gaussian_smooth(gradout, sigma, truncate=truncate, mode=mode, alpha=alpha), None, None, None, None


def gaussian_smooth(x, sigma, truncate=4.0, mode="wrap", alpha=1.0):
    """Gaussian filtering of x (N, C, *sp), len(sp) in {2, 3}, float32 or float64, on the GPU: out = G_z G_y G_x x, each
    factor a 1-D correlation with `gaussian_taps(sigma_axis, truncate)` along one spatial axis (taps computed in
    float64 and rounded once to x's dtype).

    sigma: a number or one per spatial axis, in voxels; sigma <= 0 (or a radius int(truncate * sigma + 0.5) of 0)
    leaves that axis alone.  A radius above 32 raises ValueError: use the FFT operator for such widths.
    mode "wrap": periodic, indices modulo the extent however large the radius is (the fluid metric's domain);
    mode "zero": samples outside the grid are 0.
    alpha (beyond scipy's signature): a factor on the result, applied in the last kernel.

    Non-finite values: an inf or NaN spreads along a filtered axis a little beyond the radius (up to the radius rounded
    up to 4, plus 3: the kernels multiply by their zero padding taps); with every sigma 0 the copy is exact, inf, NaN and
    -0 included.

    Non-contiguous input is made contiguous; the result is always a new tensor.  Deterministic (no atomics), and
    differentiable to any order (the operator is its own adjoint)."""
    lagomorph_ext._check_tensors((("x", x),))
    _plan(x, sigma, truncate, mode)   # argument errors before autograd records anything
    return GaussianSmoothFunction.apply(x, sigma, float(truncate), mode, float(alpha))
