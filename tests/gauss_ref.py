"""Test-side float64 reference of gaussian_smooth (numpy only; nothing of the product is imported).

Per spatial axis the output is sum_k w_k * (the array shifted by k along that axis): np.roll for the periodic border,
zero-filled slices for the zero border.  Taps by this module's own formula.  tests/test_gauss_host.py holds it against
scipy.ndimage.gaussian_filter and against a torch conv1d restatement."""
import numbers

import numpy as np

MAX_RADIUS = 32


def radius(sigma, truncate=4.0):
    return int(truncate * sigma + 0.5) if sigma > 0 else 0


def taps(sigma, truncate=4.0):
    """float64 taps w_{-r..r}, normalised; [1.] when the radius is 0."""
    r = radius(float(sigma), float(truncate))
    if r == 0:
        return np.ones(1)
    k = np.arange(-r, r + 1).astype(np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    return w / w.sum()


def per_axis(sigma, dim):
    if isinstance(sigma, numbers.Real):
        return [float(sigma)] * dim
    assert len(sigma) == dim
    return [float(s) for s in sigma]


def shifted(x, k, axis, mode):
    """y[i] = x[i + k] along `axis`: modulo the extent (wrap) or 0 outside (zero)."""
    if mode == "wrap":
        return np.roll(x, -k, axis=axis)
    assert mode == "zero"
    n = x.shape[axis]
    y = np.zeros_like(x)
    if abs(k) >= n:
        return y
    src = [slice(None)] * x.ndim
    dst = [slice(None)] * x.ndim
    if k >= 0:
        src[axis], dst[axis] = slice(k, n), slice(0, n - k)
    else:
        src[axis], dst[axis] = slice(0, n + k), slice(-k, n)
    y[tuple(dst)] = x[tuple(src)]
    return y


def correlate_axis(x, w, axis, mode):
    r = (len(w) - 1) // 2
    out = np.zeros_like(x)
    for k in range(-r, r + 1):
        out += w[k + r] * shifted(x, k, axis, mode)
    return out


def smooth_taps(x, tap_list, mode="wrap"):
    """G x in float64 for x of shape (N, C, *sp) and one tap vector per spatial axis."""
    y = np.asarray(x, dtype=np.float64)
    dim = y.ndim - 2
    assert len(tap_list) == dim
    for a in range(dim):
        if len(tap_list[a]) > 1:
            y = correlate_axis(y, np.asarray(tap_list[a], dtype=np.float64), 2 + a, mode)
    return y.copy() if y is x else y


def smooth(x, sigma, truncate=4.0, mode="wrap"):
    dim = np.ndim(x) - 2
    return smooth_taps(x, [taps(s, truncate) for s in per_axis(sigma, dim)], mode)


def rounded_taps(sigma, truncate, dtype):
    """The taps as the device holds them: rounded once to `dtype`."""
    return taps(sigma, truncate).astype(dtype).astype(np.float64)
