"""What the GPU tests share: the dtype and shape lists, seeded inputs, device <-> host copies and the two assertions
(bit for bit, and the project's rule of tests/parity_rule.py) on device tensors.  Fixtures stay in their modules."""
import re

import numpy as np
import torch

import parity_rule

DTYPES = [torch.float32, torch.float64]
NPDT = {torch.float32: np.float32, torch.float64: np.float64}
SHAPES3 = [(5, 6, 7), (8, 8, 8), (3, 4, 1), (2, 2, 2), (9, 5, 70), (6, 5, 16), (3, 4, 128)]
SHAPES2 = [(7, 9), (16, 16), (2, 2), (5, 1), (3, 130)]

OBSERVED = {}  # what -> largest observed error in units of RTOL * scale (LAGO_TOL_REPORT; tools/tolerance_report.py prints it)


def rnd(rng, shape, dtype, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(NPDT[dtype])


def dev(a, dtype=None):
    """A fresh C-ordered copy on the device (the shared reference arrays are read-only), converted to `dtype` if given."""
    t = torch.from_numpy(np.array(a, order="C"))
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _np(x):
    return host(x) if isinstance(x, torch.Tensor) else np.asarray(x)


def assert_bits(got, want, what, check_dtype=True):
    parity_rule.bits(_np(got), _np(want), what, check_dtype)


def units_of(got, want, dtype, scale=None, floor=parity_rule.FLOOR):
    """parity_rule.units of a device tensor against a numpy reference."""
    return parity_rule.units(_np(got), want, dtype, scale, floor)


def assert_close(got, want, dtype, what, scale=None, floor=parity_rule.FLOOR, record=True, show=False):
    """|got - want| <= RTOL[dtype] * scale, scale = max |want| unless given: parity_rule.close.  The units go into
    OBSERVED under `what` cut at its first bracket (record=False: not); show=True prints them."""
    fails, worst = [], {}
    units = parity_rule.close(_np(got), want, dtype, what, scale, floor, fails, worst)
    if worst and record:
        key = re.sub(r"[\(\[].*$", "", what).strip() + (" f32" if parity_rule.rtol(dtype) == 1e-5 else " f64")
        OBSERVED[key] = max(OBSERVED.get(key, 0.0), units)
    if worst and show:
        print(f"{what}: {units:.4f} of {parity_rule.rtol(dtype):.0e} x max|ref|")
    assert not fails, fails[0]
    return units


def displacement(rng, nn, sp, dtype):
    """Displacements that exercise clamp (far out of range), the negative floor rule, and
    exact-integer positions."""
    u = rnd(rng, (nn, len(sp)) + sp, dtype, 1.7)
    flat = u.reshape(-1)
    flat[::11] *= 9.0          # far outside
    flat[::7] = np.round(flat[::7])  # exact integers (weights exactly 0/1)
    flat[::13] = -np.abs(flat[::13]) - 0.25
    return u


def smooth_field(shape, sigma, seed, amp, device="cuda"):
    """Seeded normal noise blurred by bench.gaussian_blur and scaled to the amplitude `amp`."""
    import bench

    g = torch.Generator(device=device).manual_seed(seed)
    x = bench.gaussian_blur(torch.randn(shape, device=device, generator=g), sigma)
    return (x * (amp / x.abs().max())).contiguous()
