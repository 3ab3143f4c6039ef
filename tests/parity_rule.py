"""The project's acceptance rule, once (numpy only, so that the numpy-only reference modules can use it):

    max|got - ref| <= RTOL * max|ref|,   RTOL 1e-5 (float32), 1e-12 (float64), no multipliers.

`units` measures an error in units of that bound, `close` judges it (raising, or appending to a list of failures),
`bits` is the bit-for-bit comparison.  tests/gpu_util.py wraps them for device tensors; profiles/test_helpers.md lists
the copies this module replaced and the rules that are deliberately not this one."""
import numpy as np

RTOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
FLOOR = 1e-300   # stands in for a scale below it (a reference that is all zeros); 0 = "RTOL * max|ref| exactly"


def rtol(dtype):
    """RTOL of a torch dtype (recognised by its name: torch is not imported), a numpy type, an np.dtype or a dtype name."""
    name = str(dtype)
    return RTOL[np.dtype(name[len("torch."):] if name.startswith("torch.") else dtype)]


def units(got, want, dtype, scale=None, floor=FLOOR):
    """max|got - want| in units of rtol(dtype) * max(scale, floor), scale = max|want| unless given.  Accepted when
    `units <= 1`; a NaN in the difference gives NaN, so judge with `not units <= 1`.  With floor=0 and a zero scale the
    bound is 0: no error is 0 units, any other is inf."""
    got, want = np.asarray(got).astype(np.float64), np.asarray(want).astype(np.float64)
    assert got.shape == want.shape, f"shape {got.shape} vs {want.shape}"
    if scale is None:
        scale = np.abs(want).max() if want.size else 0.0
    scale = float(scale)   # (a float32 scalar would make the bound, and the quotient, float32)
    with np.errstate(invalid="ignore"):   # (inf - inf is NaN, and fails)
        err = float(np.abs(got - want).max()) if got.size else 0.0
    tol = rtol(dtype) * max(scale, floor)
    if tol == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / tol


def _fail(fails, message):
    if fails is None:
        raise AssertionError(message)
    fails.append(message)


def close(got, want, dtype, what, scale=None, floor=FLOOR, fails=None, worst=None):
    """The rule on numpy arrays; returns the units.  A failure (a shape mismatch included) raises AssertionError, or is
    appended to the list `fails` when one is given.  `worst`: a dict that keeps the largest units seen per `what`."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return _fail(fails, f"{what}: shape {got.shape} vs {want.shape}")
    u = units(got, want, dtype, scale, floor)
    if worst is not None:
        worst[what] = max(worst.get(what, 0.0), u)
    if not u <= 1.0:
        with np.errstate(invalid="ignore"):   # (inf - inf)
            d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        at = tuple(int(i) for i in np.unravel_index(int(np.argmax(np.where(np.isnan(d), np.inf, d))), d.shape))
        ref = float(np.abs(want).max()) if scale is None else scale
        _fail(fails, f"{what}: max error {float(d.max()):.3e} = {u:.3g} x {rtol(dtype):.0e} x scale {ref:.3e} at {at}")
    return u


def bits(got, want, what, check_dtype=True, fails=None):
    """Bit-identical arrays of one shape (and one dtype); reports the first differing index."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or (check_dtype and got.dtype != want.dtype):
        return _fail(fails, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}")
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        at = tuple(int(i) for i in bad[0])
        _fail(fails, f"{what}: not bit-identical in {len(bad)} of {got.size} entries, first at {at}: {got[at]!r} vs {want[at]!r}")
