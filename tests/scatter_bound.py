"""The cell-wise bound for scatter-add outputs, judged against the oracle's wide sums (oracle/lago_oracle.py:
*_wide -> sum, sabs, count per cell).

The bound.  For cell i with n = count_i contributions, A = sabs_i = sum of |contribution| and u the unit roundoff of
the output type (2^-24 for float32, 2^-53 for float64):

    k       = n + 3
    bound_i = k u / (1 - k u) * A  +  n * tiny            tiny = smallest normal number of the type

Derivation.  The wide sum S_i = sum_j t_j takes every contribution t_j = w_x w_y [w_z] m as the exact product of the
float weights and the float mass that the reference forms (same positions, floor, sequential weight flips and clamp:
the oracle's plain and wide forms share one body), summed in a type with 29 (float32) or 11 (float64) more bits.
A float implementation reaches the cell through a chain of rounded operations; every t_j picks up one factor
(1 + d), |d| <= u, per rounding on its path:

  * at most 3 when it is formed: two weight products and the product with the mass (2D: two).  The hessian diagonal
    forms w = w_a w_b and then w w: two roundings, the first one counted twice -- three factors;
  * at most n - 1 rounded additions on its way into the cell, in ANY order and through any mix of partial sums held in
    registers, LDS or float64, one narrowing to the output type, hardware atomics: the first addition onto the zeroed
    cell is exact, and a tree, a sequential loop or an unordered sequence of atomics all give every term at most n - 1;
  * one more for the yardstick's own final rounding to double.

So the computed value is sum_j t_j prod_{r <= k} (1 + d_jr) with k = n + 3, and by the standard lemma (Higham,
Accuracy and Stability of Numerical Algorithms, Lemma 3.1) |computed - S_i| <= gamma_k A with gamma_k =
k u / (1 - k u).  The n * tiny term covers additions whose subnormal results an atomic unit flushes to zero (each
loses less than tiny).  The separable regrid form multiplies by one weight per pass and adds n_x, n_y, n_z terms in
the three passes: n_x + n_y + n_z <= n_x n_y n_z + 2 = n + 2 roundings on a path, within the same k.  A form that adds
onto a start value (interp_backward_fused(..., d_I=start)) has one more term: n + 1 and A + |start_i|.

The bound holds for the reference's own float result and for any correct kernel, whatever its summation order; there is
no tolerance in it and no multiplier.  A cell that receives nothing (count 0) must hold exactly zero, or exactly its
start value.  Every cell of every output is judged.

gamma_k needs k u < 1.  A float32 cell that collects 2^24 contributions or more -- a clamped face cell of the
large-matrix affine cases (tests/affine_box_cases.py), where most of 8 million samples leave the grid -- is judged by the
product form of the same lemma, which holds for every k: |prod_{r <= k} (1 + d_r) - 1| <= (1 + u)^k - 1, so

    bound_i = ((1 + u)^k - 1) * A  +  n * tiny            where k u >= 1

(at most gamma_k wherever both exist).  Weak -- about 1.7 A at k u = 1 -- but finite: no cell is exempt, and a value that
is not finite is over any bound.
"""
import numpy as np

UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def cell_bound(sabs, count, dtype, start=None):
    """bound_i of the module docstring, float64 array of the cells' shape."""
    dtype = np.dtype(dtype)
    u, tiny = UNIT[dtype], float(np.finfo(dtype).tiny)
    n = np.asarray(count, dtype=np.float64)
    A = np.asarray(sabs, dtype=np.float64)
    if start is not None:
        n = n + 1.0
        A = A + np.abs(np.asarray(start, dtype=np.float64))
    k = n + 3.0
    ku = k * u
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        factor = np.where(ku < 1.0, ku / (1.0 - ku), np.expm1(k * np.log1p(u)))
    return factor * A + n * tiny


def cell_errors(got, wide, dtype, start=None):
    """(err, bound) per cell: |got - (sum [+ start])| and bound_i.  float64 results are differenced in long double, so
    that the comparison itself adds nothing of the order of the bound."""
    dtype = np.dtype(dtype)
    s, sabs, count = wide
    got = np.asarray(got)
    assert got.shape == s.shape, f"shape {got.shape} vs {s.shape}"
    work = np.longdouble if dtype == np.float64 else np.float64
    d = got.astype(work) - s.astype(work)
    if start is not None:
        d = d - np.asarray(start).astype(work)
    return np.abs(d).astype(np.float64), cell_bound(sabs, count, dtype, start)


def violations(got, wide, dtype, start=None):
    """Boolean array: cells over their bound (an empty cell: anything but exactly zero / its start value)."""
    err, bound = cell_errors(got, wide, dtype, start)
    bad = ~(err <= bound)          # (a NaN compares False: it is over the bound)
    empty = np.asarray(wide[2]) == 0
    if empty.any():
        want = 0.0 if start is None else np.asarray(start)
        bad |= empty & (np.asarray(got) != want)
    return bad


def worst_ratio(got, wide, dtype, start=None):
    """max err_i / bound_i (0 where err is 0; inf for a wrong value in a cell of bound 0; NaN as soon as one cell holds a
    NaN)."""
    err, bound = cell_errors(got, wide, dtype, start)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def assert_cells(got, wide, dtype, what, start=None, ref=None):
    """Every cell within its bound; returns the worst err / bound.  On failure the message names the worst cell with
    its count, sabs, the judged value, the wide sum and (when `ref` is given) the float oracle's value there."""
    bad = violations(got, wide, dtype, start)
    ratio = worst_ratio(got, wide, dtype, start)
    if bad.any():
        err, bound = cell_errors(got, wide, dtype, start)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bad, np.where(bound > 0, err / bound, np.inf), 0.0)   # (argmax takes a NaN first)
        at = np.unravel_index(int(r.argmax()), r.shape)
        s, sabs, count = wide
        msg = (f"{what}: {int(bad.sum())} of {bad.size} cells over the bound; worst at {tuple(int(a) for a in at)}: "
               f"err {err[at]:.6e} = {r[at]:.3f} x bound {bound[at]:.6e}; count {count[at]:.0f}, sabs {sabs[at]:.9e}, "
               f"got {float(np.asarray(got)[at])!r}, wide {float(s[at])!r}")
        if start is not None:
            msg += f", start {float(np.asarray(start)[at])!r}"
        if ref is not None:
            msg += f", oracle {float(np.asarray(ref)[at])!r}"
        raise AssertionError(msg)
    return ratio

