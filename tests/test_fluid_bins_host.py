"""CPU: the bin-by-bin judge of the fluid metric (tests/fluid_bins.py) is right, would fail a subtly wrong kernel, and
its reference stays within its own conditions on the inputs of tests/test_gpu_fluid_bins.py.

The planted errors are the mistakes the FFT passes can make -- one bin of the Nyquist plane, the whole Nyquist plane (the
column kept in its own buffer), one kx row of one component (a twiddle of one stage), two ky rows with each other's
coefficients (a permuted coefficient table), the y and z LUTs exchanged -- planted into the spectrum of the float32
pocketfft pipeline before its inverse transform, the pipeline otherwise untouched.  The suite's older criterion,
max |out - ref| / max |ref| <= 2e-6 on white input, accepts the single bin and the kx row: that is the gap the bin rule
closes.

Only the well-conditioned cases claim rejection: `flat` at either parameter set and `sharp` at gamma = 1.  `sharp` at
(0.1, 0.05, 0.01) is not among them: its symbol spans four decades, which float32 cannot hold per bin, and the CLEAN
reference already reaches about 59 units in its worst bin there (56 at 64^3, 67 at 64 x 80 x 96), so a margin over it
says little about an error of a few hundred units.
"""
import numpy as np
import pytest
import scipy.fft

import fluid_bins as fb
from oracle import lago_oracle as orc

WELL = [(fb.PARAMS_WELL, False), (fb.PARAMS_WELL, True), (fb.PARAMS_USUAL, False)]
WELL_IDS = ["flat-gamma1", "sharp-gamma1", "flat-usual"]


# ---------------------------------------------------------------------------------------------------- the helper is right


@pytest.mark.parametrize("inverse", [False, True], ids=["flat", "sharp"])
@pytest.mark.parametrize("params", [(0.1, 0.05, 0.01), (1.0, 0.0, 0.01), (0.1, 0.05, 1.0)])
@pytest.mark.parametrize("sp", [(6, 5, 8), (7, 5, 9), (8, 6), (9, 7)])
def test_symbol_is_the_oracles_float64_operator(sp, params, inverse):
    """`symbol`, written from the mathematics, applied to a random complex spectrum against the oracle's float64
    `fluid_operator` (the reference kernel's Cholesky solve) on the same spectrum: 1e-12 of the bin's magnitude.  No
    gamma = 0 case: there the clamp of the reference's safe square root, not the mathematics, defines the result."""
    rng = np.random.default_rng(sum(sp))
    csh = (2, len(sp)) + tuple(sp[:-1]) + (sp[-1] // 2 + 1,)
    F = rng.standard_normal(csh) + 1j * rng.standard_normal(csh)
    want = fb.reference_operator(F, sp, params, inverse)
    assert want.dtype == np.complex128
    got = fb.apply_symbol(fb.symbol(sp, params, inverse), F)
    mag = np.sqrt((np.abs(want) ** 2).sum(1, keepdims=True))   # the bin's magnitude over its components
    assert (np.abs(got - want) <= 1e-12 * mag).all(), float((np.abs(got - want) / mag).max())
    K, norm = fb.symbol_pair(sp, params)[inverse]
    np.testing.assert_array_equal(K, fb.symbol(sp, params, inverse))
    np.testing.assert_allclose(norm, np.linalg.norm(K, 2, axis=(-2, -1)), rtol=1e-6)   # (a norm in a denominator: closed form, below)


def test_closed_form_eigenvalue_range_is_lapacks():
    """Random symmetric matrices, multiples of the identity and pairs of equal eigenvalues (where the cubic's
    discriminant vanishes: the arc cosine there costs half the digits, 1e-8 of the norm), and l itself on a non-cubic
    grid."""
    rng = np.random.default_rng(5)
    for d in (2, 3):
        a = rng.standard_normal((500, d, d))
        a = a + np.swapaxes(a, -1, -2)
        a[:20] = np.eye(d) * rng.standard_normal((20, 1, 1))
        a[20:40] = np.eye(d) + np.eye(d)[0][:, None] * np.eye(d)[0][None, :] * rng.standard_normal((20, 1, 1))
        lo, hi = fb.sym_eigenvalue_range(a)
        ev = np.linalg.eigvalsh(a)
        scale = np.abs(ev).max(-1)
        assert (np.abs(lo - ev[..., 0]) <= 1e-7 * scale).all() and (np.abs(hi - ev[..., -1]) <= 1e-7 * scale).all()
    for sp in [(12, 10, 14), (16, 12)]:
        l = fb._little_l(sp, fb.PARAMS_USUAL)
        lo, hi = fb.sym_eigenvalue_range(l)
        ev = np.linalg.eigvalsh(l)
        np.testing.assert_allclose(lo, ev[..., 0], rtol=1e-6)
        np.testing.assert_allclose(hi, ev[..., -1], rtol=1e-6)


def test_luts_are_the_metrics():
    """w and s as `metric.fluid_luts` and the oracle build them: rounded through float32."""
    for sp in [(6, 5, 8), (9, 7), (64, 80, 96)]:
        w, s = fb.luts(sp)
        cos, sin = orc.fluid_luts(sp, np.float64)
        for a, b in zip(w + s, cos + sin):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, a.astype(np.float32).astype(np.float64))


def test_units_of_the_exact_answer_are_zero_and_scale_free():
    """The float64 pipeline itself sits at rounding level of float64 (1e-8 of a float32 unit), and the units do not
    depend on the input's scale."""
    sp = (12, 10, 14)
    m = fb.white_input(sp, 2, np.float64, 3)
    for inverse in (False, True):
        exact = scipy.fft.irfftn(fb.expected_spectrum(m, fb.PARAMS_WELL, inverse), s=sp, axes=(2, 3, 4), norm="ortho")
        assert fb.units(exact, m, fb.PARAMS_WELL, inverse, fb.EPS32).max() < 1e-6
        ref = fb.reference(m.astype(np.float32), fb.PARAMS_WELL, inverse)
        u1 = fb.units(ref, m.astype(np.float32), fb.PARAMS_WELL, inverse, fb.EPS32)
        u2 = fb.units(ref * np.float32(1024), m.astype(np.float32) * np.float32(1024), fb.PARAMS_WELL, inverse, fb.EPS32)
        np.testing.assert_allclose(u1, u2, rtol=1e-9)


# ---------------------------------------------------------------------------------------------------- the lists


@pytest.mark.parametrize("name", sorted(fb.MACRO_LISTS))
def test_macro_list_copies_match_the_sources(name):
    """The instantiation lists are read from the sources as text: a new length, plane or 2D shape fails here until
    tests/fluid_bins.py has it, and then tests/test_gpu_fluid_bins.py has its bin-by-bin case."""
    fname, copy = fb.MACRO_LISTS[name]
    assert fb.macro_list(fb.source_text(fname), name) == copy


def test_every_instantiation_has_a_case():
    lds = [c[1] for c in fb.white_cases() if c[4] == "fluid_lds"]
    assert len(fb.x_length_cases()) == len(fb.X_SIZES) and {sp[0] for sp in fb.x_length_cases()} == set(fb.X_SIZES)
    assert {sp[1:] for sp in fb.plane_cases()} == set(fb.ZY_SHAPES) and len(fb.plane_cases()) == len(fb.ZY_SHAPES)
    big = fb.big_plane_cases()
    assert sorted(sp[1] for sp in big) == sorted(fb.BIG_Y_SIZES) and sorted(sp[2] for sp in big) == sorted(fb.BIG_Z_SIZES)
    assert not any(sp[1:] in fb.ZY_SHAPES for sp in big)
    for sp in lds + list(fb.VARIANT_SHAPES):
        assert sp[0] in fb.X_SIZES
        assert sp[1:] in fb.ZY_SHAPES or (sp[1] in fb.BIG_Y_SIZES and sp[2] in fb.BIG_Z_SIZES)
        assert sp[1] % 16 == 0 or sp[0] % 16 != 0   # a half tile at the end of the Nyquist plane needs a masking x length
    assert {c[1] for c in fb.white_cases() if c[4] == "fluid_2d"} == set(fb.SHAPES_2D)
    assert not any(c[1] in fb.SHAPES_2D for c in fb.white_cases() if c[4] == "fluid_generic")
    ids = [c[0] for c in fb.white_cases()]
    assert len(set(ids)) == len(ids)
    assert max(int(np.prod(c[1])) for c in fb.white_cases()) <= 64 * 240 * 160   # (the largest one-kernel plane at nx = 64)


# ---------------------------------------------------------------------------------------------------- planted errors


class Planted:
    """The float32 pipeline on one white input, with hooks between its stages."""

    def __init__(self, sp):
        self.sp = sp
        self.m = fb.white_input(sp, 2, np.float32, fb.case_seed(sp))
        self.Mhat = fb.spectrum(self.m)
        self.F0 = fb.reference_forward(self.m)
        assert self.F0.dtype == np.complex64
        self._combo = {}

    def combo(self, params, inverse):
        key = (params, inverse)
        if key not in self._combo:
            J = fb.Judge(self.m, params, inverse, fb.EPS32, self.Mhat)
            F = fb.reference_operator(self.F0, self.sp, params, inverse)
            clean = fb.reference_inverse(F, self.sp)
            exact = scipy.fft.irfftn(J.What, s=self.sp, axes=(2, 3, 4), norm="ortho")   # the old criterion's `ref`
            self._combo[key] = (J, F, J.figures(clean), exact)
        return self._combo[key]


@pytest.fixture(scope="module", params=[(64, 64, 64), (64, 80, 96)], ids=["64x64x64", "64x80x96"])
def planted(request):
    return Planted(request.param)


def old_criterion(out, exact):
    return float(np.abs(out.astype(np.float64) - exact).max() / np.abs(exact).max())


def plant(P, params, inverse, what):
    """The clean spectrum after the operator, with one error planted; Hermitian partners move together."""
    J, F, ref_fig, exact = P.combo(params, inverse)
    nx, ny, nz = P.sp
    G = F.copy()
    if what == "one Nyquist-plane bin x 1.001":
        G[1, 2, 5, 7, nz // 2] *= np.float32(1.001)
        G[1, 2, -5, -7, nz // 2] *= np.float32(1.001)   # (its mirror image: the same bin of a real field)
    elif what == "kz = nz/2 plane x 1.0001":
        G[..., nz // 2] *= np.float32(1.0001)
    elif what == "one kx row of one component x 1.00002":
        # the row that holds the least of the output's energy, where the global norm is blindest: flat grows with the
        # frequency (kx = 1), sharp falls with it (kx = nx / 2)
        G[:, 1, nx // 2 if inverse else 1] *= np.float32(1.00002)
    elif what == "two ky rows with each other's coefficients":
        K = fb.symbol(P.sp, params, inverse)
        for a, b in ((9, 10), (10, 9)):
            G[:, :, :, a, :] = fb.apply_symbol(K[:, b], P.F0[:, :, :, a, :].astype(np.complex128)).astype(np.complex64)
    elif what == "y and z LUTs exchanged":
        G = fb.reference_operator(P.F0, P.sp, params, inverse, periods=(nx, nz, ny))
    else:
        raise KeyError(what)
    return fb.reference_inverse(G, P.sp)


PLANTS = ["one Nyquist-plane bin x 1.001", "kz = nz/2 plane x 1.0001", "one kx row of one component x 1.00002",
          "two ky rows with each other's coefficients", "y and z LUTs exchanged"]


@pytest.mark.parametrize("params,inverse", WELL, ids=WELL_IDS)
def test_the_bin_rule_rejects_every_planted_error(planted, params, inverse):
    J, F, ref_fig, exact = planted.combo(params, inverse)
    assert fb.reference_guard(ref_fig, np.float32, planted.Mhat.size) and planted.Mhat.size <= fb.GUARD_BINS, ref_fig
    ok, rmax, rp = fb.verdict(ref_fig, ref_fig)
    assert ok and rmax == 1.0   # (the clean pipeline passes its own rule)
    for what in PLANTS:
        if what == "y and z LUTs exchanged" and planted.sp[1] == planted.sp[2]:
            continue   # (on the cube the two LUTs are the same)
        out = plant(planted, params, inverse, what)
        fig = J.figures(out)
        ok, rmax, rp = fb.verdict(fig, ref_fig)
        print(f"{planted.sp} {params} {'sharp' if inverse else 'flat'} {what}: {fig['max']:.0f} units, "
              f"{rmax:.0f} x the reference (p99.9 {rp:.1f} x), old criterion {old_criterion(out, exact):.2e}")
        assert not ok, fb.describe(what, fig, ref_fig)
        # well clear of the margin, not just over it: the weakest planted error was measured at 25 x the reference
        assert rmax >= 4 * fb.MARGIN, (what, rmax)


@pytest.mark.parametrize("params,inverse", [(fb.PARAMS_WELL, True), (fb.PARAMS_USUAL, False)], ids=["sharp-gamma1", "flat-usual"])
def test_the_global_norm_accepts_the_single_bin_and_the_kx_row(planted, params, inverse):
    """The gap being closed: max |out - ref| / max |ref| <= 2e-6, the criterion of every older FFT test, passes two of
    the errors that the bin rule rejects at 25 to 1200 x the reference (measured: 4e-7 to 1.3e-6 for the bin, 1.1e-6
    to 1.5e-6 for the row)."""
    J, F, ref_fig, exact = planted.combo(params, inverse)
    assert old_criterion(fb.reference_inverse(F, planted.sp), exact) <= 2e-6
    for what in ("one Nyquist-plane bin x 1.001", "one kx row of one component x 1.00002"):
        out = plant(planted, params, inverse, what)
        assert old_criterion(out, exact) <= 2e-6, what
        assert not fb.verdict(J.figures(out), ref_fig)[0], what


@pytest.mark.parametrize("inverse", [False, True], ids=["flat", "sharp"])
@pytest.mark.parametrize("sp", [(64, 64, 64), (24, 20, 28), (64, 96)])
def test_two_bin_input_resolves_its_two_bins(sp, inverse):
    """m = a + b (-1)^(x + y + z): with the coherent noise level (fluid_bins.Judge) the clean pipeline stays within a
    unit or two in every bin (0.2 to 1.8 measured), so the rule with its floor of one unit amounts to 4 units; the DC bins
    or the Nyquist-corner bins off by 1e-4 are rejected.  (The white-noise level would not do here: it puts the final
    rounding of the two-valued output, which lands whole in the two bins, at hundreds of units.)"""
    m = fb.two_bin_input(sp, 2, np.float32, fb.case_seed(sp))
    J = fb.Judge(m, fb.PARAMS_WELL, inverse, fb.EPS32, coherent=True)
    F = fb.reference_operator(fb.reference_forward(m), sp, fb.PARAMS_WELL, inverse)
    ref = J.figures(fb.reference_inverse(F, sp))
    assert ref["max"] <= fb.MARGIN, ref
    for where in ((0,) * len(sp), tuple(n // 2 for n in sp)):
        G = F.copy()
        G[(slice(None), slice(None)) + where] *= np.float32(1.0001)
        fig = J.figures(fb.reference_inverse(G, sp))
        assert not fb.verdict(fig, ref, floor=1.0)[0], (where, fig)
        assert fig["worst"][2:] == where


# ---------------------------------------------------------------------------------------------------- the reference's own conditions

SMALL = [c for c in fb.white_cases() if int(np.prod(c[1])) <= 64 * 64 * 64 and c[3] == 3]


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_reference_stays_within_its_own_conditions(case):
    """On the inputs of the GPU cases (those of at most 64^3 points; the GPU module asserts the same for all of them at
    run time): the reference pipeline's own units on the well-conditioned cases, max <= 8 and p99.9 <= 5 (measured 5.3
    to 6.7 and 3.5 to 3.9 at 64^3 and 64 x 80 x 96).  This guards the denominator of the GPU rule against a degenerate
    input; it is not a tolerance for a kernel.  float64 cases: the same pipeline in double, eps = 2^-53
    (fluid_bins.reference_guard)."""
    _, sp, dt, _, _ = case
    m = fb.white_input(sp, 2, np.dtype(dt), fb.case_seed(sp))
    eps = fb.EPS32 if dt == "float32" else fb.EPS64
    Mhat = fb.spectrum(m)
    for params in (fb.PARAMS_WELL, fb.PARAMS_USUAL):
        pair = fb.symbol_pair(sp, params)
        for inverse in (False, True):
            if not fb.well_conditioned(params, inverse):
                continue
            fig = fb.Judge(m, params, inverse, eps, Mhat, pair).figures(fb.reference(m, params, inverse))
            assert fb.reference_guard(fig, dt, Mhat.size), (sp, dt, params, inverse, fig)
