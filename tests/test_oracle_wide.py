"""CPU: the wide scatter sums of the oracle (oracle_*_wide: sum, sabs, count per cell) and the cell-wise bound of
tests/scatter_bound.py built on them.

  * the plain oracle (float32 and float64) lies within bound_i of the wide sum at every cell, for the four scatter
    operators -- a theorem, so a failure means the wide code's terms are not the oracle's: this pins the yardstick to the
    already pinned oracle;
  * the wide sum does not depend on the summation order beyond count * 2^-53 * sabs;
  * three seeded defects that the max-norm criterion of tests/test_gpu_parity.py accepts are rejected by the bound;
  * the float64 oracle on upcast float32 inputs is NOT a yardstick: the float32 oracle itself is far outside the bound
    around it (positions rounded in float64 are other positions).
"""
import numpy as np
import pytest

import affine_box_cases as abc
import parity_rule
import scatter_cases as sc
from oracle import lago_oracle as orc
from scatter_bound import assert_cells, cell_bound, violations, worst_ratio

SHAPES3 = [(5, 6, 7), (8, 8, 8), (3, 4, 1), (2, 2, 2), (9, 5, 70), (6, 5, 16), (3, 4, 128)]   # gpu_util.SHAPES3
SHAPES2 = [(7, 9), (16, 16), (2, 2), (5, 1), (3, 130)]                                          # gpu_util.SHAPES2  
NPDT = [np.float32, np.float64]


def test_shape_lists_are_those_of_the_parity_suite():
    """The shape lists above are copies (importing tests/gpu_util.py would pull torch into this module)."""
    import ast
    import os

    tree = ast.parse(open(os.path.join(os.path.dirname(__file__), "gpu_util.py")).read())
    got = {t.id: ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign)
           for t in n.targets if isinstance(t, ast.Name) and t.id in ("SHAPES3", "SHAPES2")}
    assert got == {"SHAPES3": SHAPES3, "SHAPES2": SHAPES2}


# ---------------------------------------------------------------- the reference within the bound


@pytest.mark.parametrize("npdt", NPDT)
@pytest.mark.parametrize("sp", SHAPES3 + SHAPES2 + sc.LDS2D_SHAPES + [(64, 64, 64)])
@pytest.mark.parametrize("nn,nc,bc", [(2, 1, False), (3, 3, True), (2, 3, False), (3, 1, True)])
def test_interp_backward_oracle_within_bound(npdt, sp, nn, nc, bc):
    go, u = sc.interp_inputs(sp, nn, nc, npdt)
    I = np.zeros(((1 if bc else nn), nc) + sp, npdt)
    for dt in (1.0, -1.0, 0.8):
        oI, _ = orc.interp_backward(go, I, u, dt, True, False)
        wide = orc.interp_backward_wide(go, u, dt, broadcast_I=bc)
        # every sample deposits 2^dim contributions, none is lost to the clamp
        assert wide[2].sum() == go.size * 2 ** len(sp)
        r = assert_cells(oI, wide, npdt, f"interp_backward oracle {sp} dt={dt} bc={bc} nc={nc}")
        assert r <= 1.0


@pytest.mark.parametrize("npdt", NPDT)
@pytest.mark.parametrize("sp", [(128, 128), (40, 36, 96)])
def test_interp_backward_oracle_within_bound_smooth(npdt, sp):
    go, u = sc.interp_inputs(sp, 2, 2, npdt, kind="smooth")
    I = np.zeros((2, 2) + sp, npdt)
    for dt in (1.0, -1.0, 0.8):
        oI, _ = orc.interp_backward(go, I, u, dt, True, False)
        assert_cells(oI, orc.interp_backward_wide(go, u, dt), npdt, f"interp_backward oracle smooth {sp} dt={dt}")


@pytest.mark.parametrize("npdt", NPDT)
@pytest.mark.parametrize("kind", sc.AFFINE_KINDS)
@pytest.mark.parametrize("bc", [False, True])
def test_affine_backward_oracle_within_bound(npdt, kind, bc):
    go, I, A, T = sc.affine_kind_inputs(kind, bc, npdt)
    oI, oA, oT = orc.affine_interp_backward(go, I, A, T, True, True, True)
    wI, wA, wT = orc.affine_interp_backward_wide(go, I, A, T)
    assert wI[2].sum() == go.size * 8
    assert_cells(oI, wI, npdt, f"affine d_I oracle {kind} bc={bc}")
    # d_A / d_T: hundreds of thousands of cancelling terms into one number; the rigorous bound holds (it is a theorem
    # for these sums as well: two products, then the sum) but says little -- the GPU test judges them by the project's
    # max-norm bound against the wide sum instead
    for got, w, what in ((oA, wA, "d_A"), (oT, wT, "d_T")):
        assert w[2].min() == w[2].max() == go[0].size
        # the product g * diff is rounded before the fma with f: one rounding per product, n - 1 (+ tree) additions
        assert_cells(got, w, npdt, f"affine {what} oracle {kind} bc={bc}")
    # the wide splat alone equals the one computed next to d_A / d_T
    only, none_A, none_T = orc.affine_interp_backward_wide(go, I, A, T, True, False, False)
    assert none_A is None and none_T is None
    assert all(np.array_equal(a, b) for a, b in zip(only, wI))


@pytest.mark.parametrize("npdt", NPDT)
@pytest.mark.parametrize("idx", range(len(abc.GPU_ADVERSARIAL)))
def test_affine_backward_oracle_within_bound_large_matrices(npdt, idx):
    name, shape, A, T, srcs, go = abc.gpu_adversarial_inputs(idx, npdt)
    I = np.zeros((2, 1) + shape, npdt)
    oI, _, _ = orc.affine_interp_backward(go, I, A, T, True, False, False)
    wI, _, _ = orc.affine_interp_backward_wide(go, I, A, T, True, False, False)
    # most samples of these maps leave the grid and pile onto a few clamped face cells; past 2^24 contributions a float32
    # cell is judged by the product form of the bound (scatter_bound docstring): weak there, but no cell is exempt
    print(f"{name}: most contributions in one cell {wI[2].max():.0f}, finite bound everywhere: "
          f"{bool(np.isfinite(cell_bound(wI[1], wI[2], npdt)).all())}")
    assert np.isfinite(cell_bound(wI[1], wI[2], npdt)).all()
    assert_cells(oI, wI, npdt, f"affine d_I oracle {name}")


@pytest.mark.parametrize("npdt", NPDT)
@pytest.mark.parametrize("sp,out,scale", sc.REGRID_CASES)
def test_regrid_backward_oracle_within_bound(npdt, sp, out, scale):
    go, origin, spacing = sc.regrid_inputs(sp, out, scale, npdt)
    want = orc.regrid_backward(go, sp, out, origin, spacing)
    wide = orc.regrid_backward_wide(go, sp, out, origin, spacing)
    assert wide[2].sum() == go.size * 2 ** len(sp)
    assert_cells(want, wide, npdt, f"regrid_backward oracle {sp} <- {out} x {scale}")


@pytest.mark.parametrize("npdt", NPDT)
@pytest.mark.parametrize("origin,spacing", sc.REGRID_SEP_ENTRY)
def test_regrid_backward_oracle_within_bound_entry_cases(npdt, origin, spacing):
    go, sp, out = sc.regrid_sep_entry_inputs(npdt)
    want = orc.regrid_backward(go, sp, out, origin, spacing)
    assert_cells(want, orc.regrid_backward_wide(go, sp, out, origin, spacing), npdt, f"regrid_backward oracle {origin} {spacing}")


@pytest.mark.parametrize("npdt", NPDT)
@pytest.mark.parametrize("sp,nn,nc", [((9, 8), 2, 3), ((7, 9), 3, 1), ((2, 2), 2, 2), ((5, 1), 1, 1), ((130, 200), 2, 3)])
def test_hessian_diagonal_oracle_within_bound(npdt, sp, nn, nc):
    I, u = sc.hessian_inputs(npdt, sp, nn, nc)
    for dt in (0.6, 1.0, -1.0):
        want = orc.interp_hessian_diagonal_image(I, u, dt)
        wide = orc.interp_hessian_diagonal_image_wide(I, u, dt)
        assert wide[2].sum() == nn * nc * sp[0] * sp[1] * 4
        assert wide[2].reshape(-1, sp[0], sp[1])[1:].sum() == 0     # everything lands in plane 0, as in the reference
        assert_cells(want, wide, npdt, f"hessian diagonal oracle {sp} dt={dt}")


# ---------------------------------------------------------------- the wide sum does not depend on the order


@pytest.mark.parametrize("npdt", NPDT)
@pytest.mark.parametrize("sp", [(9, 5, 70), (130, 200), (24, 20, 32)])
def test_wide_sum_is_order_independent(npdt, sp):
    nn, nc = 4, 2
    go, u = sc.interp_inputs(sp, nn, nc, npdt)
    perm = [2, 0, 3, 1]
    for bc in (False, True):
        base = orc.interp_backward_wide(go, u, 0.8, broadcast_I=bc)
        orc.set_threads(4)
        try:
            thr = orc.interp_backward_wide(go, u, 0.8, broadcast_I=bc)
        finally:
            orc.set_threads(1)
        per = orc.interp_backward_wide(go[perm], u[perm], 0.8, broadcast_I=bc)
        if not bc:
            per = tuple(a[np.argsort(perm)] for a in per)
        margin = base[2] * 2.0 ** -53 * base[1]
        for other in (thr, per):
            assert np.array_equal(other[2], base[2])
            assert np.all(np.abs(other[0] - base[0]) <= margin)
            assert np.all(np.abs(other[1] - base[1]) <= margin)
        if not bc:   # no plane is shared: not a bit moves
            assert all(np.array_equal(a, b) for a, b in zip(thr, base))
            assert all(np.array_equal(a, b) for a, b in zip(per, base))
        if npdt == np.float32:   # the margin is nothing next to the bound it serves
            assert np.all(margin <= 2.0 ** -20 * cell_bound(base[1], base[2], np.float32))


# ---------------------------------------------------------------- seeded defects


def _numpy_splat(go, u, defect=None, lose=None):
    """interp_backward's d_I (dt = 1, float32, no broadcast) in numpy: the reference's float32 positions, floor,
    sequentially flipped weights, clamp and products; the sum per cell in float64, rounded to float32 once (a correct
    implementation by the bound's derivation).  `defect`: 'drop' leaves out every corner of weight below 1e-6;
    'fraction' takes the upper weight of each axis as the fraction t where the reference takes 1 - (1 - t).
    `lose` = (sample index, corner): that one contribution is left out."""
    nn, nc = go.shape[:2]
    sp = go.shape[2:]
    dim = len(sp)
    one = np.float32(1)
    grids = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sp], indexing="ij")
    out = np.zeros((nn, nc) + sp, np.float32)
    nvox = int(np.prod(sp))
    for n in range(nn):
        h = [(u[n, a].astype(np.float64) + grids[a]).astype(np.float32) for a in range(dim)]   # fma(1, u, i) is u + i
        f = [np.floor(x) for x in h]
        lower = [one - (x - fl) for x, fl in zip(h, f)]
        upper = [(x - fl) if defect == "fraction" else one - lo for x, fl, lo in zip(h, f, lower)]
        f = [np.clip(fl, -2.0 ** 30, 2.0 ** 30).astype(np.int64) for fl in f]
        for c in range(nc):
            mass = go[n, c]
            acc = np.zeros(nvox, np.float64)
            for corner in range(2 ** dim):
                bits = [(corner >> (dim - 1 - a)) & 1 for a in range(dim)]
                w = None
                for a in range(dim):
                    wa = upper[a] if bits[a] else lower[a]
                    w = wa if w is None else w * wa          # float32 products, in the reference's order
                term = (w * mass).astype(np.float64)
                if defect == "drop":
                    term = np.where(w < np.float32(1e-6), 0.0, term)
                at = np.zeros(sp, np.int64)
                for a in range(dim):
                    at = at * sp[a] + np.clip(f[a] + bits[a], 0, sp[a] - 1)
                if lose is not None and lose[:3] == (n, c, corner):
                    term = term.copy()
                    term.reshape(-1)[lose[3]] = 0.0
                acc += np.bincount(at.reshape(-1), weights=term.reshape(-1), minlength=nvox)
            out[n, c] = acc.reshape(sp).astype(np.float32)
    return out


def _quiet_contribution(go, u, wide, old_bound):
    """(n, c, corner, flat sample index): a contribution of |value| about old_bound / 4 -- invisible to a max-norm check
    with that bound -- into a cell that is not a clamped border cell (few contributions)."""
    sp = go.shape[2:]
    dim = len(sp)
    one = np.float32(1)
    grids = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in sp], indexing="ij")
    n = c = 0
    h = [(u[n, a].astype(np.float64) + grids[a]).astype(np.float32) for a in range(dim)]
    f = [np.floor(x) for x in h]
    inside = np.ones(sp, bool)
    w = one
    for a in range(dim):
        inside &= (f[a] >= 1) & (f[a] <= sp[a] - 3)
        w = w * (one - (h[a] - f[a]))                      # corner 0: the product of the lower weights
    term = np.abs((w * go[n, c]).astype(np.float64))
    score = np.where(inside & (term <= 0.25 * old_bound), term, -1.0)
    q = int(score.argmax())
    assert score.reshape(-1)[q] > 0.05 * old_bound
    return (n, c, 0, q)


def _defect_inputs(sp):
    """(go, u), float32, two items.  Item 0 is the suite's wild field (clamped pile-ups: the loud cells that set the
    max-norm bound).  Item 1 is quiet -- zero displacement and zero grad_out -- except for what the two weight defects
    need in order to show deterministically rather than by the luck of a seed:
      * rows x = 2, 3 carry mass and sit 2^-21 above their integer position (representable below 4): the upper x
        corner has weight 2^-21 < 1e-6 and, for row 3, lands in a cell that receives nothing else;
      * isolated voxels of row 0 carry mass and sit at x = t in (0.001, 0.02) -- only below 1 does a float32 position
        have a fraction with bits under 2^-24, where 1 - (1 - t) and t differ: their upper x corner lands, with weight
        1 - (1 - t), in a cell of row 1 that receives nothing else of value."""
    go, u = sc.interp_inputs(sp, 2, 1, np.float32)
    rng = np.random.default_rng(5)
    go[1] = 0
    u[1] = 0
    go[1, 0, 2:4] = sc.normal(rng, (2,) + sp[1:], np.float32)
    u[1, 0, 2:4] = np.float32(2.0 ** -21)
    lone = (slice(None, None, 3),) * (len(sp) - 1)
    go[1, 0, 0][lone] = sc.normal(rng, go[1, 0, 0][lone].shape, np.float32)
    u[1, 0, 0][lone] = rng.uniform(0.001, 0.02, go[1, 0, 0][lone].shape).astype(np.float32)
    return go, u


@pytest.mark.parametrize("sp", [(9, 5, 70), (130, 200), (64, 64, 64)])
def test_seeded_defects_pass_the_max_norm_and_fail_the_bound(sp):
    """The evidence that the cell-wise check sees what the max-norm check cannot.  The defects live here, not in the
    product: a numpy splat with a switch."""
    npdt = np.float32
    go, u = _defect_inputs(sp)
    I = np.zeros((2, 1) + sp, npdt)
    oI, _ = orc.interp_backward(go, I, u, 1.0, True, False)
    wide = orc.interp_backward_wide(go, u, 1.0)
    # the control: the numpy splat without a defect is the oracle's operator -- inside the bound, and accepted before
    good = _numpy_splat(go, u)
    assert_cells(good, wide, npdt, f"numpy splat without defect {sp}")
    assert parity_rule.units(good, oI, np.float32) <= 1.0
    old_bound = 1e-5 * float(np.abs(oI).max())
    cases = {"drop": _numpy_splat(go, u, defect="drop"), "fraction": _numpy_splat(go, u, defect="fraction"),
             "lost corner": _numpy_splat(go, u, lose=_quiet_contribution(go, u, wide, old_bound))}
    for name, bad in cases.items():
        units = parity_rule.units(bad, oI, np.float32)
        cells = int(violations(bad, wide, npdt).sum())
        print(f"{sp} {name}: {units:.4f} of the max-norm bound, {cells} cells over the cell-wise bound, "
              f"worst {worst_ratio(bad, wide, npdt):.1f} x")
        assert units <= 1.0, f"{name}: the max-norm criterion was expected to accept this defect ({units:.3f})"
        assert cells >= 1, f"{name}: the cell-wise bound did not reject the defect"
        with pytest.raises(AssertionError, match="over the bound"):
            assert_cells(bad, wide, npdt, name, ref=oI)


@pytest.mark.parametrize("sp", [(9, 5, 70), (64, 64, 64)])
def test_weight_defects_show_on_the_suite_data_too(sp):
    """The same two weight defects on the suite's wild field alone, nothing planted: fewer cells, and none at (130, 200),
    which is why the test above plants its samples -- but the rejection is not only a constructed best case."""
    go, u = sc.interp_inputs(sp, 2, 1, np.float32)
    oI, _ = orc.interp_backward(go, np.zeros((2, 1) + sp, np.float32), u, 1.0, True, False)
    wide = orc.interp_backward_wide(go, u, 1.0)
    assert_cells(_numpy_splat(go, u), wide, np.float32, f"numpy splat without defect {sp}")
    for defect in ("drop", "fraction"):
        bad = _numpy_splat(go, u, defect=defect)
        cells = int(violations(bad, wide, np.float32).sum())
        print(f"{sp} {defect}, unplanted: {parity_rule.units(bad, oI, np.float32):.4f} of the max-norm bound, {cells} cells over")
        assert parity_rule.units(bad, oI, np.float32) <= 1.0
        assert cells >= 1


@pytest.mark.parametrize("npdt", NPDT)
@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_non_finite_values_are_rejected(npdt, poison):
    """A NaN or an infinity is over every bound: in the fullest cell, in a quiet cell, in an empty cell, and in a face
    cell of a large-matrix affine case whose float32 bound is the weak product form."""
    sp = (9, 5, 70)
    go, u = sc.interp_inputs(sp, 2, 1, npdt)
    oI, _ = orc.interp_backward(go, np.zeros((2, 1) + sp, npdt), u, 1.0, True, False)
    wide = orc.interp_backward_wide(go, u, 1.0)
    assert_cells(oI, wide, npdt, "clean")
    count = wide[2]
    assert (count == 0).any()
    spots = [np.unravel_index(int(count.argmax()), count.shape), np.unravel_index(int(np.where(count > 0, count, np.inf).argmin()), count.shape),
             np.unravel_index(int((count == 0).argmax()), count.shape)]
    for at in spots:
        bad = oI.copy()
        bad[at] = poison
        assert violations(bad, wide, npdt)[at]
        r = worst_ratio(bad, wide, npdt)
        assert np.isnan(r) or r == np.inf
        with pytest.raises(AssertionError, match="over the bound"):
            assert_cells(bad, wide, npdt, f"{poison} at {at}")
    # a start value does not hide it either
    start = sc.normal(np.random.default_rng(3), oI.shape, npdt)
    bad = oI.astype(np.float64) + start
    bad = bad.astype(npdt)
    assert_cells(bad, wide, npdt, "clean, with start", start=start)
    bad[spots[0]] = poison
    with pytest.raises(AssertionError, match="over the bound"):
        assert_cells(bad, wide, npdt, "poisoned, with start", start=start)


def test_non_finite_values_are_rejected_in_the_loudest_face_cell():
    name, shape, A, T, srcs, go = abc.gpu_adversarial_inputs(6, np.float32)
    I = np.zeros((2, 1) + shape, np.float32)
    oI, _, _ = orc.affine_interp_backward(go, I, A, T, True, False, False)
    wI, _, _ = orc.affine_interp_backward_wide(go, I, A, T, True, False, False)
    at = np.unravel_index(int(wI[2].argmax()), wI[2].shape)
    for poison in (np.nan, np.inf):
        bad = oI.copy()
        bad[at] = poison
        with pytest.raises(AssertionError, match="over the bound"):
            assert_cells(bad, wI, np.float32, name)
    # and a finite value that lost the cell's whole sum is rejected as well once it is off by more than the bound
    bad = oI.copy()
    bad[at] = oI[at] + np.float32(4.0) * np.float32(cell_bound(wI[1], wI[2], np.float32)[at]) + np.float32(1.0)
    with pytest.raises(AssertionError, match="over the bound"):
        assert_cells(bad, wI, np.float32, name)


# ---------------------------------------------------------------- what cannot serve as the yardstick


def test_upcast_float64_oracle_is_not_a_yardstick():
    """The float64 oracle on the upcast float32 inputs rounds the positions i + dt u in float64: other positions, other
    weights.  The float32 oracle -- correct by definition -- is far outside the cell-wise bound around that result, so
    nobody may 'simplify' the yardstick to it."""
    sp = (130, 200)
    go, u = sc.interp_inputs(sp, 2, 1, np.float32)
    I = np.zeros((2, 1) + sp, np.float32)
    o32, _ = orc.interp_backward(go, I, u, 0.8, True, False)
    o64, _ = orc.interp_backward(go.astype(np.float64), I.astype(np.float64), u.astype(np.float64), 0.8, True, False)
    wide = orc.interp_backward_wide(go, u, 0.8)
    assert_cells(o32, wide, np.float32, "oracle f32 against its own wide sum")
    upcast = (o64, wide[1], wide[2])
    assert violations(o32, upcast, np.float32).any()
    assert worst_ratio(o32, upcast, np.float32) > 100.0
    # while the two agree in the max norm: the difference is invisible to the older criterion
    assert parity_rule.units(o32, o64, np.float32) <= 1.0
