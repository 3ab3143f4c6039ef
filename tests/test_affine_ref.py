"""tests/affine_ref.py pinned to the CPU oracle, and the GPU cases of tests/test_gpu_affine_partition.py checked for
what they can see -- all on the CPU, so that a case that could not notice a dropped source never reaches a GPU.

  * the reference's positions, floors and clamps reproduce oracle affine_interp_forward bit for bit;
  * |reference - oracle d_I| <= u (n + 1) S per cell: the oracle sums its n float32 terms sequentially, which the bound
    covers by derivation (affine_ref's docstring);
  * every committed adversarial case is SENSITIVE where it matters: a cell is sensitive when n (n + 1) u <= 1/16 (one
    missing term of average size is then sixteen bounds); (a) the eight cells of each directed corner source are
    sensitive, (b) so are at least 90 % of the cells that are not on a grid face;
  * and the per-cell comparison REJECTS the oracle's d_I with one directed source's eight terms taken out.
"""
import numpy as np
import pytest

import affine_box_cases as cases
import affine_ref as ref
from oracle import lago_oracle as orc

F = np.float32


def _mild_inputs(shape, nn, nc, bc, seed):
    rng = np.random.default_rng(seed)
    mats = list(cases.mild_matrices().values())
    A = np.stack([mats[(seed + q) % len(mats)] for q in range(nn)])
    T = (2.0 * rng.standard_normal((nn, 3))).astype(F)
    I = rng.standard_normal(((1 if bc else nn), nc) + shape).astype(F)
    go = cases.gpu_go(rng, (nn, nc) + shape, F)
    return I, A, T, go


@pytest.mark.parametrize("shape,nn,nc,bc", [((9, 17, 49), 3, 2, False), ((7, 9, 97), 2, 1, True), ((36, 20, 70), 4, 1, False),
                                            ((2, 2, 16), 2, 3, True)])
def test_reference_reproduces_the_oracle(shape, nn, nc, bc):
    for seed in range(4):
        I, A, T, go = _mild_inputs(shape, nn, nc, bc, seed)
        assert np.array_equal(ref.forward(I, A, T), orc.affine_interp_forward(I, A, T)), "forward bits"
        oI, _, _ = orc.affine_interp_backward(go, I, A, T, True, False, False)
        r = ref.backward_dI(go, A, T, bc)
        ratio, at = ref.worst_ratio(oI, r)
        assert ratio <= 1.0, (ratio, at)
        assert r[1].sum() == 8 * nn * nc * np.prod(shape)   # every source, eight terms, once


def _adversarial(idx):
    name, shape, A, T, srcs, go = cases.gpu_adversarial_inputs(idx)
    return name, shape, A, T, srcs, go, ref.backward_dI(go, A, T, False)


@pytest.mark.parametrize("idx", range(len(cases.GPU_ADVERSARIAL)))
def test_adversarial_gpu_cases_can_see_a_dropped_source(idx):
    name, shape, A, T, srcs, go, r = _adversarial(idx)
    tot, n, S = r
    # the inputs are what they claim: regular by the numbers, positions pinned to the oracle's forward
    assert cases.inv_rowsum(A[0]) <= 4.0 and np.abs(A).max() < 1e3
    I = np.random.default_rng(idx).standard_normal((2, 1) + shape).astype(F)
    assert np.array_equal(ref.forward(I, A, T), orc.affine_interp_forward(I, A, T)), f"{name}: forward bits"
    oI, _, _ = orc.affine_interp_backward(go, I, A, T, True, False, False)
    ratio, at = ref.worst_ratio(oI, r)
    print(f"{name}: oracle / bound = {ratio:.3f} at {at}; max n = {n.max()}")
    assert ratio <= 1.0, (name, ratio, at)
    sens = ref.sensitive(n)
    inner = ref.interior(shape)
    for item, s in enumerate(srcs):
        # (a) the directed source is in the grid, away from the faces, and all of its eight cells are sensitive
        flat = int(np.ravel_multi_index(s, shape))
        tw = ref.terms(A[item], T[item], shape)
        cells = [int(c[flat]) for c, _ in tw]
        assert len(set(cells)) == 8, f"{name} item {item}: the directed source {s} is clamped"
        for c in cells:
            pos = np.unravel_index(c, shape)
            assert inner[pos], (name, item, s, pos)
            assert sens[item, 0][pos], f"{name} item {item}: cell {pos} of the directed source has n = {n[item, 0][pos]}"
        # ... and the comparison rejects a result that lacks exactly this source
        broken = oI.astype(np.float64)
        for c, w in tw:
            broken[item, 0].reshape(-1)[c[flat]] -= np.float64(F(w[flat] * go[item, 0].reshape(-1)[flat]))
        bad, _ = ref.worst_ratio(broken, r)
        assert bad > 1.0, f"{name} item {item}: a dropped source passes the per-cell bound (ratio {bad:.3f})"
        # (b)
        frac = sens[item, 0][inner].mean()
        assert frac >= 0.9, f"{name} item {item}: only {frac:.1%} of the interior cells are sensitive"
