"""GPU: affine_interp_backward's image gradient where its two kernels split the batch between them.

affine_splat_box_kernel (affine.hip) takes the items affine_item_regular (common.hpp) accepts, the gated general
tiled kernel (splat.hip) the others; a source the box kernel's candidate range misses is dropped silently.  Every
float32 d_I here is held, CELL BY CELL, against tests/affine_ref.py:

    |HIP - float64 sum of the same n float32 terms| <= u (n + 1) S,   u = 2^-24,  S = sum |term|,

which holds for any order the atomics and the LDS windows add in (affine_ref's docstring) and which a dropped or
doubled term breaks outright in a cell with few terms -- tests/test_affine_ref.py asserts, on the CPU, that the
adversarial cases below have their directed sources in such cells.  The three routes are compared: target boxes (the
default), the general tiled kernel alone (tune(affine_box=0)) and global atomics (set_splat_mode(0)).  float64 inputs
stay on the comparison with the oracle (affine_ref is float32 only: it has no exact double fma).  Worst ratio per
route: OBSERVED / LAGO_TOL_REPORT of test_gpu_parity.py, keys "affine d_I per cell (...)".
"""
import json
import os

import numpy as np
import pytest
import torch

import affine_box_cases as cases
import affine_ref as ref
from gpu_util import DTYPES, OBSERVED, assert_close, dev, host
from oracle import lago_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    import lagomorph_amd

    lagomorph_amd.set_debug_mode(True)
    e = lagomorph_amd.lagomorph_ext
    try:
        yield e
    finally:
        e.tune(affine_box=1)
        e.set_splat_mode(1)
        out = os.environ.get("LAGO_TOL_REPORT")
        if out:
            json.dump(dict(sorted(OBSERVED.items())), open(out, "w"), indent=1)


def np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def three_routes(ext, go, I, A, T, box_expected):
    """d_I by target boxes (asserting that the box kernel was / was not launched), by the tiled kernel, by global atomics."""
    args = (dev(go), dev(I), dev(A), dev(T), True, False, False)
    before = ext.path_launches("splat_affine_box")
    out = {"boxes": ext.affine_interp_backward(*args)[0]}
    assert ext.path_launches("splat_affine_box") == before + (1 if box_expected else 0)
    ext.tune(affine_box=0)
    try:
        out["tiled"] = ext.affine_interp_backward(*args)[0]
    finally:
        ext.tune(affine_box=1)
    assert ext.path_launches("splat_affine_box") == before + (1 if box_expected else 0)
    ext.set_splat_mode(0)
    try:
        out["global atomics"] = ext.affine_interp_backward(*args)[0]
    finally:
        ext.set_splat_mode(1)
    return out


def check_dI(routes, go, I, A, T, bc, dtype, what, oracle_too=True):
    """float32: per cell against affine_ref; both dtypes: the existing yardstick against the oracle (unless the case's
    face cells hold sums of 1e5 .. 1e6 float32 terms, for which the float32 oracle's sequential sum is no truth)."""
    if dtype == torch.float32:
        r = ref.backward_dI(go, A, T, bc)
        for route, dI in routes.items():
            ratio, at = ref.worst_ratio(host(dI), r)
            key = f"affine d_I per cell ({route}) f32"
            OBSERVED[key] = max(OBSERVED.get(key, 0.0), ratio)
            print(f"{what} [{route}]: worst |HIP - ref| / (u (n + 1) S) = {ratio:.3f} at {at}, n = {r[1][at]}")
            assert ratio <= 1.0, f"{what} [{route}]: cell {at} is off by {ratio:.2f} bounds (n = {r[1][at]}, S = {r[2][at]:.3e})"
    if oracle_too:
        oI, _, _ = orc.affine_interp_backward(go, I, A, T, True, False, False)
        for route, dI in routes.items():
            assert_close(dI, oI, dtype, f"affine d_I partition ({route})")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("idx", range(len(cases.GPU_ADVERSARIAL)))
def test_large_regular_matrices(ext, dtype, idx):
    """Regular matrices with entries of 500 .. 999.99 and inverse row sums up to 3.98, translated so that an in-grid
    source hits a box corner: the cases the host walk ranked highest by needed slack (affine_box_cases.GPU_ADVERSARIAL).
    Nearly every source is clamped onto a face, whose cells sum up to a million terms; the sources that land inside are
    judged per cell.  float64: against the oracle."""
    name, shape, A, T, srcs, go = cases.gpu_adversarial_inputs(idx, np_dtype(dtype))
    I = np.zeros((2, 1) + shape, go.dtype)   # (d_I does not depend on I)
    routes = three_routes(ext, go, I, A, T, True)
    check_dI(routes, go, I, A, T, False, dtype, name, oracle_too=dtype == torch.float64)


def mixed_batch(dtype):
    th = cases.threshold_matrices()
    names = list(th)
    A = np.stack([th[k][0] for k in names]).astype(np_dtype(dtype))
    regular = [th[k][1] for k in names]
    rng = np.random.default_rng(31)
    T = (1.5 * rng.standard_normal((len(names), 3))).astype(A.dtype)
    return names, A, T, regular


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("bc", [False, True])
def test_mixed_batch_across_the_thresholds(ext, dtype, nc, bc):
    """One call whose items sit on both sides of every threshold of affine_item_regular (finite values only): each item
    is splatted exactly once, by one of the two kernels -- a dropped or doubled item is a 100 % error in every cell it
    reaches.  Broadcast sums share cells, so each item is also run alone and compared with itself inside the batch."""
    names, A, T, regular = mixed_batch(dtype)
    assert any(regular) and not all(regular)
    nn, shape = len(names), (24, 20, 70)
    rng = np.random.default_rng(7 + nc)
    go = cases.gpu_go(rng, (nn, nc) + shape, A.dtype)
    I = rng.standard_normal(((1 if bc else nn), nc) + shape).astype(A.dtype)
    routes = three_routes(ext, go, I, A, T, True)
    check_dI(routes, go, I, A, T, bc, dtype, f"mixed batch nc={nc} bc={bc}")
    if bc:
        In = np.repeat(I, nn, axis=0)
        inside = host(ext.affine_interp_backward(dev(go), dev(In), dev(A), dev(T), True, False, False)[0])
        for q, k in enumerate(names):
            alone = ext.affine_interp_backward(dev(go[q:q + 1]), dev(I), dev(A[q:q + 1]), dev(T[q:q + 1]), True, False, False)[0]
            if dtype == torch.float32:
                r = ref.backward_dI(go[q:q + 1], A[q:q + 1], T[q:q + 1], False)
                for what, got in (("alone", host(alone)), ("inside the batch", inside[q:q + 1])):
                    ratio, at = ref.worst_ratio(got, r)
                    assert ratio <= 1.0, f"item {k} {what}: cell {at} is off by {ratio:.2f} bounds"
            assert_close(alone, inside[q:q + 1], dtype, f"affine d_I item alone vs in the mixed batch ({k})")


c6, s6 = np.cos(0.6), np.sin(0.6)
MILD = {
    "rotation": [[c6, -s6, 0], [s6, c6, 0], [0, 0, 1]],
    "rotation_yz": [[1, 0, 0], [0, c6, -s6], [0, s6, c6]],
    "zoom_out": np.diag([0.4, 0.4, 0.4]),
    "zoom_in": np.diag([2.5, 2.5, 2.5]),
    "near_identity": np.eye(3) + 0.02 * np.random.default_rng(3).standard_normal((3, 3)),
}
# (grid, does the box kernel run?)  affine_splat_boxes (affine.hip) takes nz >= 16, nx >= 2, ny >= 2 and needs make_tiles
# (splat.hip, affine_cfg = 16 x 8 x 64 tiles) to accept the grid for the gated general kernel: that refuses only a tile
# of fewer than 256 voxels in a grid of 256 or more, which none of these is ((2, 2, 16) has 64 voxels in all).
GEOMETRY = [
    ((8, 8, 48), True),      # exactly one box
    ((9, 17, 49), True),     # one cell over on every axis
    ((7, 9, 97), True),
    ((2, 2, 16), True),      # the smallest grid the box path takes: 4 candidate rows, one per wave, the unrolled rows 2 and 3 all tail
    ((3, 40, 15), False),    # nz < 16: declined, the general kernel does every item
    ((1, 9, 64), False),     # nx < 2: declined
    ((16, 16, 200), True),   # five z boxes per row; the candidate z range of a box is longer than 64: the lane loop runs twice
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,box", GEOMETRY)
@pytest.mark.parametrize("nc,bc", [(1, False), (3, True), (4, False)])
def test_box_geometry_edges(ext, dtype, shape, box, nc, bc):
    """Grids that whole 8 x 8 x 48 boxes do not cover, with mild matrices (the candidate row counts of these are not
    multiples of 4 * LAGO_BOX_ROWS, so the unrolled row loop ends in its tail), all three outputs."""
    rng = np.random.default_rng(abs(hash((shape, nc))) % 2**31)
    A = np.stack([np.asarray(m, np.float64) for m in MILD.values()]).astype(np_dtype(dtype))
    nn = A.shape[0]
    T = (1.5 * rng.standard_normal((nn, 3))).astype(A.dtype)
    go = cases.gpu_go(rng, (nn, nc) + shape, A.dtype)
    I = rng.standard_normal(((1 if bc else nn), nc) + shape).astype(A.dtype)
    routes = three_routes(ext, go, I, A, T, box)
    check_dI(routes, go, I, A, T, bc, dtype, f"geometry {shape} nc={nc} bc={bc}")
    before = ext.path_launches("splat_affine_box")
    dI, dA, dT = ext.affine_interp_backward(dev(go), dev(I), dev(A), dev(T), True, True, True)
    assert ext.path_launches("splat_affine_box") == before + (1 if box else 0)
    oI, oA, oT = orc.affine_interp_backward(go, I, A, T, True, True, True)
    assert_close(dI, oI, dtype, "affine d_I partition (all three outputs)")
    assert_close(dA, oA, dtype, "affine d_A partition")
    assert_close(dT, oT, dtype, "affine d_T partition")
