"""GPU: every scatter-add output of the library, cell by cell, against the oracle's wide sums with the bound of
tests/scatter_bound.py -- a theorem of floating-point summation, no tolerance, no multiplier, every cell judged (the
max-norm tests of test_gpu_parity.py and its siblings allow a typical cell a thousand times its own rounding scale).

  interp_backward d_I       global atomics, tiled (any tile configuration), sheared one / several channels, 2D LDS,
                            the production geometries at 128^3 and 160^3
  interp_backward_fused     addgo, a running d_I (one more term: the start value), the reverse sweep's combination
  affine_interp_backward    d_I by target boxes, by the general tiled kernel, by global atomics, incl. the large matrices
  regrid_backward           separable, tiled, global atomics, and what the separable entry hands back to the splat
  interp_hessian_diagonal_image
  affine d_A / d_T          millions of cancelling terms into one number: the rigorous bound says nothing, so HIP and the
                            float oracle are each measured against the wide sum in the project's max-norm unit

`path_launches` tells which kernel served each call; the worst err / bound per path goes into OBSERVED (LAGO_TOL_REPORT)
under "cell ..." keys.
"""
import json
import os

import numpy as np
import pytest
import torch

import affine_box_cases as abc
import scatter_cases as sc
from gpu_util import DTYPES, OBSERVED, SHAPES2, SHAPES3, dev, host
from oracle import lago_oracle as orc
from parity_rule import rtol, units
from scatter_bound import assert_cells, worst_ratio

pytestmark = pytest.mark.gpu

SPLAT_PATHS = ("splat_shear", "splat_shear_mc", "splat_tiled", "splat_global", "splat_2d", "splat_affine_box")
DEFAULT_SHEAR = (1, 8, 6, 0, 1, 1, 4, 1024)
DEFAULT_TILE = (0, 8, 0, 1, 1, 4, 512)


@pytest.fixture(scope="module")
def ext():
    import lagomorph_amd

    lagomorph_amd.set_debug_mode(True)
    e = lagomorph_amd.lagomorph_ext
    try:
        yield e
    finally:
        e.set_splat_shear(*DEFAULT_SHEAR)
        e.set_splat_shear_mc(2)
        e.set_splat_mc(1)
        e.set_splat_mode(1)
        e.set_splat_tile(*DEFAULT_TILE)
        e.tune(affine_box=1)
        e.REGRID_BACKWARD_SEPARABLE = 1
        out = os.environ.get("LAGO_TOL_REPORT")
        if out:
            json.dump(dict(sorted(OBSERVED.items())), open(out, "w"), indent=1)


def npdt(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def tag(dtype):
    return "f32" if dtype == torch.float32 else "f64"


class Paths:
    """with Paths(ext) as p: ...; p.ran -> the splat paths whose launch counter moved inside the block."""

    def __init__(self, ext):
        self.ext = ext

    def __enter__(self):
        self.before = self.ext.path_launches()
        return self

    def __exit__(self, *exc):
        after = self.ext.path_launches()
        self.ran = tuple(k for k in SPLAT_PATHS if after[k] != self.before[k])
        self.count = {k: after[k] - self.before[k] for k in self.ran}
        return False


def _note(key, value):
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), value)


def judge(got, wide, dtype, op, path, what, start=None, ref=None):
    """Every cell of `got` within its bound of the wide sum.  Recorded in OBSERVED: the worst err / bound under
    'cell <op> [<path>]' and the same error in the max-norm unit (RTOL x max |wide sum|) under 'wide <op> [<path>]';
    with `ref`, the float oracle's result of the same call, its own two figures under '[oracle]' and the older direct
    comparison HIP against oracle under 'direct <op> [<path>]' -- so that profiles/scatter_cell_bound.md can say how much
    of a direct figure is the oracle's own summation error."""
    g = host(got) if torch.is_tensor(got) else np.asarray(got)
    t = tag(dtype)
    _note(f"cell {op} [{path}] {t}", worst_ratio(g, wide, npdt(dtype), start))
    if start is None:
        _note(f"wide {op} [{path}] {t}", units(g, wide[0], dtype))
        if ref is not None:
            _note(f"cell {op} [oracle] {t}", worst_ratio(ref, wide, npdt(dtype)))
            _note(f"wide {op} [oracle] {t}", units(ref, wide[0], dtype))
            _note(f"direct {op} [{path}] {t}", units(g, ref, dtype))
    return assert_cells(g, wide, npdt(dtype), f"{what} [{path}]", start, ref)


# ---------------------------------------------------------------- interp_backward d_I


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", SHAPES3 + SHAPES2)
@pytest.mark.parametrize("nn,nc,bc", [(2, 1, False), (3, 3, True), (2, 3, False)])
def test_interp_backward_global_and_default(ext, dtype, sp, nn, nc, bc):
    """splat_mode 0 (the reference's form: one global atomic per corner) and whatever the library picks by default at
    the parity suite's shapes, wild field, dt = 1, -1, 0.8, broadcast image or not."""
    go, u = sc.interp_inputs(sp, nn, nc, npdt(dtype))
    I = np.zeros(((1 if bc else nn), nc) + sp, go.dtype)
    for dt in (1.0, -1.0, 0.8):
        wide = orc.interp_backward_wide(go, u, dt, broadcast_I=bc)
        ref = orc.interp_backward(go, I, u, dt, True, False)[0]
        ext.set_splat_mode(0)
        try:
            with Paths(ext) as p:
                dI, _ = ext.interp_backward(dev(go), dev(I), dev(u), dt, True, False)
        finally:
            ext.set_splat_mode(1)
        assert p.ran == ("splat_global",), p.ran
        judge(dI, wide, dtype, "interp_backward d_I", "splat_global", f"{sp} dt={dt} bc={bc} nc={nc}", ref=ref)
        for need_u in (True, False):
            with Paths(ext) as p:
                dI, _ = ext.interp_backward(dev(go), dev(I), dev(u), dt, True, need_u)
            assert len(p.ran) == 1, p.ran
            judge(dI, wide, dtype, "interp_backward d_I", p.ran[0], f"{sp} dt={dt} bc={bc} nc={nc} need_u={need_u}", ref=ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["wild", "smooth"])
@pytest.mark.parametrize("tile", [(4, 4, 0, 1, 1, 16, 256), (2, 3, 16, 0, 0, 0, 256), (8, 8, 0, 2, 2, 16, 512),
                                  (16, 16, 16, 2, 2, 2, 1024)])
def test_tiled_splat_tile_configs(ext, dtype, kind, tile):
    """splat_tiled_kernel (the sheared kernel switched off, which would take every float32 3D call first) under the tile
    configurations of test_tiled_splat_any_tile_config, windows too small for the displacement included."""
    sp = (12, 10, 40)
    go, u = sc.interp_inputs(sp, 2, 2, npdt(dtype), kind=kind)
    for bc in (False, True):
        I = np.zeros(((1 if bc else 2), 2) + sp, go.dtype)
        for dt in (1.0, -1.0, 0.8):
            wide = orc.interp_backward_wide(go, u, dt, broadcast_I=bc)
            ref = orc.interp_backward(go, I, u, dt, True, False)[0]
            for mc in (1, 0):
                ext.set_splat_shear(0, *DEFAULT_SHEAR[1:])
                ext.set_splat_tile(*tile)
                ext.set_splat_mc(mc)
                try:
                    with Paths(ext) as p:
                        dI, _ = ext.interp_backward(dev(go), dev(I), dev(u), dt, True, True)
                finally:
                    ext.set_splat_shear(*DEFAULT_SHEAR)
                    ext.set_splat_tile(*DEFAULT_TILE)
                    ext.set_splat_mc(1)
                # (a tile of fewer than 256 voxels is "not worth a window": make_tiles, csrc/splat.hip, hands the call to
                # the plain kernel -- the 2 x 3 x 16 configuration)
                want = "splat_global" if tile[0] * tile[1] * tile[2] in range(1, 256) else "splat_tiled"
                assert p.ran == (want,), (p.ran, tile)
                judge(dI, wide, dtype, "interp_backward d_I", want, f"{kind} tile={tile} dt={dt} bc={bc} mc={mc}", ref=ref)


@pytest.mark.parametrize("kind", ["wild", "smooth"])
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("bc", [False, True])
def test_sheared_splat(ext, kind, nc, bc):
    """splat_shear_kernel (one channel) and splat_shear_mc_kernel (three channels with d_u), float32 3D, at the sweep's
    (40, 36, 96) in the default configuration."""
    sp = (40, 36, 96)
    go, u = sc.interp_inputs(sp, 2, nc, np.float32, kind=kind)
    I = np.zeros(((1 if bc else 2), nc) + sp, np.float32)
    seen = set()
    for dt in (1.0, -1.0, 0.8):
        wide = orc.interp_backward_wide(go, u, dt, broadcast_I=bc)
        ref = orc.interp_backward(go, I, u, dt, True, False)[0]
        for need_u in (True, False):
            with Paths(ext) as p:
                dI, _ = ext.interp_backward(dev(go), dev(I), dev(u), dt, True, need_u)
            assert set(p.ran) <= {"splat_shear", "splat_shear_mc"} and p.ran, p.ran
            seen |= set(p.ran)
            judge(dI, wide, torch.float32, "interp_backward d_I", "+".join(p.ran), f"{kind} {sp} C={nc} dt={dt} bc={bc} need_u={need_u}", ref=ref)
    assert ("splat_shear_mc" if nc > 1 else "splat_shear") in seen, seen


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", sc.LDS2D_SHAPES)
@pytest.mark.parametrize("nn,nc,bc", [(2, 1, False), (3, 3, True), (2, 2, False)])
@pytest.mark.parametrize("kind", ["smooth", "wild"])
def test_2d_lds_splat(ext, dtype, sp, nn, nc, bc, kind):
    """splat2d_lds_kernel on the five shapes of test_interp_backward_2d_lds_splat: everything inside the windows
    (smooth) and mostly outside (wild: the global-atomic fall-back per corner)."""
    go, u = sc.interp_inputs(sp, nn, nc, npdt(dtype), kind=kind)
    I = np.zeros(((1 if bc else nn), nc) + sp, go.dtype)
    for dt in (1.0, -1.0, 0.8):
        wide = orc.interp_backward_wide(go, u, dt, broadcast_I=bc)
        ref = orc.interp_backward(go, I, u, dt, True, False)[0]
        for need_u in (True, False):
            with Paths(ext) as p:
                dI, _ = ext.interp_backward(dev(go), dev(I), dev(u), dt, True, need_u)
            assert p.ran == ("splat_2d",), p.ran
            judge(dI, wide, dtype, "interp_backward d_I", "splat_2d", f"{kind} {sp} dt={dt} bc={bc} nc={nc} need_u={need_u}", ref=ref)


def _smooth_gpu(shape, sigma, gen):
    import bench

    return bench.gaussian_blur(torch.randn(shape, device="cuda", generator=gen), sigma)


def _judge_items(ext, dI, go, u, dt, what, path):
    """The production volumes item by item (an item's planes are its own: the wide sums of one item at a time keep the
    host arrays small)."""
    orc.set_threads(min(os.cpu_count() or 1, 16))
    try:
        for n in range(go.shape[0]):
            wide = orc.interp_backward_wide(go[n:n + 1], u[n:n + 1], dt)
            for name, t in dI.items():
                judge(t[n:n + 1], wide, torch.float32, "interp_backward d_I production", path, f"{what} item {n} ({name})")
    finally:
        orc.set_threads(1)


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("dt", [1.0, -0.2])
def test_production_geometry_128(ext, nc, dt):
    """test_config1_splat_production_geometry_vs_oracle's call (8 x nc x 128^3, its input builder), all eight items and
    every one of their cells instead of two items in the max norm."""
    g = torch.Generator(device="cuda").manual_seed(11)
    N, S = 8, 128
    I = _smooth_gpu((N, nc, S, S, S), 2.0, g)
    I = I / I.std()
    u = _smooth_gpu((N, 3, S, S, S), 8.0, g)
    u = u * (4.0 / u.abs().max())
    go = torch.randn((N, nc, S, S, S), device="cuda", generator=g)
    with Paths(ext) as p:
        dI, _ = ext.interp_backward(go, I, u, dt, True, True)
        dI2, _ = ext.interp_backward(go, I, u, dt, True, False)
    assert set(p.ran) <= {"splat_shear", "splat_shear_mc"} and sum(p.count.values()) == 2, p.count
    _judge_items(ext, {"with d_u": dI, "d_I only": dI2}, host(go), host(u), dt, f"128^3 C={nc} dt={dt}", "+".join(p.ran))


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("dt", [1.0, -0.2])
def test_production_geometry_160(ext, nc, dt):
    """test_config4_splat_production_geometry_160_vs_oracle's call (2 x nc x 160^3), both items, every cell."""
    g = torch.Generator(device="cuda").manual_seed(160 + nc)
    N, S = 2, 160
    I = _smooth_gpu((N, nc, S, S, S), 2.0, g)
    I = I / I.std()
    u = _smooth_gpu((N, 3, S, S, S), 8.0, g)
    u = u * (4.0 / u.abs().max())
    go = torch.randn((N, nc, S, S, S), device="cuda", generator=g)
    with Paths(ext) as p:
        dI, _ = ext.interp_backward(go, I, u, dt, True, True)
        dI2, _ = ext.interp_backward(go, I, u, dt, True, False)
    assert set(p.ran) <= {"splat_shear", "splat_shear_mc"} and sum(p.count.values()) == 2, p.count
    _judge_items(ext, {"with d_u": dI, "d_I only": dI2}, host(go), host(u), dt, f"160^3 C={nc} dt={dt}", "+".join(p.ran))


# ---------------------------------------------------------------- interp_backward_fused


# The kernel that serves interp_backward_fused (d_u wanted, default settings) at each shape, by the dispatch rules of
# csrc/interp.hip and csrc/splat.hip: thin volumes and small 2D fields take the plain kernel, 2D fields of 8192 pixels
# and more the 2D LDS splat; float32 3D volumes whose sheared tile has at least 256 voxels the sheared kernels (several
# channels: the geometry-once form), every other 3D volume the tiled kernel.
FUSED_SHAPES = {(6, 5, 8): "tiled", (7, 9): "global", (4, 3, 70): "shear", (12, 10, 40): "shear", (3, 4, 1): "global",
                (130, 200): "2d"}


def _fused_path(sp, dtype, nc):
    kind = FUSED_SHAPES[sp]
    if kind == "shear":
        return ("splat_shear_mc" if nc > 1 else "splat_shear") if dtype == torch.float32 else "splat_tiled"
    return {"tiled": "splat_tiled", "global": "splat_global", "2d": "splat_2d"}[kind]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", list(FUSED_SHAPES))
@pytest.mark.parametrize("dt", [1.0, -0.3])
def test_fused_start_values(ext, dtype, sp, dt):
    """interp_backward_fused at the shapes of test_interp_backward_fused_start_values (and one 2D LDS shape): d_I with
    addgo, with a running d_u, and added onto a running d_I -- one more term per cell, its start value."""
    d = len(sp)
    rng = np.random.default_rng(hash((sp, dt)) % 2**31)
    u = sc.disp(rng, 2, sp, npdt(dtype))
    for nc, bc in ((d, False), (1, False), (2, True)):
        I = sc.normal(rng, (1 if bc else 2, nc) + sp, u.dtype)
        go = sc.normal(rng, (2, nc) + sp, u.dtype)
        startu = sc.normal(rng, u.shape, u.dtype)
        startI = sc.normal(rng, I.shape, u.dtype)
        wide = orc.interp_backward_wide(go, u, dt, broadcast_I=bc)
        want = (_fused_path(sp, dtype, nc),)
        with Paths(ext) as p:
            dI, _ = ext.interp_backward_fused(dev(go), dev(I), dev(u), dt, True, d_u=dev(startu))
        assert p.ran == want, (p.ran, want)
        judge(dI, wide, dtype, "interp_backward_fused d_I", want[0], f"running d_u {sp} dt={dt} nc={nc} bc={bc}")
        if nc == d:
            with Paths(ext) as p:
                dI, _ = ext.interp_backward_fused(dev(go), dev(I), dev(u), dt, True, addgo=0.37)
            assert p.ran == want, (p.ran, want)
            judge(dI, wide, dtype, "interp_backward_fused d_I", want[0], f"addgo {sp} dt={dt}")
        run_I = dev(startI)
        with Paths(ext) as p:
            dI, _ = ext.interp_backward_fused(dev(go), dev(I), dev(u), dt, True, d_u=dev(startu), d_I=run_I)
        assert p.ran == want, (p.ran, want)
        assert dI.data_ptr() == run_I.data_ptr()
        judge(dI, wide, dtype, "interp_backward_fused running d_I", want[0], f"running d_I {sp} dt={dt} nc={nc} bc={bc}",
              start=startI)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", [(20, 12, 40), (9, 11, 33)])
@pytest.mark.parametrize("shear,mode", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("bc", [False, True])
def test_fused_production_combination(ext, dtype, sp, shear, mode, bc):
    """The calls of the expmap reverse sweep (test_fused_backward_production_combination): need_I with addgo, and need_I
    with a running d_u and a running d_I, three channels, through the sheared, the tiled and the plain-atomic kernel."""
    rng = np.random.default_rng(hash((sp, shear, mode, bc)) % 2**31)
    u = sc.disp(rng, 2, sp, npdt(dtype))
    I = sc.normal(rng, (1 if bc else 2, 3) + sp, u.dtype)
    go = sc.normal(rng, (2, 3) + sp, u.dtype)
    startu = sc.normal(rng, (2, 3) + sp, u.dtype)
    startI = sc.normal(rng, I.shape, u.dtype)
    want = {(1, 1): ({"splat_shear", "splat_shear_mc"} if dtype == torch.float32 else {"splat_tiled"}),
            (0, 1): {"splat_tiled"}, (1, 0): {"splat_global"}}[(shear, mode)]
    ext.set_splat_shear(shear, *DEFAULT_SHEAR[1:])
    ext.set_splat_mode(mode)
    try:
        for dt in (1.0, -0.25):
            wide = orc.interp_backward_wide(go, u, dt, broadcast_I=bc)
            for mc in (2, 1, 0):
                ext.set_splat_shear_mc(mc)
                ext.set_splat_mc(1 if mc else 0)
                with Paths(ext) as p:
                    dI, _ = ext.interp_backward_fused(dev(go), dev(I), dev(u), dt, True, addgo=-0.2)
                assert p.ran and set(p.ran) <= want, (p.ran, want)
                judge(dI, wide, dtype, "interp_backward_fused d_I", "+".join(p.ran), f"addgo {sp} dt={dt} mc={mc} bc={bc}")
                run_I = dev(startI)
                with Paths(ext) as p:
                    dI, _ = ext.interp_backward_fused(dev(go), dev(I), dev(u), dt, True, d_u=dev(startu), d_I=run_I)
                assert p.ran and set(p.ran) <= want, (p.ran, want)
                judge(dI, wide, dtype, "interp_backward_fused running d_I", "+".join(p.ran),
                      f"running d_I {sp} dt={dt} mc={mc} bc={bc}", start=startI)
    finally:
        ext.set_splat_shear(*DEFAULT_SHEAR)
        ext.set_splat_mode(1)
        ext.set_splat_shear_mc(2)
        ext.set_splat_mc(1)


# ---------------------------------------------------------------- affine_interp_backward d_I


def _affine_routes(ext, go, I, A, T, box_expected):
    """d_I by target boxes (the default), by the general tiled kernel, by global atomics.  Only the box kernel has a
    launch counter (LAGO_PATH_*, include/lagomorph_hip.h): the general tiled kernel (affine_splat_lds) and the plain
    reduction kernel have none, so those two routes are pinned by the switches that select them (tune(affine_box=0),
    set_splat_mode(0): csrc/affine.hip, affine_backward_impl) and by no counter of any other splat moving."""
    args = (dev(go), dev(I), dev(A), dev(T), True, False, False)
    with Paths(ext) as p:
        out = {"boxes": ext.affine_interp_backward(*args)[0]}
    assert p.ran == (("splat_affine_box",) if box_expected else ()), p.ran
    ext.tune(affine_box=0)
    try:
        with Paths(ext) as p:
            out["general"] = ext.affine_interp_backward(*args)[0]
        assert p.ran == (), p.ran
        ext.set_splat_mode(0)
        try:
            with Paths(ext) as p:
                out["global atomics"] = ext.affine_interp_backward(*args)[0]
            assert p.ran == (), p.ran
        finally:
            ext.set_splat_mode(1)
    finally:
        ext.tune(affine_box=1)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sc.AFFINE_KINDS)
@pytest.mark.parametrize("bc", [False, True])
def test_affine_backward_image(ext, dtype, kind, bc):
    go, I, A, T = sc.affine_kind_inputs(kind, bc, npdt(dtype))
    wI, _, _ = orc.affine_interp_backward_wide(go, I, A, T, True, False, False)
    ref = orc.affine_interp_backward(go, I, A, T, True, False, False)[0]
    for route, dI in _affine_routes(ext, go, I, A, T, True).items():
        judge(dI, wI, dtype, "affine_interp_backward d_I", route, f"{kind} bc={bc}", ref=ref)
    # and next to d_A / d_T (another kernel instantiation)
    dI, _, _ = ext.affine_interp_backward(dev(go), dev(I), dev(A), dev(T), True, True, True)
    judge(dI, wI, dtype, "affine_interp_backward d_I", "boxes", f"{kind} bc={bc} with d_A, d_T")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("idx", range(len(abc.GPU_ADVERSARIAL)))
def test_affine_backward_image_large_matrices(ext, dtype, idx):
    """The large-matrix cases of tests/affine_box_cases.py.  Most samples leave the grid; a face cell that collects 2^24
    contributions or more is judged by the product form of the bound (scatter_bound docstring)."""
    name, shape, A, T, srcs, go = abc.gpu_adversarial_inputs(idx, npdt(dtype))
    I = np.zeros((2, 1) + shape, go.dtype)
    wI, _, _ = orc.affine_interp_backward_wide(go, I, A, T, True, False, False)
    ref = orc.affine_interp_backward(go, I, A, T, True, False, False)[0]
    for route, dI in _affine_routes(ext, go, I, A, T, True).items():
        judge(dI, wI, dtype, "affine_interp_backward d_I large matrices", route, name, ref=ref)


# ---------------------------------------------------------------- regrid_backward


def _regrid_forms(ext, go, sp, out, origin, spacing):
    """(form, d_I, splat paths that ran): the default entry (separable where the map allows), the tiled splat, global atomics."""
    res = []
    with Paths(ext) as p:
        res.append(("default", ext.regrid_backward(dev(go), sp, out, origin, spacing), p))
    ext.REGRID_BACKWARD_SEPARABLE = 0
    try:
        with Paths(ext) as p:
            res.append(("splat", ext.regrid_backward(dev(go), sp, out, origin, spacing), p))
        ext.set_splat_mode(0)
        try:
            with Paths(ext) as p:
                res.append(("global atomics", ext.regrid_backward(dev(go), sp, out, origin, spacing), p))
        finally:
            ext.set_splat_mode(1)
    finally:
        ext.REGRID_BACKWARD_SEPARABLE = 1
    return res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp,out,scale", sc.REGRID_CASES)
def test_regrid_backward_every_form(ext, dtype, sp, out, scale):
    go, origin, spacing = sc.regrid_inputs(sp, out, scale, npdt(dtype))
    wide = orc.regrid_backward_wide(go, sp, out, origin, spacing)
    ref = orc.regrid_backward(go, sp, out, origin, spacing)
    for form, dI, p in _regrid_forms(ext, go, sp, out, origin, spacing):
        if form == "default" and all(x > 0 for x in spacing):
            assert p.ran == (), p.ran            # lago_regrid_backward_sep: gathers, no splat kernel
            path = "separable"
        elif form == "global atomics":
            assert p.ran == ("splat_global",), p.ran
            path = "splat_global"
        else:
            assert p.ran and set(p.ran) <= {"splat_tiled", "splat_global"}, p.ran
            path = "+".join(p.ran)
        judge(dI, wide, dtype, "regrid_backward", path, f"{sp} <- {out} x {scale} ({form})", ref=ref)


# (the `sep` column of test_regrid_backward_separable_entry_accepts_what_the_reference_accepts: None = float64 only)
REGRID_SEP_EXPECTED = [False, False, None, True, False]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(sc.REGRID_SEP_ENTRY)))
def test_regrid_backward_separable_entry(ext, dtype, case):
    """The inputs of test_regrid_backward_separable_entry_accepts_what_the_reference_accepts, in the form that test pins
    for each: the separable passes (no splat kernel) or the splat the C entry falls back to."""
    origin, spacing = sc.REGRID_SEP_ENTRY[case]
    sep = REGRID_SEP_EXPECTED[case]
    if sep is None:
        sep = dtype == torch.float64
    go, sp, out = sc.regrid_sep_entry_inputs(npdt(dtype))
    wide = orc.regrid_backward_wide(go, sp, out, origin, spacing)
    with Paths(ext) as p:
        dI = ext.regrid_backward(dev(go), sp, out, origin, spacing)
    if sep:
        assert p.ran == (), p.ran
    else:
        assert len(p.ran) == 1 and p.ran[0] in ("splat_tiled", "splat_global"), p.ran
    judge(dI, wide, dtype, "regrid_backward", p.ran[0] if p.ran else "separable", f"entry {origin} {spacing}",
          ref=orc.regrid_backward(go, sp, out, origin, spacing))


# ---------------------------------------------------------------- interp_hessian_diagonal_image


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp,nn,nc", [((9, 8), 2, 3), ((7, 9), 3, 1), ((2, 2), 2, 2), ((5, 1), 1, 1), ((130, 200), 2, 3)])
def test_hessian_diagonal(ext, dtype, sp, nn, nc):
    I, u = sc.hessian_inputs(npdt(dtype), sp, nn, nc)
    for dt in (0.6, 1.0, -1.0):
        wide = orc.interp_hessian_diagonal_image_wide(I, u, dt)
        with Paths(ext) as p:   # (the operator has one kernel and no launch counter; no splat kernel may stand in for it)
            got = ext.interp_hessian_diagonal_image(dev(I), dev(u), dt)
        assert p.ran == (), p.ran
        judge(got, wide, dtype, "interp_hessian_diagonal_image", "atomics", f"{sp} dt={dt}",
              ref=orc.interp_hessian_diagonal_image(I, u, dt))


# ---------------------------------------------------------------- affine d_A / d_T


def _affine_parameter_gradients(ext, dtype, go, I, A, T, what):
    _, dA, dT = ext.affine_interp_backward(dev(go), dev(I), dev(A), dev(T), False, True, True)
    _, oA, oT = orc.affine_interp_backward(go, I, A, T, False, True, True)
    _, wA, wT = orc.affine_interp_backward_wide(go, I, A, T, False, True, True)
    for name, got, ref, w in (("d_A", host(dA), oA, wA), ("d_T", host(dT), oT, wT)):
        hip_units, orc_units = units(got, w[0], dtype), units(ref, w[0], dtype)
        for who, val in (("HIP", hip_units), ("oracle", orc_units)):
            key = f"wide affine {name} [{who}] {tag(dtype)}"
            OBSERVED[key] = max(OBSERVED.get(key, 0.0), val)
        print(f"{what} {name}: HIP {hip_units:.4f}, oracle {orc_units:.4f} of {rtol(dtype):.0e} x max |wide sum|")
        assert hip_units <= 1.0, f"{what} {name}: HIP is {hip_units:.3f} x {rtol(dtype):.0e} x max from the wide sum (oracle: {orc_units:.3f})"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sc.AFFINE_KINDS)
@pytest.mark.parametrize("bc", [False, True])
def test_affine_parameter_gradients(ext, dtype, kind, bc):
    """d_A / d_T: hundreds of thousands of cancelling terms into nine and three numbers.  The rigorous bound is useless
    there; HIP must be within the project's 1e-5 (1e-12) x max of the WIDE sum -- a yardstick without summation error of
    its own -- and the float oracle's distance from it is recorded next to HIP's."""
    go, I, A, T = sc.affine_kind_inputs(kind, bc, npdt(dtype))
    _affine_parameter_gradients(ext, dtype, go, I, A, T, f"{kind} bc={bc}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sp", [(5, 6, 7), (2, 2, 2), (4, 3, 1), (7, 9), (2, 2), (64, 64)])
@pytest.mark.parametrize("nn,nc,bc", [(2, 1, False), (3, 2, True), (2, 4, False)])
def test_affine_parameter_gradients_small(ext, dtype, sp, nn, nc, bc):
    """The shapes and inputs of test_gpu_parity.test_affine_interp."""
    rng = np.random.default_rng(hash((sp, nn, nc, 2)) % 2**31)
    d = len(sp)
    I = sc.normal(rng, ((1 if bc else nn), nc) + sp, npdt(dtype))
    A = (np.eye(d)[None] + 0.3 * rng.standard_normal((nn, d, d))).astype(I.dtype)
    T = (1.5 * rng.standard_normal((nn, d))).astype(I.dtype)
    go = sc.normal(rng, (nn, nc) + sp, npdt(dtype))
    _affine_parameter_gradients(ext, dtype, go, I, A, T, f"{sp} nn={nn} nc={nc} bc={bc}")
    # and d_I at these shapes: 2D has the reduction kernel's atomics only; 3D goes by target boxes where the box kernel
    # takes the shape, else to the general tiled kernel (which has no launch counter, see _affine_routes)
    wI, _, _ = orc.affine_interp_backward_wide(go, I, A, T, True, False, False)
    with Paths(ext) as p:
        dI, _, _ = ext.affine_interp_backward(dev(go), dev(I), dev(A), dev(T), True, True, True)
    assert p.ran in ((() ,) if d == 2 else ((), ("splat_affine_box",))), p.ran
    judge(dI, wI, dtype, "affine_interp_backward d_I", "boxes" if p.ran else ("plain 2D" if d == 2 else "general"),
          f"{sp} nn={nn} nc={nc} bc={bc}")
