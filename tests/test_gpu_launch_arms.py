"""GPU: every arm of the host-side dispatch ladders, at the smallest shapes that reach them.

The kernels are templates over a few flags (bc, need_I, need_u, unit dt, ...) and small integers (threads, voxels per
lane) that csrc/launch.hpp turns into template arguments.  The parity tests cover most combinations at some shape; this
file walks each ladder arm by arm on the path it belongs to: every output against the oracle with the comparison the
parity test of that op makes (test_gpu_parity: assert_bits / assert_close), and `path_launches` says that the intended
kernel family really ran.  The shapes follow from make_shear / make_tiles / slab_grid / the window conditions:

 * sheared-window splat, default tile 8 x 6 x nz: 768 voxels at 16^3 (one pass of 1024 threads), 1536 at (16, 16, 32)
   (two passes);
 * general tiled splat, default tile (auto) x 8 x nz: 16 x 8 x 16 = 2048 voxels at 16^3;
 * slab-unrolled gathers: nz >= 2, 256 / nz + 1 < ny, at least 2048 voxels; LDS window: at least 32768 voxels.
"""
import contextlib
import functools
import itertools

import numpy as np
import pytest
import torch

import gpu_util
from gpu_util import assert_close, dev, displacement, rnd
from oracle import lago_oracle as orc

pytestmark = pytest.mark.gpu
assert_bits = functools.partial(gpu_util.assert_bits, check_dtype=False)   # these sites compare shape and bits, as they always did

F32, F64 = torch.float32, torch.float64
BOOLS = (False, True)


@pytest.fixture(scope="module")
def ext():
    import lagomorph_amd

    lagomorph_amd.set_debug_mode(True)
    shim = lagomorph_amd.lagomorph_ext
    saved = shim.get_tuning()
    try:
        yield shim
    finally:
        shim.tune(**saved)


def _took(ext, f):
    before = ext.path_launches()
    out = f()
    after = ext.path_launches()
    return out, {k: after[k] - before[k] for k in after if after[k] != before[k]}


@contextlib.contextmanager
def _tuned(ext, **fields):
    """The given tuning fields for the body, every field as it was afterwards."""
    saved = ext.get_tuning()
    try:
        ext.tune(**fields)
        yield
    finally:
        ext.tune(**saved)


def _splat_sweep(ext, sp, dtype, want_path, needs=((True, True), (True, False)), ncs=(1, 3), dts=(1.0, -0.3)):
    """interp_backward over bc x (need_I, need_u) x dt x nc; want_path(nc, need_I, need_u) names the counter."""
    nn = 2
    rng = np.random.default_rng(hash(sp + (dtype == F64,)) % 2**31)
    u = displacement(rng, nn, sp, dtype)
    for nc, bc in itertools.product(ncs, BOOLS):
        I = rnd(rng, ((1 if bc else nn), nc) + sp, dtype)
        go = rnd(rng, (nn, nc) + sp, dtype)
        for (need_I, need_u), dt in itertools.product(needs, dts):
            what = f"{sp} nc={nc} bc={bc} need_I={need_I} need_u={need_u} dt={dt}"
            (dI, du), took = _took(ext, lambda: ext.interp_backward(dev(go), dev(I), dev(u), dt, need_I, need_u))
            assert took == {want_path(nc, need_I, need_u): 1}, (what, took)
            oI, ou = orc.interp_backward(go, I, u, dt, need_I, need_u)
            assert_bits(du, ou, f"d_u ({what})")          # thread-owned: exact
            assert_close(dI, oI, dtype, f"d_I ({what})")  # (summation order of the atomics)


@pytest.mark.parametrize("sp", [(16, 16, 16), (16, 16, 32)])
def test_sheared_window_splat_arms(ext, sp):
    """need_u x unit x bc of splat_shear_kernel and unit x bc of splat_shear_mc_kernel, whose one-pass form serves the
    768-voxel tile and whose two-pass form the 1536-voxel one."""
    _splat_sweep(ext, sp, F32, lambda nc, need_I, need_u: "splat_shear_mc" if nc == 3 and need_u else "splat_shear")


@pytest.mark.parametrize("sp", [(12, 10, 16), (20, 12, 40)])
def test_geometry_once_splat_partial_tiles(ext, sp):
    """splat_shear_mc_kernel (three channels, d_u wanted) on grids that are no multiple of the 8 x 6 x nz tile, so that the
    shared tile decode, window placement and flush meet partial tiles in x and y: 768-voxel tiles in one pass at
    (12, 10, 16); 1920-voxel tiles in two passes at (20, 12, 40), where the window's last z segment is half filled."""
    _splat_sweep(ext, sp, F32, lambda nc, need_I, need_u: "splat_shear_mc", needs=((True, True),), ncs=(3,), dts=(1.0, -0.2))


@pytest.mark.parametrize("nthreads", [1024, 512, 256])
def test_sheared_window_splat_register_forms(ext, nthreads):
    """splat_shear_mc 1: several channels with d_u keep d_u in the registers of splat_shear_kernel over 1, 2 or 4
    passes -- the 768-voxel tile of 16^3 takes 1 pass of 1024 threads, 2 of 512, 3 of 256."""
    with _tuned(ext, splat_shear_mc=1, splat_shear=[1, 8, 6, 0, 1, 1, 4, nthreads]):
        _splat_sweep(ext, (16, 16, 16), F32, lambda nc, need_I, need_u: "splat_shear", needs=((True, True),), ncs=(3,))


@pytest.mark.parametrize("sp,dtype", [((16, 16, 16), F32), ((16, 16, 32), F32), ((16, 16, 16), F64)])
def test_tiled_splat_arms(ext, sp, dtype):
    """Without the sheared window: bc x need_u x unit of the general tiled kernel and, for three channels with d_u in
    float32, unit x bc of its multi-channel form."""
    with _tuned(ext, splat_shear=[0, 8, 6, 0, 1, 1, 4, 1024]):
        _splat_sweep(ext, sp, dtype, lambda nc, need_I, need_u: "splat_tiled")


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9)])
def test_global_atomics_splat_arms(ext, sp, dtype):
    """splat_mode 0: dim x bc x (need_I, need_u) of interp_bwd_kernel; neither needed launches nothing."""
    with _tuned(ext, splat_mode=0):
        _splat_sweep(ext, sp, dtype, lambda nc, need_I, need_u: "splat_global",
                     needs=((True, True), (True, False), (False, True)))
        rng = np.random.default_rng(3)
        go, u = rnd(rng, (2, 1) + sp, dtype), displacement(rng, 2, sp, dtype)
        (dI, du), took = _took(ext, lambda: ext.interp_backward(dev(go), dev(go), dev(u), 1.0, False, False))
        assert took == {} and not dI.any() and not du.any()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_2d_window_splat_arms(ext, dtype):
    _splat_sweep(ext, (128, 128), dtype, lambda nc, need_I, need_u: "splat_2d", ncs=(2,))


@pytest.mark.parametrize("sp,nc,path", [((32, 32, 32), 2, "gather_window"), ((8, 16, 32), 1, "vector_gather"),
                                        ((5, 6, 7), 2, None), ((7, 9), 2, None)])
def test_interp_forward_arms(ext, sp, nc, path):
    """unit x bc of the window and the slab-unrolled kernels, dim x bc of the plain one."""
    nn = 2
    rng = np.random.default_rng(hash(sp) % 2**31)
    u = rnd(rng, (nn, len(sp)) + sp, F32, 0.5) if path else displacement(rng, nn, sp, F32)
    for bc, dt in itertools.product(BOOLS, (1.0, -0.3)):
        I = rnd(rng, ((1 if bc else nn), nc) + sp, F32)
        out, took = _took(ext, lambda: ext.interp_forward(dev(I), dev(u), dt))
        assert took == ({path: 1} if path else {}), (sp, bc, dt, took)
        assert_bits(out, orc.interp_forward(I, u, dt), f"interp_forward {sp} bc={bc} dt={dt}")


@pytest.mark.parametrize("sp,window,path", [((32, 32, 32), 1, "gather_window"), ((32, 32, 32), 0, "vector_gather"),
                                            ((7, 9), 1, None)])
def test_compose_arms(ext, sp, window, path):
    rng = np.random.default_rng(hash(sp) % 2**31)
    u = rnd(rng, (2, len(sp)) + sp, F32, 0.5)
    v = rnd(rng, (2, len(sp)) + sp, F32)
    with _tuned(ext, gather_window=window):
        for ds in (1.0, 0.5):
            out, took = _took(ext, lambda: ext.compose(dev(u), dev(v), ds, -0.1))
            assert took == ({path: 1} if path else {}), (sp, window, ds, took)
            want = np.float32(ds) * u + np.float32(-0.1) * orc.interp_forward(v, u, ds)
            assert_bits(out, want, f"compose {sp} window={window} ds={ds}")


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9)])
@pytest.mark.parametrize("splat_mode", [0, 1])
def test_affine_backward_arms(ext, sp, dtype, splat_mode):
    """The seven non-empty (need_I, need_A, need_T) sets x bc of affine_bwd_kernel.  splat_mode 0 keeps d_I in that
    kernel for 3D too (by default the tiled splat makes d_I and the kernel runs with NEED_I off)."""
    nn, nc, d = 2, 2, len(sp)
    rng = np.random.default_rng(hash((sp, 2)) % 2**31)
    A = (np.eye(d)[None] + 0.3 * rng.standard_normal((nn, d, d))).astype(np.float32 if dtype == F32 else np.float64)
    T = (1.5 * rng.standard_normal((nn, d))).astype(A.dtype)
    go = rnd(rng, (nn, nc) + sp, dtype)
    with _tuned(ext, splat_mode=splat_mode):
        for bc in BOOLS:
            I = rnd(rng, ((1 if bc else nn), nc) + sp, dtype)
            for needs in itertools.product(BOOLS, repeat=3):
                if not any(needs):
                    continue
                got, took = _took(ext, lambda: ext.affine_interp_backward(dev(go), dev(I), dev(A), dev(T), *needs))
                assert took == {}, (sp, needs, took)   # (below the box and window splats: no counted path)
                want = orc.affine_interp_backward(go, I, A, T, *needs)
                for need, g, o, name in zip(needs, got, want, ("d_I", "d_A", "d_T")):
                    if need:
                        assert_close(g, o, dtype, f"affine {name} ({sp} bc={bc} needs={needs})")
                    else:
                        assert g.numel() == 0


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n", [64, 63])
def test_lincomb_arms(ext, n, dtype):
    """K = 1..4 in the vector form (n = 64) and the scalar form (n = 63): bit for bit the left-to-right fma chain."""
    g = torch.Generator(device="cuda").manual_seed(11)
    xs = [torch.randn(n, device="cuda", dtype=dtype, generator=g) for _ in range(4)]
    cs = [1.25, -0.37, 2.5e-3, 11.0]
    for k in range(1, 5):
        want = cs[0] * xs[0]
        for c, x in zip(cs[1:k], xs[1:k]):
            want = torch.add(want, x, alpha=c)
        got = ext.lincomb(list(zip(cs[:k], xs[:k])))
        assert torch.equal(got, want), (k, n, dtype, float((got - want).abs().max()))
