"""GPU: distance_transform, signed_distance and surface_distance against the numpy reference tests/edt_ref.py
(tests/test_edt_host.py ties that reference to the brute-force definition, to scipy and to the header the kernels call).

Which kernel variant a shape takes (csrc/edt.hip: edt_tile -- a pass whose axis has extent n stages tiles of 64 lines for
n <= 256, of 32 for n <= 512 and of 16 above, and a lane holds 8 outputs of a line): every pass of the small shapes
takes the 64-line tile; (8, 16, 32) and (33, 40, 41) straddle the 8 outputs of a lane, the 64 contiguous voxels of a
strided tile and the 64 rows of a first-pass tile, with several workgroups per pass; (300, 5, 6), (5, 300, 6), (5, 6, 300)
and (300, 9) are the smallest listed shapes that take the 32-line tile in the x, y and z (first) pass and in the 2D y
pass, and (513, 3, 4), (3, 513, 4), (3, 4, 513) and (513, 3) the smallest that take the 16-line tile there.  (1, 9),
(1, 5, 4) and (6, 1, 3) have passes over a single voxel; (2, 2, 2) has lines of two."""
import functools

import numpy as np
import pytest
import torch

import edt_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

N = 2
SHAPES = ((5, 6, 7), (7, 9), (1, 9), (1, 5, 4), (6, 1, 3), (2, 2, 2), (8, 16, 32), (33, 40, 41),
          (300, 5, 6), (5, 300, 6), (5, 6, 300), (300, 9), (513, 3, 4), (3, 513, 4), (3, 4, 513), (513, 3))
SPACING = (1.5, 0.7, 2.0)
REL = 8 * 2.0 ** -24   # one rounding for s delta, one for the square, one per addition over three axes (and the
                       # spacing's own rounding to float32): every term is non-negative, so the errors only add


@functools.lru_cache(maxsize=None)
def _labels(kind, sp):
    L = ref.labels(kind, N, sp)
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def _want_sq(kind, sp, where, spacing):
    """float64 squared distances (+inf without a feature), computed once per case and shared."""
    w = ref.as_float(ref.edt_sq(ref.features(_labels(kind, sp), where, 1), spacing))
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("sp", SHAPES, ids=str)
def test_unit_spacing_is_exact(sp):
    import lagomorph_amd as lm

    for kind in ref.KINDS:
        L = _labels(kind, sp)
        Ld = dev(L)
        if kind not in ("none", "all"):
            assert not np.array_equal(L[0], L[1])   # an item-stride error would show
        for where in ref.WHERES:
            want = _want_sq(kind, sp, where, 1.0).astype(np.float32)
            got = lm.distance_transform(Ld, where, 1, squared=True)
            assert got.dtype == torch.float32 and got.shape == (N, 1) + sp and not got.requires_grad
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (kind, where)
            got = lm.distance_transform(Ld, where, 1)
            assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(np.sqrt(want)).view(torch.int32)), (kind, where)
    assert torch.equal(lm.distance_transform(dev(_labels("dense", sp))).cpu(),   # the defaults: L != 0, unit spacing, the root
                       torch.from_numpy(np.sqrt(_want_sq("dense", sp, "nonzero", 1.0).astype(np.float32))))


@pytest.mark.parametrize("sp", SHAPES, ids=str)
def test_anisotropic_spacing_is_within_the_derived_bound(sp):
    import lagomorph_amd as lm

    s = SPACING[-len(sp):]
    worst = 0.0
    for kind in ref.KINDS:
        Ld = dev(_labels(kind, sp))
        for where in ref.WHERES:
            want = _want_sq(kind, sp, where, s)
            got = lm.distance_transform(Ld, where, 1, s, squared=True).cpu().numpy().astype(np.float64)
            assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isnan(got).any(), (kind, where)
            fin = np.isfinite(want) & (want > 0)
            assert np.all(got[want == 0] == 0)
            err = np.abs(got[fin] - want[fin]) / want[fin]
            worst = max(worst, float(err.max()) if err.size else 0.0)
            assert np.all(err <= REL), (kind, where, err.max())
            root = lm.distance_transform(Ld, where, 1, s).cpu().numpy()
            assert np.array_equal(root.view(np.uint32), np.sqrt(got.astype(np.float32)).view(np.uint32)), (kind, where)
    print(f"{sp}: largest relative error {worst / 2.0 ** -24:.2f} * 2^-24 (bound 8)")
    # one spacing for all axes is that spacing on every axis
    Ld = dev(_labels("sparse", sp))
    assert torch.equal(lm.distance_transform(Ld, spacing=0.7), lm.distance_transform(Ld, spacing=(0.7,) * len(sp)))


def test_dtypes_layout_determinism_and_limits():
    import lagomorph_amd as lm

    sp = (5, 6, 7)
    L = _labels("dense", sp)   # labels 0, 1, 2
    Ld = dev(L).requires_grad_(False)
    want = lm.distance_transform(Ld, "equal", 1)
    assert want.dtype == torch.float32 and want.grad_fn is None and not want.requires_grad
    for dt in (torch.uint8, torch.int16, torch.int64):
        for where in ref.WHERES:
            assert torch.equal(lm.distance_transform(Ld.to(dt), where, 1), lm.distance_transform(Ld, where, 1)), (dt, where)
    assert torch.equal(lm.distance_transform(Ld != 0), lm.distance_transform(Ld))
    assert torch.equal(lm.distance_transform(Ld == 1, "equal", 1), want)
    assert torch.equal(lm.distance_transform(Ld == 1, "surface", 1), lm.distance_transform(Ld, "surface", 1))
    # negative labels are values like any other
    assert torch.equal(lm.distance_transform(Ld - 2, "surface", -1), lm.distance_transform(Ld, "surface", 1))
    for _ in range(2):   # determinism
        assert torch.equal(lm.distance_transform(Ld, "equal", 1), want)
    with pytest.raises(RuntimeError, match="contiguous"):
        lm.distance_transform(Ld.transpose(2, 3))
    for big in ((1025, 2, 2), (2, 2, 1025), (2, 1025)):
        with pytest.raises(RuntimeError, match="extents up to 1024"):
            lm.distance_transform(torch.zeros((1, 1) + big, dtype=torch.uint8, device="cuda"))
    assert lm.distance_transform(torch.zeros((0, 1, 4, 5), dtype=torch.int32, device="cuda")).shape == (0, 1, 4, 5)


def test_largest_extent():
    """Extent 1024, the 16-line tile at its full 64 KB, in the first pass and in a strided one."""
    import lagomorph_amd as lm

    for sp in ((3, 1024), (1024, 3)):
        L = np.zeros((N, 1) + sp, dtype=np.int32)
        L[0, 0, 0, 0] = L[1, 0, -1, -1] = 1
        grid = np.indices(sp)
        want = np.stack([grid[0] ** 2 + grid[1] ** 2, (grid[0] - sp[0] + 1) ** 2 + (grid[1] - sp[1] + 1) ** 2])[:, None]
        assert torch.equal(lm.distance_transform(dev(L), squared=True).cpu(), torch.from_numpy(want.astype(np.float32)))


def test_signed_distance():
    import lagomorph_amd as lm

    sp = (9, 10, 11)
    L = _labels("blobs", sp)
    Ld = dev(L)
    for label, s in ((2, 1.0), (None, 1.0), (1, SPACING)):
        got = lm.signed_distance(Ld, label, s)
        assert got.dtype == torch.float32 and got.shape == L.shape
        want = ref.signed_distance(L, label, s)
        assert np.allclose(got.cpu().numpy(), want, rtol=1e-6, atol=0), (label, s)
        m = (L != 0) if label is None else (L == label)
        assert np.array_equal(got.cpu().numpy() < 0, m) and not (got == 0).any()
        if s == 1.0:   # one of the two roots is 0 at every voxel: the float32 roots themselves, signed
            w = "nonzero" if label is None else "equal"
            out = ref.distance_transform(L, w, label or 0)
            ins = ref.distance_transform(~m, "nonzero")
            assert torch.equal(got.cpu(), torch.from_numpy(out - ins))
    # the sign convention on a box: negative inside, positive outside, +-1 across a face
    B = np.concatenate([ref.box((9, 9), (3, 3), (6, 6), 4), ref.box((9, 9), (2, 3), (5, 6), 4)])
    sd = lm.signed_distance(dev(B), 4).cpu().numpy()
    assert sd[0, 0, 4, 4] == -2 and sd[0, 0, 3, 4] == -1 and sd[0, 0, 2, 4] == 1 and sd[0, 0, 0, 0] == np.float32(np.sqrt(18.0))
    assert sd[1, 0, 3, 4] == -2 and sd[1, 0, 1, 4] == 1
    # an empty side is the other side's infinity
    assert torch.all(lm.signed_distance(dev(B), 7) == float("inf")) and torch.all(lm.signed_distance(dev(B * 0 + 7), 7) == -float("inf"))


def _check_surface(got, want, rel=1e-6):
    assert set(got) == {"hausdorff", "hd95", "assd"}
    for k, w in want.items():
        g = got[k]
        assert g.dtype == torch.float64 and g.is_cuda and tuple(g.shape) == w.shape
        g = g.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(w)), (k, g, w)
        ok = ~np.isnan(w)
        assert np.all(np.abs(g[ok] - w[ok]) <= rel * np.abs(w[ok])), (k, g, w)


@pytest.mark.parametrize("sp", [(12, 13, 14), (20, 23)], ids=str)
def test_surface_distance_on_blobs(sp):
    import lagomorph_amd as lm

    A = ref.labels("blobs", N, sp, seed=1)
    B = ref.labels("blobs", N, sp, seed=2)
    B = np.where(B == 3, 0, B)                               # label 3 is absent from B: nan
    B = np.where(A == 2, 2, np.where(B == 2, 0, B)).astype(np.int32)   # label 2 is the same structure in both: 0
    labels = [1, 2, 3]
    for s in (1.0, SPACING[-len(sp):]):
        want = ref.surface_distance(A, B, labels, s)
        assert np.isfinite(want["hausdorff"][:, 0]).all() and (want["assd"][:, 0] > 0).all()
        assert np.isnan(want["hd95"][:, 2]).all()
        got = lm.surface_distance(dev(A), dev(B), labels, s)
        _check_surface(got, want)
        for k in got:
            assert torch.all(got[k][:, 1] == 0), k
    # the selection mask is the kernel's own predicate
    assert torch.equal(lm.surface_mask(dev(A), 1).cpu(), torch.from_numpy(ref.surface(A == 1)))


@pytest.mark.parametrize("d", [2, 3])
def test_surface_distance_on_the_closed_form_boxes(d):
    import lagomorph_amd as lm

    A, B, hausdorff, assd = ref.concentric_boxes(d)
    A2, B2 = np.concatenate([A, B]), np.concatenate([B, A])   # the second item the other way round: symmetric
    got = lm.surface_distance(dev(A2), dev(B2), [1])
    for n in range(2):
        assert abs(got["hausdorff"][n, 0].item() - hausdorff) <= 1e-6 * hausdorff
        assert abs(got["assd"][n, 0].item() - assd) <= 1e-6 * assd
    _check_surface(got, ref.surface_distance(A2, B2, [1]))


def test_other_stream_gives_the_same_bits():
    import lagomorph_amd as lm

    sp = (33, 40, 41)
    Ld = dev(_labels("blobs", sp))
    want = [lm.distance_transform(Ld, w, 1, SPACING) for w in ref.WHERES]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = [lm.distance_transform(Ld, w, 1, SPACING) for w in ref.WHERES]
    side.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)
