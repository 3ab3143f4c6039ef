"""GPU: warp_labels and label_overlap against the numpy reference tests/labels_ref.py, label for label and count for
count (tests/test_labels_host.py ties that reference to known answers and to the header the kernels call).

Which kernel a shape takes (csrc/labels.hip, launch.hpp: slab_grid -- nz >= 2, 256 / nz + 1 < ny, at least 2048 voxels):
(8, 16, 32) is the smallest power-of-two volume of the slab-unrolled 3D kernel (checked with path_launches); (5, 6, 7) and
the thin 3D volumes take the plain 3D kernel, (7, 9) and (1, 9) the 2D one.  (1, 5, 4) and (6, 1, 3) have extents of one
voxel, (2, 2, 2) rows of two, where the (z, z + 1) pair of a corner row is the whole row, and (1, 9) is a single row."""
import numpy as np
import pytest
import torch

import labels_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

N = 2
WARP_SHAPES = ((5, 6, 7), (7, 9), (8, 16, 32), (1, 5, 4), (6, 1, 3), (2, 2, 2), (1, 9))
OVERLAP_SHAPES = ((5, 6, 7), (33, 40, 41), (7, 9))
KS = (1, 2, 5, 200, 4096)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("sp", WARP_SHAPES, ids=str)
def test_warp_labels_equals_the_reference(sp, dtype):
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    slab = sp == (8, 16, 32)
    calls = 0
    before = ext.path_launches("vector_gather")
    for lk, dk, dt, L, u in ref.warp_cases(N, sp, dtype):
        ud = dev(u)
        for bc in (False, True):
            Lh = L[:1] if bc else L
            Ld = dev(Lh)
            for mode in ref.MODES:
                got = lm.warp_labels(Ld, ud, dt, mode)
                calls += 1
                assert got.dtype == torch.int32 and got.shape == (N, 1) + sp and not got.requires_grad
                assert torch.equal(got.cpu(), torch.from_numpy(ref.warp(Lh, u, dt, mode))), (lk, dk, dt, bc, mode)
    assert calls == 2 * 2 * len(ref.LABEL_KINDS) * len(ref.DISP_KINDS) * len(ref.DTS)
    assert ext.path_launches("vector_gather") - before == (calls if slab else 0)


def test_warp_labels_dtypes_defaults_and_no_graph():
    import lagomorph_amd as lm

    sp = (5, 6, 7)
    L = ref.labels("random5", N, sp)
    u = ref.displacement("random", N, sp, np.float32)
    ud = dev(u).requires_grad_(True)
    want = lm.warp_labels(dev(L), ud)
    assert torch.equal(want.cpu(), torch.from_numpy(ref.warp(L, u, 1.0, "vote")))   # the defaults: dt = 1, vote
    assert not want.requires_grad and want.grad_fn is None and want.dtype == torch.int32
    for dt in (torch.uint8, torch.int16, torch.int64):
        got = lm.warp_labels(dev(L).to(dt), ud, mode="vote")
        assert got.dtype == dt and torch.equal(got.to(torch.int32), want) and not got.requires_grad
    # label values of the whole int32 range survive the int64 round trip
    Lx = ref.labels("extreme", N, sp)
    got = lm.warp_labels(dev(Lx).to(torch.int64), ud)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(ref.warp(Lx, u, 1.0, "vote")).to(torch.int64))
    # determinism
    assert torch.equal(lm.warp_labels(dev(L), ud), want)
    with pytest.raises(RuntimeError, match="contiguous"):
        lm.warp_labels(dev(L).transpose(2, 3), dev(u).transpose(2, 3))


def _overlap_inputs(sp, K):
    """(name, A, B) int32 (N, 1, *sp)."""
    rng = np.random.default_rng([K, *sp])
    zero = np.zeros((N, 1) + sp, dtype=np.int32)
    yield "zeros", zero, zero.copy()
    hi = min(K, 300)
    yield "random", rng.integers(0, hi, zero.shape).astype(np.int32), rng.integers(0, hi, zero.shape).astype(np.int32)
    nb = max(2, min(K, 6))
    A = ref.blobs(rng, N, sp, nb)
    B = np.where(rng.random(A.shape) < 0.1, rng.integers(0, nb, A.shape), A).astype(np.int32)   # A with 10 % of it relabelled
    yield "blobs", A, B
    out = rng.integers(-3, K + 3, zero.shape).astype(np.int32)   # some labels negative or >= K
    out.reshape(-1)[:3] = (-2 ** 31, 2 ** 31 - 1, K)
    yield "outside", out, np.roll(out, 1, -1)
    yield "same", A, A


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("sp", OVERLAP_SHAPES, ids=str)
def test_label_overlap_equals_bincount(sp, K):
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    nvox = int(np.prod(sp))
    chunks = ext.label_overlap_chunks(K, N, nvox)
    print(f"{sp} K={K}: {chunks} workgroups (partial tables) a row")
    if sp == (33, 40, 41):
        assert chunks >= 2          # 54 120 voxels: a row is shared by several workgroups
    for name, A, B in _overlap_inputs(sp, K):
        Ad = dev(A)
        Bd = Ad if name == "same" else dev(B)
        got = lm.label_overlap(Ad, Bd, K)
        assert got.dtype == torch.int64 and got.shape == (N, K, 3)
        want = ref.overlap(A, B, K)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), name
        assert torch.equal(lm.label_overlap(Ad, Bd, K), got), name   # determinism
        # dice: plain float64 arithmetic on the table
        for empty in (float("nan"), -1.0):
            d = lm.dice(Ad, Bd, K, empty=empty)
            assert d.dtype == torch.float64 and d.shape == (N, K)
            assert np.array_equal(d.cpu().numpy(), ref.dice(want, empty), equal_nan=True), name
        occurs = torch.from_numpy(want[..., 0] + want[..., 1] > 0)
        d = lm.dice(Ad, Bd, K, empty=-1.0).cpu()
        assert bool((d[~occurs] == -1.0).all()) and bool((d[occurs] >= 0).all())
        if name == "same":
            assert occurs.any() and bool((d[occurs] == 1.0).all())


@pytest.mark.parametrize("offs", [(1, 1), (3, 3), (1, 2), (0, 3)])
def test_label_overlap_at_odd_pointer_offsets(offs):
    """Label maps that start 1 .. 3 elements past a 16-byte boundary: equal offsets run the scalar head, the vectors and
    the scalar tail; different ones leave no common vector boundary, every voxel is then read as a scalar."""
    import lagomorph_amd as lm

    K, rng = 5, np.random.default_rng(5)
    for sp in ((5, 6, 7), (33, 40, 41), (7, 9)):
        n = N * int(np.prod(sp))
        A, B = rng.integers(-1, K + 1, n).astype(np.int32), rng.integers(-1, K + 1, n).astype(np.int32)
        views = []
        for x, o in ((A, offs[0]), (B, offs[1])):
            buf = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
            assert buf.data_ptr() % 16 == 0
            v = buf[o:o + n].view((N, 1) + sp)
            v.copy_(torch.from_numpy(x).view((N, 1) + sp))
            assert v.is_contiguous() and v.data_ptr() % 16 == 4 * o
            views.append(v)
        got = lm.label_overlap(views[0], views[1], K)
        assert torch.equal(got.cpu(), torch.from_numpy(ref.overlap(A.reshape((N, 1) + sp), B.reshape((N, 1) + sp), K))), sp


def _overlap_with_scratch(A, B, K, chunks):
    """lago_label_overlap with a scratch of `chunks` partial tables a row, as lagomorph_ext.label_overlap calls it."""
    from lagomorph_amd import lagomorph_ext as ext

    rows, nvox = A.size(0), A[0].numel()
    counts = torch.full((rows, K, 3), -1, dtype=torch.int64, device=A.device)
    scratch = torch.empty((rows * chunks * K * 3,), dtype=torch.int32, device=A.device)
    ext._launch(ext._lib.lago_label_overlap, A, ext._ptr(counts), ext._ptr(A), ext._ptr(B), ext._ptr(scratch), chunks, K, rows, nvox)
    return counts


@pytest.mark.parametrize("K", [5, 200, 4096])
@pytest.mark.parametrize("sp", [(27, 25, 25), (131, 127)], ids=str)
def test_two_ragged_chunks_a_row_equal_one_chunk_a_row(sp, K):
    """16875 voxels are chunks of 8440 + 8435, 16637 of 8320 + 8317 (csrc/chunk_table.hpp); the rows are odd, so rows 1
    and 2 start off the 16-byte boundary.  Labels outside [0, K) and negative ones among them.  The counts equal the
    reference, and so does the same call with a scratch of ONE table a row (one workgroup walks the row)."""
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    rows, nvox = 3, int(np.prod(sp))
    assert nvox % 2 == 1 and ext.label_overlap_chunks(K, rows, nvox) == 2
    rng = np.random.default_rng([K, *sp])
    A = rng.integers(-3, K + 3, (rows, 1) + sp).astype(np.int32)
    B = np.where(rng.random(A.shape) < 0.5, A, rng.integers(-3, K + 3, A.shape)).astype(np.int32)
    A.reshape(-1)[:3] = (-2 ** 31, 2 ** 31 - 1, K)
    Ad, Bd = dev(A), dev(B)
    got = lm.label_overlap(Ad, Bd, K)
    assert torch.equal(got.cpu(), torch.from_numpy(ref.overlap(A, B, K)))
    assert torch.equal(_overlap_with_scratch(Ad, Bd, K, 1), got)


@pytest.mark.parametrize("sp", [(1, 1), (1, 5), (3, 3, 3), (1, 259)], ids=str)
def test_label_overlap_of_the_smallest_rows(sp):
    """Rows below one vector, below one workgroup of lanes, and of a vector count that is no multiple of 256 with a tail:
    every lane takes part in the wave's ballots whether it holds a voxel or not."""
    import lagomorph_amd as lm

    K, rng = 3, np.random.default_rng([3, *sp])
    A, B = (rng.integers(-1, K + 1, (N, 1) + sp).astype(np.int32) for _ in range(2))
    assert torch.equal(lm.label_overlap(dev(A), dev(B), K).cpu(), torch.from_numpy(ref.overlap(A, B, K)))


def test_label_overlap_dtypes():
    import lagomorph_amd as lm

    sp, K = (5, 6, 7), 5
    A, B = ref.labels("random5", N, sp), ref.labels("blobs", N, sp)
    want = torch.from_numpy(ref.overlap(A, B, K))
    for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):
        assert torch.equal(lm.label_overlap(dev(A).to(dt), dev(B).to(dt), K).cpu(), want)


def test_warp_back_reproduces_the_labels_and_dice_is_one():
    """Blobs that keep four voxels clear of the border, shifted by an integer displacement s and warped back with -s:
    away from the border the labels are reproduced exactly, and Dice is 1 on every structure that does not touch it."""
    import lagomorph_amd as lm

    sp, K, s = (14, 15, 16), 6, (2.0, -1.0, 3.0)
    rng = np.random.default_rng(3)
    L = np.zeros((N, 1) + sp, dtype=np.int32)
    inner = (slice(None), slice(None)) + (slice(4, -4),) * 3
    L[inner] = ref.blobs(rng, N, sp, K)[inner]
    inside = torch.tensor([[k > 0 and bool((L[n] == k).any()) for k in range(K)] for n in range(N)])   # (N, K): the blobs
    assert int(inside.sum()) >= 6
    u = np.broadcast_to(np.array(s, dtype=np.float32).reshape(1, 3, 1, 1, 1), (N, 3) + sp)
    Ld, ud = dev(L), dev(u)
    for mode in ref.MODES:
        moved = lm.warp_labels(Ld, ud, 1.0, mode)
        assert not torch.equal(moved, Ld)
        back = lm.warp_labels(moved, ud, -1.0, mode)
        assert torch.equal(back[inner], Ld[inner])
        d = lm.dice(back, Ld, K).cpu()
        assert bool((d[inside] == 1.0).all())
        assert bool((lm.dice(moved, Ld, K).cpu()[inside] < 1.0).all())


def test_both_operators_capture_in_a_graph():
    """One capture of warp_labels followed by label_overlap, no parallel branch: neither call synchronises with the host
    (a synchronisation fails the capture), and the replay gives the eager result, for new contents of the inputs too."""
    import lagomorph_amd as lm

    sp, K = (8, 16, 32), 6
    L = dev(ref.labels("blobs", N, sp))
    u = dev(ref.displacement("random", N, sp, np.float32))

    def fn():
        w = lm.warp_labels(L, u)
        return w, lm.label_overlap(w, L, K)

    want = [x.clone() for x in fn()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    u.copy_(dev(ref.displacement("half", N, sp, np.float32)))
    want2 = [x.clone() for x in fn()]
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], want2[0]) and torch.equal(out[1], want2[1]) and not torch.equal(want2[0], want[0])
    del graph
