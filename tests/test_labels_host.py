"""CPU: the specification of warp_labels and label_overlap before any GPU run.

- tests/labels_ref.py, the numpy reference: its fma is the correctly rounded one, it gives the known answers (zero and
  integer displacements, half-voxel ties), and its vote is the argmax over labels of a float64 trilinear one-hot;
- lagomorph_amd/csrc/label_vote.hpp, the header the kernels call: tests/native/label_emul.cpp runs every voxel of every
  case through its functions with a plain host compiler, and labels, corners and offsets equal the reference exactly;
  the same program is run once more built with -fsanitize=address,undefined;
- the public surface: names, C symbols, the argument errors (raised on CPU tensors, before any device call) and the
  sizing of label_overlap's scratch."""
import ctypes
import os
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

import labels_ref as ref
import native_build

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = ((5, 6, 7), (7, 9), (8, 16, 32), (1, 5, 4), (6, 1, 3), (2, 2, 2), (1, 9))


# ---- the reference against itself

def test_reference_fma_is_correctly_rounded():
    rng = np.random.default_rng(11)
    n = 4000
    a = np.where(rng.random(n) < 0.5, 0.7, rng.standard_normal(n))
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 10, n)
    b[: n // 2] = b[: n // 2].astype(np.float32)
    c = rng.integers(0, 200, n).astype(np.float64)
    c[::7] = rng.standard_normal(n)[::7]
    # sums that nearly cancel, where the product's tail decides the result
    c[1::5] = -(a * b)[1::5]
    got = ref.fma(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert (got != a * b + c).sum() > 50   # ... and the plain two-rounding expression is a different function
    with np.errstate(invalid="ignore"):
        odd = ref.fma(0.7, np.array([np.nan, np.inf, -np.inf, 3e9, 1e300]), 3.0)
    assert np.isnan(odd[0]) and odd[1] == np.inf and odd[2] == -np.inf and odd[3] == 0.7 * 3e9 + 3.0 and odd[4] == 7e299


@pytest.mark.parametrize("sp", [(5, 6, 7), (7, 9), (1, 5, 4)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_known_answers(sp, dtype):
    N, d = 2, len(sp)
    for kind in ref.LABEL_KINDS:
        L = ref.labels(kind, N, sp)
        zero = np.zeros((N, d) + sp, dtype=dtype)
        for mode in ref.MODES:
            for dt in ref.DTS:
                assert np.array_equal(ref.warp(L, zero, dt, mode), L)
            # an integer shift: the shifted, border-clamped L (dt = -1 shifts the other way)
            for shift in ((2, -1, 3)[:d], (-40, 50, -3)[:d]):
                u = np.broadcast_to(np.array(shift, dtype=dtype).reshape((1, d) + (1,) * d), (N, d) + sp)
                for dt in (1.0, -1.0):
                    idx = np.indices(sp)
                    src = tuple(np.clip(idx[a] + int(dt) * shift[a], 0, sp[a] - 1) for a in range(d))
                    assert np.array_equal(ref.warp(L, u, dt, mode), L[(slice(None), slice(None)) + src]), (kind, mode, shift, dt)
        # half a voxel along the last axis alone: two corners of weight 1/2 each -- the smaller label; nearest: the lower
        u = np.zeros((N, d) + sp, dtype=dtype)
        u[:, d - 1] = 0.5
        nxt = np.take(L, np.minimum(np.arange(sp[-1]) + 1, sp[-1] - 1), axis=-1)
        assert np.array_equal(ref.warp(L, u, 1.0, "vote"), np.minimum(L, nxt)), kind
        assert np.array_equal(ref.warp(L, u, 1.0, "nearest"), L), kind
    # half a voxel along every axis, two labels: all 2^d weights are 2^-d, the label on more corners wins, the smaller
    # one where they share the corners evenly
    L = ref.labels("two", N, sp)
    u = np.full((N, d) + sp, 0.5, dtype=dtype)
    c, w = ref.corners(L, u, 1.0)
    assert np.all(w == 0.5 ** d)
    small = (c == 3).sum(-1)
    want = np.where(2 * small >= 2 ** d, 3, 10)
    assert (2 * small == 2 ** d).sum() >= 4   # exact ties do occur
    assert np.array_equal(ref.warp(L, u, 1.0, "vote")[:, 0], want)


def _onehot_argmax(L, u, K):
    """The route warp_labels replaces: K float64 one-hot volumes, each interpolated multilinearly (nested lerps, clamped
    corners) at x + u, and the argmax.  Returns (label, margin between the two best scores)."""
    N, d, sp = u.shape[0], u.shape[1], u.shape[2:]
    idx = np.indices(sp).astype(np.float64)
    p = [np.clip(idx[a] + u[:, a], 0.0, sp[a] - 1.0) for a in range(d)]
    f = [np.minimum(np.floor(x).astype(np.int64), max(sp[a] - 2, 0)) for a, x in enumerate(p)]
    t = [x - fl for x, fl in zip(p, f)]
    item = np.arange(N).reshape((N,) + (1,) * d)
    val = []
    for k in range(K):
        hot = np.broadcast_to((L[:, 0] == k).astype(np.float64), (N,) + sp)

        def lerp(a, where):
            if a == d:
                return hot[(item,) + tuple(where)]
            lo = lerp(a + 1, where + [f[a]])
            hi = lerp(a + 1, where + [np.minimum(f[a] + 1, sp[a] - 1)])
            return lo + t[a] * (hi - lo)

        val.append(lerp(0, []))
    val = np.stack(val, -1)
    order = np.sort(val, -1)
    return val.argmax(-1), order[..., -1] - order[..., -2]


@pytest.mark.parametrize("sp", [(9, 10, 11), (17, 19)])
def test_vote_is_the_argmax_of_a_trilinear_one_hot(sp):
    N, d = 2, len(sp)
    L = ref.labels("random5", N, sp)
    u = ref.displacement("random", N, sp, np.float64)
    got = ref.warp(L, u, 1.0, "vote")[:, 0]
    want, margin = _onehot_argmax(L, u, 5)
    clear = margin >= 1e-9
    print(f"{sp}: {(~clear).sum()} of {clear.size} voxels excluded as near-ties, {(got != want).sum()} labels differ in all")
    assert (~clear).sum() <= 0.01 * clear.size
    assert np.array_equal(got[clear], want[clear])
    assert (got != np.broadcast_to(L[:, 0], got.shape)).mean() > 0.3   # (the displacement does move labels)


# ---- the header against the reference

def _build_emul(tmp_path, name, extra=()):
    return native_build.build(tmp_path, "label_emul.cpp", extra=extra, name=name)


def _emul_cases():
    """(sp, dtype, NL, L, u, dt): every label kind, displacement kind and dt at every shape in both precisions, with one
    label map per item, and one shape per dimension once more with the map shared."""
    N = 2
    for sp in SHAPES:
        for dtype in (np.float32, np.float64):
            for lk, dk, dt, L, u in ref.warp_cases(N, sp, dtype):
                yield sp, dtype, N, L, u, dt
                if sp in ((5, 6, 7), (7, 9)) and lk in ("random5", "extreme"):
                    yield sp, dtype, 1, L[:1], u, dt


def _write_cases(path, cases):
    with open(path, "wb") as f:
        for sp, dtype, NL, L, u, dt in cases:
            n = tuple(sp) + (1,) * (3 - len(sp))
            f.write(struct.pack("<7id", len(sp), np.dtype(dtype).itemsize, u.shape[0], NL, *n, dt))
            f.write(np.ascontiguousarray(L, dtype="<i4").tobytes())
            f.write(np.ascontiguousarray(u).tobytes())


def _read_results(path, cases):
    raw, at = open(path, "rb").read(), 0
    for sp, dtype, NL, L, u, dt in cases:
        m, d = u.shape[0] * int(np.prod(sp)), len(sp)
        got = []
        for dt_, cnt in (("<i4", m), ("<i4", m), ("<i4", m * d), ("<i4", m * d), ("<f8", m * d)):
            got.append(np.frombuffer(raw, dtype=dt_, count=cnt, offset=at))
            at += cnt * np.dtype(dt_).itemsize
        yield got
    assert at == len(raw)


@native_build.needs_cxx
def test_header_emulation_equals_the_reference_exactly(tmp_path):
    cases = list(_emul_cases())
    assert len(cases) > 1400
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    _write_cases(src, cases)
    native_build.run(_build_emul(tmp_path, "label_emul"), src, dst)
    moved = ties = 0
    for (sp, dtype, NL, L, u, dt), (nearest, vote, lo, hi, t) in zip(cases, _read_results(dst, cases)):
        N, d = u.shape[0], len(sp)
        what = (sp, np.dtype(dtype).name, NL, dt)
        tp = ref.taps(u, dt)
        for k, name in ((lo, 0), (hi, 1)):
            assert np.array_equal(k.reshape((N,) + sp + (d,)), np.stack([x[name] for x in tp], -1)), what
        want_t = np.stack([x[2] for x in tp], -1)
        assert np.array_equal(t.view(np.uint64).reshape(want_t.shape), want_t.view(np.uint64)), what
        assert np.array_equal(nearest.reshape((N, 1) + sp), ref.warp(L, u, dt, "nearest")), what
        want = ref.warp(L, u, dt, "vote")
        assert np.array_equal(vote.reshape((N, 1) + sp), want), what
        moved += int((want != np.broadcast_to(L, want.shape)).sum())
        c, w = ref.corners(L, u, dt)
        s = np.sort(ref.scores(c, w), -1)
        ties += int(((s[..., -1] == 0.5) & (c.min(-1) != c.max(-1))).sum())
    assert moved > 10000 and ties > 500   # the cases do move labels, and exact ties between two labels are among them


@native_build.needs_cxx
def test_header_emulation_under_the_sanitizers(tmp_path):
    """The same stand-alone host program with AddressSanitizer and UndefinedBehaviorSanitizer: the corner indices,
    conversions of out-of-range, infinite and NaN positions included, stay defined and inside the label map."""
    cases = [c for c in _emul_cases() if c[0] in ((5, 6, 7), (7, 9), (1, 5, 4), (2, 2, 2))]
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    _write_cases(src, cases)
    exe = _build_emul(tmp_path, "label_emul_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    native_build.run(exe, src, dst, quiet=True)
    for (sp, dtype, NL, L, u, dt), (nearest, vote, lo, hi, t) in zip(cases, _read_results(dst, cases)):
        assert np.array_equal(vote.reshape((u.shape[0], 1) + sp), ref.warp(L, u, dt, "vote"))


# ---- the public surface

def test_names_symbols_and_abi_version():
    import lagomorph_amd as lm
    from lagomorph_amd import labels, lagomorph_ext as ext

    for name in ("warp_labels", "label_overlap", "dice"):
        assert callable(getattr(lm, name)) and getattr(lm, name) is getattr(labels, name)
        assert getattr(lm, name).__doc__
    assert callable(ext.warp_labels) and callable(ext.label_overlap)
    assert ext.LABEL_MODES == {"nearest": 0, "vote": 1} and ext.LABELS_MAX == 4096
    lib = ctypes.CDLL(ext.LIB_PATH)
    for sym in ("lago_warp_labels_f32", "lago_warp_labels_f64", "lago_label_overlap", "lago_label_overlap_scratch_chunks"):
        assert hasattr(lib, sym), sym
    assert lib.lago_abi_version() == ext.ABI_VERSION == 5
    header = open(os.path.join(os.path.dirname(HERE), "include", "lagomorph_hip.h")).read()
    for text in ("#define LAGO_LABELS_NEAREST 0", "#define LAGO_LABELS_VOTE 1", "#define LAGO_LABELS_MAX 4096",
                 "lago_warp_labels##SUF(", "int lago_label_overlap(", "int lago_label_overlap_scratch_chunks("):
        assert text in header, text
    assert "differentiable" in labels.warp_labels.__doc__
    assert "int32 range" in labels.warp_labels.__doc__


def test_argument_errors_are_raised_on_cpu_tensors():
    import lagomorph_amd as lm

    L = torch.zeros((2, 1, 4, 5, 6), dtype=torch.int32)
    u = torch.zeros((2, 3, 4, 5, 6))
    for mode in ("linear", "", None, 1, "Vote"):
        with pytest.raises(ValueError, match="mode"):
            lm.warp_labels(L, u, mode=mode)
    for bad in (L.float(), L.double(), L.bool()):
        with pytest.raises(RuntimeError, match="integer labels"):
            lm.warp_labels(bad, u)
    for bad in (torch.zeros((2, 2, 4, 5, 6), dtype=torch.int32), torch.zeros((2, 1, 4), dtype=torch.int32),
                torch.zeros((2, 1, 4, 5, 6, 7), dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="label map of shape"):
            lm.warp_labels(bad, u)
    for bad in (u[:, :2], u[..., :5], torch.zeros((2, 2, 5, 6))):
        with pytest.raises(RuntimeError, match="does not match"):
            lm.warp_labels(L, bad)
    with pytest.raises(RuntimeError, match="batch sizes"):
        lm.warp_labels(torch.zeros((3, 1, 4, 5, 6), dtype=torch.int32), u)
    with pytest.raises(RuntimeError, match="batch sizes"):
        lm.warp_labels(L, u[:1])
    with pytest.raises(RuntimeError, match="float32 and float64"):
        lm.warp_labels(L, u.half())
    with pytest.raises(TypeError):
        lm.warp_labels(L.numpy(), u)
    with pytest.raises(TypeError):
        lm.warp_labels(L, u.numpy())
    for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):   # all fine but for the device
        for uu in (u, u.double(), u.requires_grad_(True)):
            with pytest.raises(RuntimeError, match="CUDA tensor"):
                lm.warp_labels(L.to(dt), uu)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            lm.warp_labels(L[:1].to(dt), u, dt=0.7, mode="nearest")

    A = torch.zeros((2, 1, 5, 6), dtype=torch.int64)
    for f in (lm.label_overlap, lm.dice):
        for K in (0, -1, 4097, 2.5, True, None, "7"):
            with pytest.raises(ValueError, match="num_labels"):
                f(A, A, K)
        with pytest.raises(RuntimeError, match="same shape"):
            f(A, A[..., :5], 3)
        with pytest.raises(RuntimeError, match="dtype"):
            f(A, A.int(), 3)
        with pytest.raises(RuntimeError, match="integer labels"):
            f(A.float(), A.float(), 3)
        with pytest.raises(RuntimeError, match="label map of shape"):
            f(A[:, 0], A[:, 0], 3)
        with pytest.raises(TypeError):
            f(A.numpy(), A, 3)
        for K in (1, 200, 4096):
            with pytest.raises(RuntimeError, match="CUDA tensor"):
                f(A, A, K)


def test_c_entry_points_validate_before_any_device_call():
    from lagomorph_amd import lagomorph_ext as ext

    OK, INVALID = 0, -1
    p, q, r = 0x10000, 0x20000, 0x40000   # never dereferenced: every call below returns before a launch
    for suf in ("_f32", "_f64"):
        f = ext._fn["lago_warp_labels" + suf]
        assert f(p, q, r, 1.0, 1, 0, 5, 1, 4, 4, 4, None) == INVALID and b"dimensional" in ext._lib.lago_last_error()
        assert f(p, q, r, 1.0, 1, 0, 1, 1, 4, 4, 4, None) == INVALID
        for mode in (2, -1):
            assert f(p, q, r, 1.0, mode, 0, 3, 1, 4, 4, 4, None) == INVALID and b"mode" in ext._lib.lago_last_error()
        assert f(p, p, r, 1.0, 1, 0, 3, 1, 4, 4, 4, None) == INVALID and b"overlap" in ext._lib.lago_last_error()
        assert f(p, q, p + 16, 1.0, 0, 1, 2, 2, 4, 4, 0, None) == INVALID and b"overlap" in ext._lib.lago_last_error()
        assert f(p, q, r, 1.0, 1, 0, 3, 1, 4, -1, 4, None) == INVALID
        for ext_ in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0)):   # empty: nothing to do
            assert f(None, None, None, 1.0, 1, 0, 3, *ext_, None) == OK
        assert f(None, None, None, 1.0, 0, 0, 2, 1, 4, 0, 0, None) == OK
    g = ext._lib.lago_label_overlap
    for K in (0, -3, 4097):
        assert g(p, q, r, 0x80000, 1, K, 1, 64, None) == INVALID and b"num_labels" in ext._lib.lago_last_error()
    assert g(p, q, r, 0x80000, 1, 3, 1, (1 << 30) + 1, None) == INVALID
    assert g(p, q, r, 0x80000, 0, 3, 1, 64, None) == INVALID and b"scratch" in ext._lib.lago_last_error()
    assert g(p, p, r, 0x80000, 1, 3, 1, 64, None) == INVALID and b"overlap" in ext._lib.lago_last_error()
    assert g(None, None, None, None, 1, 3, 0, 64, None) == OK


def test_scratch_chunks_stay_within_the_cap():
    from lagomorph_amd import lagomorph_ext as ext

    cap = 8 << 20   # bytes: include/lagomorph_hip.h, lago_label_overlap
    for K in (1, 2, 5, 200, 1365, 1366, 4096):
        for rows in (0, 1, 2, 8, 32, 1000):
            for nvox in (0, 1, 63, 210, 16384, 16385, 54120, 128 ** 3, 160 ** 3, 1 << 30):
                c = ext.label_overlap_chunks(K, rows, nvox)
                assert c >= 1
                assert c == 1 or max(rows, 1) * c * K * 3 * 4 <= cap, (K, rows, nvox, c)
                assert c <= max(1, -(-nvox // 16384))
    assert ext.label_overlap_chunks(200, 2, 33 * 40 * 41) >= 2
    assert ext.label_overlap_chunks(4096, 2, 33 * 40 * 41) >= 2
    for bad in ((0, 1, 64), (4097, 1, 64), (3, -1, 64), (3, 1, -1), (3, 1, (1 << 30) + 1)):
        assert ext.label_overlap_chunks(*bad) == 1
