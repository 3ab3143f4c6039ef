"""CPU: the specification of the image pyramid (pyramid_reduce, pyramid_expand and their transposes) before any GPU run.

- tests/pyramid_ref.py, the numpy reference, against torch on the CPU in float64 (R: replicate pad and a strided
  convolution with the binomial kernel; E: F.interpolate with align_corners=True on all-odd extents) and against known
  answers: constants, linear ramps, the band claims, the transposes as dense matrices transposed;
- lagomorph_amd/csrc/pyramid_weights.hpp, the header the kernels call: tests/native/pyramid_emul.cpp runs it with a
  plain host compiler; its entries equal the reference's matrices exactly for n in 1..40, its float32 output equals
  the float32 numpy restatement of the header's order bit for bit, its float64 output the reference at 1e-12; the
  same program once more under -fsanitize=address,undefined (stand-alone, nothing preloaded);
- the rounding bound of the GPU test without the kernel: the float32 restatement stays inside it;
- the public surface: names, C symbols, header text, every argument error and the order of the checks (raised on CPU
  tensors, ending in "must be a CUDA tensor"), the C entry points' validation with pointers that are never
  dereferenced, and the argument rules of pyramid_shape and image_pyramid."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import native_build
import pyramid_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_SHAPES = ((1, 1, 1), (2, 3, 1), (5, 4, 7), (9, 17, 33), (6, 1, 12), (1, 1), (2, 3), (6, 7), (33, 20), (1, 9))
ops = pytest.mark.parametrize("op", ref.OPS)


# ---- the reference against torch

@pytest.mark.parametrize("shape", HOST_SHAPES, ids=str)
def test_reduce_is_a_strided_binomial_convolution_of_the_replicate_padded_field(shape):
    d = len(shape)
    a = ref.real_field(2, 3, shape, np.float64, seed=1)
    w1 = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=torch.float64) / 16
    w = w1
    for _ in range(d - 1):
        w = w[..., None] * w1
    t = torch.from_numpy(a).reshape((6, 1) + shape)
    for ax in range(d):   # (replicate padding, one axis at a time: F.pad's replicate mode wants a pad below the extent)
        lo, hi = t.narrow(2 + ax, 0, 1), t.narrow(2 + ax, t.size(2 + ax) - 1, 1)
        t = torch.cat([lo, lo, t, hi, hi], dim=2 + ax)
    got = (F.conv3d if d == 3 else F.conv2d)(t, w[None, None], stride=2).reshape((2, 3) + ref.coarse_shape(shape))
    assert np.abs(got.numpy() - ref.reference("reduce", a, shape)).max() <= 1e-15


@pytest.mark.parametrize("shape", ((1, 1, 1), (3, 5, 7), (9, 17, 33), (1, 5, 3), (1, 1), (3, 5), (33, 21)), ids=str)
def test_expand_is_align_corners_interpolation_on_odd_extents(shape):
    c = ref.real_field(2, 2, ref.coarse_shape(shape), np.float64, seed=2)
    got = F.interpolate(torch.from_numpy(c), size=shape, mode="trilinear" if len(shape) == 3 else "bilinear", align_corners=True)
    assert np.abs(got.numpy() - ref.reference("expand", c, shape)).max() <= 1e-15


# ---- known answers

def test_band_and_row_sum_claims():
    for n in range(1, 66):
        m = (n + 1) // 2
        R, E = ref.reduce_matrix(n), ref.expand_matrix(n)
        assert R.shape == (m, n) and E.shape == (n, m)
        assert (R.sum(1) == 1).all() and (E.sum(1) == 1).all() and (R >= 0).all() and (E >= 0).all()
        assert (R * 16 == np.round(R * 16)).all() and (E * 2 == np.round(E * 2)).all()
        j, x = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
        assert (R[np.abs(2 * j - x) > 2] == 0).all() and (E.T[np.abs(x - 2 * j) > 1] == 0).all()
        assert ((R != 0).sum(0) <= 3).all()
        for jj in range(m):   # the definition, as a gather
            a = np.random.default_rng(n).random(n)
            assert abs(R[jj] @ a - sum(w * a[min(max(2 * jj + k, 0), n - 1)] for k, w in zip(range(-2, 3), (1, 4, 6, 4, 1))) / 16) <= 1e-15
    assert not np.array_equal(2 * ref.reduce_matrix(8).T, ref.expand_matrix(8))   # 2 R^T is not E


@pytest.mark.parametrize("shape", HOST_SHAPES + ref.CASES[3:5], ids=str)
def test_constants_and_ramps(shape):
    d, cs = len(shape), ref.coarse_shape(shape)
    assert (ref.reference("reduce", np.full((1, 1) + shape, 3.25), shape) == 3.25).all()
    assert (ref.reference("expand", np.full((1, 1) + cs, 3.25), shape, scale=2.0) == 6.5).all()
    for dtype in (np.float32, np.float64):
        assert (ref.native("reduce", np.full((1, 1) + shape, 3.25, dtype), shape) == 3.25).all()
        assert (ref.native("expand", np.full((1, 1) + cs, 3.25, dtype), shape, 2.0) == 6.5).all()
    coef = (3.0, -2.0, 5.0)[:d]
    fine = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    coarse = np.meshgrid(*[2.0 * np.arange(m) for m in cs], indexing="ij")   # coarse voxel j sits at fine voxel 2 j
    ramp_f = (sum(c * g for c, g in zip(coef, fine)) + 7.0)[None, None]
    ramp_c = (sum(c * g for c, g in zip(coef, coarse)) + 7.0)[None, None]
    got = ref.reference("reduce", ramp_f, shape)
    inner = tuple(slice(1, max(1, (n - 3) // 2 + 1)) for n in shape)   # 2 j - 2 >= 0 and 2 j + 2 <= n - 1
    assert (got[(0, 0) + inner] == ramp_c[(0, 0) + inner]).all()
    got = ref.reference("expand", ramp_c, shape)
    inner = tuple(slice(0, 2 * m - 1) for m in cs)   # every fine voxel up to the last coarse one: the clamp acts beyond it
    assert (got[(0, 0) + inner] == ramp_f[(0, 0) + inner]).all()


@pytest.mark.parametrize("shape", ((5, 4, 7), (2, 3, 1), (6, 7), (1, 1)), ids=str)
def test_transposes_are_the_dense_matrices_transposed(shape):
    for base in ("reduce", "expand"):
        dense = np.ones((1, 1))
        for n in shape:
            dense = np.kron(dense, ref.axis_matrix(base, n))
        b = ref.real_field(1, 1, ref.out_shape(base, shape), np.float64, seed=5)
        want = (dense.T @ b.reshape(-1)).reshape(ref.in_shape(base, shape))
        got = ref.reference(base + "_adjoint", b, shape)[0, 0]
        assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()   # (two float64 summation orders of up to 125 terms)
        a = ref.real_field(1, 1, ref.in_shape(base, shape), np.float64, seed=6)
        lhs, rhs = (ref.reference(base, a, shape) * b).sum(), (a * ref.reference(base + "_adjoint", b, shape)).sum()
        assert abs(lhs - rhs) <= 5e-16 * max(abs(lhs), 1.0) * 4


# ---- the header, emulated on the host

def _cases():
    out = []
    for shape in HOST_SHAPES:
        for o, op in enumerate(ref.OPS):
            for dtype in (np.float32, np.float64):
                scale = 1.0 if op.startswith("reduce") else 1.7
                out.append((o, shape, dtype, scale, ref.real_field(1, 1, ref.in_shape(op, shape), dtype, seed=len(out)) - dtype(0.25)))
    return out


def _run_emul(tmp_path, name, cases, extra=()):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for o, shape, dtype, scale, a in cases:
            f.write(struct.pack("<5id", o, *((1,) * (3 - len(shape)) + tuple(shape)), np.dtype(dtype).itemsize, scale))
            f.write(a.tobytes())
    exe = native_build.build(tmp_path, "pyramid_emul.cpp", extra=extra, name=name)
    native_build.run(exe, src, dst, quiet=True)
    ent = str(tmp_path / "entries.bin")
    native_build.run(exe, "entries", ent, quiet=True)
    return open(dst, "rb").read(), np.fromfile(ent, dtype=np.float64)


def _check_emul(raw, entries, cases):
    at = 0
    for n in range(1, 41):   # the header's entries are the reference's matrices, exactly
        m = (n + 1) // 2
        assert np.array_equal(entries[at:at + m * n].reshape(m, n), ref.reduce_matrix(n)), n
        assert np.array_equal(entries[at + m * n:at + 2 * m * n].reshape(n, m), ref.expand_matrix(n)), n
        at += 2 * m * n
    assert at == entries.size
    at = 0
    for o, shape, dtype, scale, a in cases:
        op = ref.OPS[o]
        oshape = (1, 1) + ref.out_shape(op, shape)
        count = int(np.prod(oshape))
        got = np.frombuffer(raw, dtype=dtype, count=count, offset=at).reshape(oshape)
        at += count * np.dtype(dtype).itemsize
        want = ref.native(op, a, shape, scale)
        assert want.dtype == dtype
        assert np.array_equal(got, want), (op, shape, dtype, float(np.abs(got - want).max()))
        if dtype is np.float64:
            exact = ref.reference(op, a, shape, scale)
            assert np.abs(got - exact).max() <= 1e-12 * max(np.abs(exact).max(), 1e-300), (op, shape)
    assert at == len(raw)


@native_build.needs_cxx
def test_header_emulation_equals_the_reference(tmp_path):
    cases = _cases()
    _check_emul(*_run_emul(tmp_path, "pyramid_emul", cases), cases)


@native_build.needs_cxx
def test_header_emulation_under_the_sanitizers(tmp_path):
    """The same stand-alone host program with AddressSanitizer and UndefinedBehaviorSanitizer."""
    cases = _cases()
    _check_emul(*_run_emul(tmp_path, "pyramid_emul_san", cases, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")), cases)


# ---- the bound, without the kernel

def test_the_headers_rounding_count():
    for d in (2, 3):
        assert ref.header_roundings(d) == 5 * d + 1 <= 6 * d + 2


@ops
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=str)
def test_float32_restatement_stays_inside_the_bound(shape, op):
    K, u = ref.header_roundings(len(shape)), 2.0 ** -24
    worst = 0.0
    for scale in (1.0, 2.0, 0.3):
        a = ref.real_field(2, 3, ref.in_shape(op, shape), np.float32, seed=7)
        got = ref.native(op, a, shape, scale).astype(np.float64)
        want, bound = ref.reference(op, a, shape, np.float32(scale)), K * u * ref.abs_reference(op, a, shape, np.float32(scale))
        assert (np.abs(got - want) <= bound).all()
        worst = max(worst, float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()))
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    print(f"{shape} {op}: float32 restatement at most {worst:.3f} of the bound")


def test_integer_inputs_are_exact_in_float32():
    for shape in ((5, 4, 7), (9, 17, 33), (33, 20)):
        for op in ref.OPS:
            for scale in (1.0, 2.0):
                a = ref.integer_field(2, 2, ref.in_shape(op, shape), np.float32, seed=3)
                assert np.array_equal(ref.native(op, a, shape, scale).astype(np.float64), ref.reference(op, a, shape, scale)), (op, shape)


# ---- the public surface

def test_names_symbols_and_abi_version():
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext, pyramid

    for name in pyramid.__all__:
        assert getattr(lm, name) is getattr(pyramid, name) and getattr(lm, name).__doc__, name
    assert "pyramid_expand(u, " in pyramid.__doc__ and "scale=2.0" in pyramid.__doc__
    lib = ctypes.CDLL(ext.LIB_PATH)
    for stem in ("lago_pyramid_down", "lago_pyramid_up"):
        for suf in ("_f32", "_f64"):
            assert hasattr(lib, stem + suf) and stem + suf in ext._fn, stem + suf
    assert lib.lago_abi_version() == ext.ABI_VERSION == 5
    header = open(os.path.join(os.path.dirname(HERE), "include", "lagomorph_hip.h")).read()
    block = header[header.index("#define LAGO_DECLARE(REAL, SUF)"):header.index("LAGO_DECLARE(float, _f32)")]
    for text in ("lago_pyramid_down##SUF(", "lago_pyramid_up##SUF("):
        assert text in block, text
    for text in ("#define LAGO_ABI_VERSION 5", "#define LAGO_PYRAMID_REDUCE 0", "#define LAGO_PYRAMID_EXPAND 1"):
        assert text in header and text not in block, text
    assert (pyramid.PYRAMID_REDUCE, pyramid.PYRAMID_EXPAND) == (0, 1)
    public = {n for n, f in vars(ext).items() if callable(f) and getattr(f, "__module__", None) == ext.__name__ and not n.startswith("_")}
    assert not {n for n in public if "pyramid" in n}   # the shim gained no public function: the binding is pyramid.py's
    for doc in (pyramid.__doc__, header[header.index("lago_pyramid_down:"):]):
        assert "call to call" in doc


def test_argument_errors_and_their_order_on_cpu_tensors():
    import lagomorph_amd as lm

    x3, x2 = torch.zeros((2, 3, 5, 6, 7)), torch.zeros((2, 1, 9, 11))
    c3, c2 = torch.zeros((2, 3, 3, 3, 4)), torch.zeros((2, 1, 5, 6))
    down = ((lambda x, **k: lm.pyramid_reduce(x, **k)), (lambda x, **k: lm.pyramid_expand_adjoint(x, **k)))
    up = ((lambda c, s, **k: lm.pyramid_restrict_adjoint(c, s, **k)), (lambda c, s, **k: lm.pyramid_expand(c, s, **k)))
    strided = lambda t: t.transpose(2, 3).contiguous().transpose(2, 3)   # noqa: E731
    for f, args in [(f, ()) for f in down] + [(f, ((5, 6, 7),)) for f in up]:
        good = c3 if args else x3
        for bad in (good.numpy(), None, [1.0]):
            with pytest.raises(TypeError, match="must be a torch.Tensor"):
                f(bad, *args)
        for bad in (good.half(), good.int(), good.long()):
            with pytest.raises(RuntimeError, match="only float32 and float64 are supported"):
                f(bad, *args)
        for bad in (torch.zeros((2, 3, 4)), torch.zeros((5,)), torch.zeros((2, 3, 4, 5, 6, 7))):
            with pytest.raises(RuntimeError, match=r"must be a field of shape \(N, C, \*spatial\) with two or three spatial axes"):
                f(bad, *args)
        with pytest.raises(RuntimeError, match="has an empty spatial axis"):
            f(torch.zeros((2, 3, 5, 0, 7)), *args)
        with pytest.raises(RuntimeError, match="must be contiguous"):
            f(strided(good), *args)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):   # all fine but for the device
            f(good, *args)
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            f(good.double(), *args)
        # the order: dtype before shape before layout before device
        with pytest.raises(RuntimeError, match="only float32 and float64"):
            f(strided(torch.zeros((2, 3, 4, 5, 6, 7), dtype=torch.int32)), *args)
        with pytest.raises(RuntimeError, match="two or three spatial axes"):
            f(strided(torch.zeros((2, 3, 4, 0, 6, 7))), *args)
        with pytest.raises(RuntimeError, match="empty spatial axis"):
            f(strided(torch.zeros((2, 3, 5, 6, 0))), *args)
    for f in up:
        for bad in ((5, 6), (5, 6, 9), (4, 6, 7), (7, 6, 7), [6, 6, 9]):
            with pytest.raises(RuntimeError, match="does not match the fine grid"):
                f(c3, bad)
        for bad in (None, 5, (5, 6.0, 7), (5, 0, 7), (5, True, 7), "567", (5, 6, 7, 8)):
            with pytest.raises(RuntimeError, match="shape must give two or three spatial axes with extents >= 1"):
                f(c3, bad)
        with pytest.raises(RuntimeError, match="does not match the fine grid"):   # the shape before the layout
            f(strided(c3), (9, 6, 7))
        for shape in ((9, 11), (10, 11), (9, 12), [10, 12]):   # both n = 2 m and n = 2 m - 1
            with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
                f(c2, shape)
    for f, args in ((lm.pyramid_expand, (c3, (5, 6, 7))), (lm.pyramid_expand_adjoint, (x3,))):
        for bad in (float("inf"), float("-inf"), float("nan"), None, "2", True, [2.0], torch.ones(1)):
            with pytest.raises(RuntimeError, match="scale must be a finite number"):
                f(*args, scale=bad)
        with pytest.raises(RuntimeError, match="scale must be a finite number"):   # the scale before the layout
            f(strided(args[0]), *args[1:], scale=float("nan"))
        for scale in (2.0, 2, 0.0, -1.5):
            with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
                f(*args, scale=scale)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        lm.pyramid_reduce(x2.clone().requires_grad_(True))


def test_pyramid_shape_rules():
    import lagomorph_amd as lm

    assert lm.pyramid_shape((1, 2, 3)) == (1, 1, 2) and lm.pyramid_shape([64, 65]) == (32, 33)
    assert lm.pyramid_shape(torch.Size((7, 8))) == (4, 4)
    for shape in ref.CASES:
        assert lm.pyramid_shape(shape) == ref.coarse_shape(shape)
    for bad in ((), (5,), (1, 2, 3, 4), (0, 3), (5, -1, 2), (5.0, 3), (True, 3), None, 7, "ab", (None, 2)):
        with pytest.raises(RuntimeError, match="shape must give two or three spatial axes with extents >= 1"):
            lm.pyramid_shape(bad)


def test_image_pyramid_rules():
    import lagomorph_amd as lm

    x = torch.zeros((1, 1, 40, 33, 17))
    for bad in (0, -1, 2.0, True, "3", (2,)):
        with pytest.raises(ValueError, match="levels must be an integer >= 1 or None"):
            lm.image_pyramid(x, levels=bad)
    for bad in (0, -1, 8.0, True, None, "8"):
        with pytest.raises(ValueError, match="min_size must be an integer >= 1"):
            lm.image_pyramid(x, min_size=bad)
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        lm.image_pyramid(x.numpy())
    out = lm.image_pyramid(x, levels=1)
    assert len(out) == 1 and out[0] is x
    # the next level would be (20, 17, 9): nothing under 8, so a kernel is needed -- and x is a CPU tensor
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        lm.image_pyramid(x)
    assert len(lm.image_pyramid(x, min_size=10)) == 1            # 17 -> 9 < 10: no coarser level
    assert len(lm.image_pyramid(torch.zeros((1, 1, 1, 1)))) == 1   # single voxels: no coarser level
    assert len(lm.image_pyramid(torch.zeros((1, 2, 14, 1)), levels=5)) == 1   # 14 -> 7 < 8; the extent of 1 does not count


def test_c_entry_points_validate_before_any_device_call():
    from lagomorph_amd import lagomorph_ext as ext

    OK, INVALID = 0, -1
    p, q = 0x100000, 0x4000000   # never dereferenced: every call returns before a launch
    err = ext._lib.lago_last_error
    for suf in ("_f32", "_f64"):
        for stem in ("lago_pyramid_down", "lago_pyramid_up"):
            f = ext._fn[stem + suf]
            assert f(p, q, 0, 4, 6, 5, 6, 7, 1.0, None) == INVALID and b"dimensional" in err(), stem
            assert f(p, q, 0, 1, 6, 5, 6, 7, 1.0, None) == INVALID and b"dimensional" in err()
            assert f(p, q, 1, 3, 6, 5, -6, 7, 1.0, None) == INVALID and b"negative" in err()
            assert f(p, q, 1, 3, -6, 5, 6, 7, 1.0, None) == INVALID and b"negative" in err()
            assert f(p, q, 0, 3, 6, 1 << 10, 1 << 10, 1 << 9, 1.0, None) == INVALID and b"2^29" in err()
            assert f(p, q, 0, 2, 6, 1 << 15, 1 << 14, 1, 1.0, None) == INVALID and b"2^29" in err()
            for op in (2, -1):
                assert f(p, q, op, 3, 6, 5, 6, 7, 1.0, None) == INVALID and b"unknown op" in err()
            assert f(None, q, 0, 3, 6, 5, 6, 7, 1.0, None) == INVALID and b"null" in err()
            assert f(p, None, 1, 3, 6, 5, 6, 7, 1.0, None) == INVALID and b"null" in err()
            assert f(p, p, 0, 3, 6, 5, 6, 7, 1.0, None) == INVALID and b"overlap" in err()
            assert f(p, p + 64, 1, 2, 6, 5, 6, 1, 2.0, None) == INVALID and b"overlap" in err()
            for rows, nx, ny, nz in ((0, 5, 6, 7), (6, 0, 6, 7), (6, 5, 0, 7), (6, 5, 6, 0)):   # empty: nothing to do
                assert f(None, None, 0, 3, rows, nx, ny, nz, 1.0, None) == OK
            assert f(None, None, 1, 2, 6, 5, 0, 0, 1.0, None) == OK
        # the coarse side's bytes decide the overlap: 6 rows of 3 x 3 x 4 against 6 rows of 5 x 6 x 7
        esz = 4 if suf == "_f32" else 8
        fine, coarse = 6 * 5 * 6 * 7 * esz, 6 * 3 * 3 * 4 * esz
        assert ext._fn["lago_pyramid_down" + suf](q - coarse + esz, q, 0, 3, 6, 5, 6, 7, 1.0, None) == INVALID and b"overlap" in err()
        assert ext._fn["lago_pyramid_up" + suf](q + coarse - esz, q, 0, 3, 6, 5, 6, 7, 1.0, None) == INVALID and b"overlap" in err()
        assert ext._fn["lago_pyramid_up" + suf](q - fine + esz, q, 0, 3, 6, 5, 6, 7, 1.0, None) == INVALID and b"overlap" in err()
