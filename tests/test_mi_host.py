"""CPU: the specification of mutual information before any GPU run.

- tests/mi_ref.py, the numpy float64 reference: its two exact integer routes agree, the fixed-point table is within
  2^-33 of the unquantised one, the transpose identity is exact, and its analytic gradient meets central differences of
  the unquantised MI and NMI;
- lagomorph_amd/csrc/mi_window.hpp, the header the kernels call: tests/native/mi_emul.cpp runs every voxel of a case
  through its functions with a plain host compiler, and the table equals mi_ref's integer for integer (indices, window
  derivatives and the backward sums bit for bit as well);
- the Python layer's argument errors, and the shim's refusal of CPU tensors."""
import struct

import numpy as np
import pytest
import torch

import mi_ref
import native_build


# ---- the reference against itself

@pytest.mark.parametrize("B", mi_ref.BINS)
def test_reference_integer_routes_agree_and_quantisation_is_small(B):
    lead, sp = (2, 2), (5, 6, 7)
    for kind in mi_ref.KINDS:
        I, J, _, rI, rJ = mi_ref.inputs(lead, sp, kind)
        rI, rJ = rI or mi_ref.auto_range(I), rJ or mi_ref.auto_range(J)
        H = mi_ref.histogram_int(I, J, B, rI, rJ)
        assert H.dtype == np.int64 and np.array_equal(H, mi_ref.histogram_int_add_at(I, J, B, rI, rJ)), kind
        nvox = int(np.prod(sp))
        # every voxel's 16 products sum to 2^32 up to their 16 roundings of at most 1/2
        assert np.abs(H.sum((1, 2)) - nvox * 2 ** 32).max() <= 8 * nvox
        # a bin is the mean over the voxels of products rounded by at most 2^-33 each
        err = np.abs(mi_ref.P_of(H, nvox) - mi_ref.histogram_float(I, J, B, rI, rJ)).max()
        assert err <= 2.0 ** -33 + 1e-15, (kind, err)
        assert np.array_equal(mi_ref.histogram_int(J, I, B, rJ, rI), H.transpose(0, 2, 1)), kind


@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("B", mi_ref.BINS)
def test_reference_gradient_against_central_differences(B, normalized):
    """Central differences of the UNQUANTISED MI (the function the analytic gradient belongs to) at twelve voxels of each
    image, ranges that clamp both ends.  h = 1e-5: the truncation error h^2 / 6 |f'''| is below 1e-7 of the largest
    gradient entry (f''' / f' is about s^2 <= 23^2 here, the windows being cubic), the rounding error
    2e-16 |MI| / h = 2e-11 absolute.  The bound is 1e-6 max|g| + 1e-10.  Voxels within h of a range bound, where the
    derivative jumps, are left out (none of these draws has one among the sampled voxels more than rarely)."""
    h = 1e-5
    for lead, sp in mi_ref.FD_SHAPES:
        I, J, _, rI, rJ = mi_ref.inputs(lead, sp, "clamp")
        clamped = np.mean((I < rI[0]) | (I > rI[1])), np.mean((J < rJ[0]) | (J > rJ[1]))
        assert 0.03 <= min(clamped) and max(clamped) <= 0.3, clamped
        _, G = mi_ref.mi_of(mi_ref.histogram_float(I, J, B, rI, rJ), normalized)
        dI, dJ = mi_ref.backward(G, I, J, B, rI, rJ)
        f = lambda a, b: float(mi_ref.mi_float(a, b, B, rI, rJ, normalized)[0])
        rng = np.random.default_rng([B, *sp])
        worst, top, used = 0.0, max(np.abs(dI).max(), np.abs(dJ).max()), 0
        for which, (x, r, d) in enumerate(((I, rI, dI), (J, rJ, dJ))):
            for flat in rng.permutation(x.size)[:12]:
                idx = np.unravel_index(flat, x.shape)
                if min(abs(x[idx] - r[0]), abs(x[idx] - r[1])) <= 2 * h:
                    continue
                lo, hi = x.copy(), x.copy()
                lo[idx] -= h
                hi[idx] += h
                fd = (f(hi, J) - f(lo, J)) / (2 * h) if which == 0 else (f(I, hi) - f(I, lo)) / (2 * h)
                worst = max(worst, abs(fd - d[idx]))
                used += 1
        print(f"{sp} B={B} normalized={normalized}: max|fd - analytic| {worst:.3e} at max|g| {top:.3e} ({used} voxels)")
        assert used >= 20 and top > 0
        assert worst <= 1e-6 * top + 1e-10


# ---- the header against the reference

def _emul(tmp_path):
    return native_build.build(tmp_path, "mi_emul.cpp", werror=False)


def _run_emul(exe, tmp_path, B, rI, rJ, I, J, G):
    n = I.size
    src, dst = str(tmp_path / f"in_{B}.bin"), str(tmp_path / f"out_{B}.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<ii4d", B, n, rI[0], rI[1], rJ[0], rJ[1]))
        for a in (I, J, G):
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    native_build.run(exe, src, dst)
    raw = open(dst, "rb").read()
    out, at = [], 0
    for dt, cnt in (("<i8", B * B), ("<i4", n), ("<i4", n), ("<f8", 4 * n), ("<f8", 4 * n), ("<f8", n), ("<f8", n)):
        out.append(np.frombuffer(raw, dtype=dt, count=cnt, offset=at))
        at += cnt * np.dtype(dt).itemsize
    assert at == len(raw)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@native_build.needs_cxx
def test_header_emulation_equals_the_reference_integer_for_integer(tmp_path):
    """B in {4, 5, 32, 64}; noise voxels of float32 and of full float64 values, values exactly lo and hi, values outside
    the range, NaN, +inf and -inf in either image."""
    exe = _emul(tmp_path)
    rng = np.random.default_rng(7)
    rI, rJ = (-1.0, 0.75), (-0.3, 1.7)
    special = [rI[0], rI[1], np.nextafter(rI[0], 9), np.nextafter(rI[1], -9), np.nextafter(rI[0], -9), np.nextafter(rI[1], 9),
               -5.0, 5.0, 1e300, -1e300, np.nan, np.inf, -np.inf, 0.0, -0.0]
    specialJ = [rJ[0], rJ[1], np.nextafter(rJ[0], 9), np.nextafter(rJ[1], -9), np.nextafter(rJ[0], -9), np.nextafter(rJ[1], 9),
                -5.0, 5.0, 1e300, -1e300, np.nan, np.inf, -np.inf, 0.0, -0.0]
    noise = rng.standard_normal(700)
    noise[:350] = noise[:350].astype(np.float32)
    I = np.concatenate([noise, np.repeat(special, len(specialJ)), rng.standard_normal(60)])
    J = np.concatenate([0.5 * noise + 0.7 * rng.standard_normal(700), np.tile(specialJ, len(special)), np.repeat(specialJ, 4)])
    assert I.size == J.size
    shape = (1, 1, I.size, 1)
    for B in mi_ref.BINS:
        G = rng.standard_normal((B, B))
        H, kI, kJ, dwI, dwJ, dI, dJ = _run_emul(exe, tmp_path, B, rI, rJ, I, J, G)
        assert np.array_equal(H.reshape(1, B, B), mi_ref.histogram_int_add_at(I.reshape(shape), J.reshape(shape), B, rI, rJ))
        assert np.array_equal(H.reshape(1, B, B), mi_ref.histogram_int(I.reshape(shape), J.reshape(shape), B, rI, rJ))
        for x, r, k, dw in ((I, rI, kI, dwI), (J, rJ, kJ, dwJ)):
            rk, _, rdw = mi_ref.window(x, r, B)
            assert k.min() >= 0 and k.max() <= B - 4 and np.array_equal(k, rk)
            assert np.array_equal(_bits(dw.reshape(-1, 4)), _bits(rdw))
            with np.errstate(invalid="ignore"):
                outside = ~((x >= r[0]) & (x <= r[1]))
            assert outside.sum() >= 100 and not dw.reshape(-1, 4)[outside].any()
            assert dw.reshape(-1, 4)[~outside].any(axis=1).all()
        rdI, rdJ = mi_ref.backward(G[None], I.reshape(shape), J.reshape(shape), B, rI, rJ)
        assert np.array_equal(_bits(dI), _bits(rdI.reshape(-1))) and np.array_equal(_bits(dJ), _bits(rdJ.reshape(-1)))
        # the two backward expressions are one function with the roles swapped and G transposed
        _, _, _, _, _, sI, sJ = _run_emul(exe, tmp_path, B, rJ, rI, J, I, G.T)
        assert np.array_equal(_bits(sI), _bits(dJ)) and np.array_equal(_bits(sJ), _bits(dI))


# ---- the Python layer

def test_shim_raises_on_cpu_tensors():
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    I, J = torch.rand((1, 1, 4, 5, 6)), torch.rand((1, 1, 4, 5, 6))
    G = torch.zeros((1, 1, 8, 8), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ext.mi_histogram(I, J, 8, (0.0, 1.0), (0.0, 1.0))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ext.mi_backward(G, I, J, 8, (0.0, 1.0), (0.0, 1.0), True, True)
    for f in (lm.joint_histogram, lm.mutual_information, lm.mi_loss, lm.MISimilarity()):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            f(I, J)
    assert ext.MI_MIN_BINS == 4 and ext.MI_MAX_BINS == 64 and ext.MI_FRAC_BITS == 32


def test_argument_errors():
    import lagomorph_amd as lm

    I, J = torch.rand((1, 1, 4, 5, 6)), torch.rand((1, 1, 4, 5, 6))
    for f in (lm.joint_histogram, lm.mutual_information, lm.mi_loss):
        for bins in (3, 65, 0, -1, 7.5):
            with pytest.raises(ValueError, match="bins"):
                f(I, J, bins=bins)
        for bad in ((1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("-inf"), 0.0), (float("nan"), 1.0), (0.0,), "ab"):
            with pytest.raises(ValueError, match="range_I"):
                f(I, J, range_I=bad)
            with pytest.raises(ValueError, match="range_J"):
                f(I, J, range_J=bad)
        with pytest.raises(RuntimeError, match="same shape"):
            f(I, J[..., :5])
        with pytest.raises(RuntimeError, match="dtype"):
            f(I, J.double())
        with pytest.raises(TypeError):
            f(I, J.numpy())
        with pytest.raises(ValueError, match="explicitly"):   # no range can be taken from an image with NaN voxels
            f(torch.full_like(I, float("nan")), J)
    for eps in (0.0, -1e-10, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            lm.mutual_information(I, J, eps=eps)
        with pytest.raises(ValueError, match="eps"):
            lm.MISimilarity(eps=eps)
    with pytest.raises(ValueError, match="reduction"):
        lm.mi_loss(I, J, reduction="max")
    for kw in (dict(bins=3), dict(bins=65), dict(range_I=(1.0, 0.0)), dict(range_J=(0.0, float("nan")))):
        with pytest.raises(ValueError):
            lm.MISimilarity(**kw)
    s = lm.MISimilarity(16, range_I=(0, 1), normalized=True)
    assert (s.bins, s.range_I, s.range_J, s.normalized, s.eps) == (16, (0.0, 1.0), None, True, 1e-10)
    for name in ("JointHistogramFunction", "joint_histogram", "mutual_information", "mi_loss", "MISimilarity"):
        assert hasattr(lm, name)
