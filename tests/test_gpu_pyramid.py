"""GPU: pyramid_reduce, pyramid_expand and their transposes (csrc/pyramid.hip) against the numpy reference
tests/pyramid_ref.py (which tests/test_pyramid_host.py ties to torch's convolution and interpolation and to known
answers).

Shapes (pyramid_ref.CASES) are the smallest that reach every path of the 8 x 8 x 64 (2D: 64 x 64) fine tile; N in
{1, 2}, C in {1, d, 4}.

Exact: integer-valued inputs with |a| <= 512 and a scale of 1 or 2 -- every partial sum is representable, so the result
equals the float64 reference bit for bit after conversion, for all four operators and both dtypes.
Real-valued (uniform in [0, 1)): per element |got - ref| <= K u sum_taps |W| |a|, K = 5 d + 1 the header's own count
(pyramid_weights.hpp: kPyrRoundings, at most 6 d + 2), u the unit roundoff, against float64 sums for float32 results
and long double sums for float64; the project's rule 1e-5 / 1e-12 x max|ref|; and the same bits as the numpy
restatement of the header's order.  The worst observed ratios are printed.
Then: the same bits from call to call and on a second stream, inputs untouched, the adjoint identities in float64,
gradcheck and gradgradcheck, inputs one element off the 16-byte alignment, and the round trip of a ramp."""
import functools

import numpy as np
import pytest
import torch

import pyramid_ref as ref
from gpu_util import dev, host
from offset_views import margins_intact, offset_view, poisoned
from parity_rule import rtol

pytestmark = pytest.mark.gpu

both_dtypes = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
cases = pytest.mark.parametrize("shape", ref.CASES, ids=str)
ops = pytest.mark.parametrize("op", ref.OPS)
UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def _batches(d):
    """(N, C): N in {1, 2}, C in {1, d, 4}."""
    return [(1 if C == 1 else 2, C) for C in sorted({1, d, 4})]


def _scales(op):
    return (1.0, 2.0) if op.startswith("expand") else (1.0,)   # the reduce and its transpose take no scale


def run(lm, op, x, shape, scale=1.0):
    if op == "reduce":
        return lm.pyramid_reduce(x)
    if op == "reduce_adjoint":
        return lm.pyramid_restrict_adjoint(x, shape)
    if op == "expand":
        return lm.pyramid_expand(x, shape, scale)
    return lm.pyramid_expand_adjoint(x, scale)


@functools.lru_cache(maxsize=None)
def _exact_case(op, shape, dtype, N, C, scale):
    a = ref.integer_field(N, C, ref.in_shape(op, shape), np.dtype(dtype), seed=len(shape) + N + C)
    out = (a, ref.reference(op, a, shape, scale))
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _real_case(op, shape, dtype, N, C, scale):
    """(input, reference, bound scale sum |W| |a|, the header's order restated); the reference's sums in long double for
    float64 results."""
    dtype = np.dtype(dtype)
    a = ref.real_field(N, C, ref.in_shape(op, shape), dtype, seed=11 + len(shape) + N + C)
    work = np.longdouble if dtype == np.float64 else np.float64
    out = (a, ref.reference(op, a, shape, scale, work), ref.abs_reference(op, a, shape, scale, work), ref.native(op, a, shape, scale))
    for v in out:
        v.setflags(write=False)
    return out


@both_dtypes
@cases
def test_integer_inputs_are_exact(shape, dtype):
    import lagomorph_amd as lm

    for op in ref.OPS:
        for N, C in _batches(len(shape)):
            for scale in _scales(op):
                a, want = _exact_case(op, shape, np.dtype(dtype).name, N, C, scale)
                got = run(lm, op, dev(a), shape, scale)
                assert got.shape == (N, C) + ref.out_shape(op, shape) and got.is_contiguous() and got.dtype == dev(a).dtype
                assert np.array_equal(host(got).astype(np.float64), want), (op, N, C, scale)


@both_dtypes
@cases
def test_real_inputs_within_the_rounding_bound(shape, dtype):
    import lagomorph_amd as lm

    K, u = ref.header_roundings(len(shape)), UNIT[np.dtype(dtype)]
    assert K <= 6 * len(shape) + 2
    worst = {}
    for op in ref.OPS:
        for N, C in _batches(len(shape)):
            for scale in _scales(op):
                a, want, mag, native = _real_case(op, shape, np.dtype(dtype).name, N, C, scale)
                ad = dev(a)
                got = run(lm, op, ad, shape, scale)
                assert got.shape == (N, C) + ref.out_shape(op, shape) and got.is_contiguous() and got.dtype == ad.dtype
                h = host(got)
                err = np.abs(h.astype(want.dtype) - want)
                ratio = float((err / (K * u * mag)).max())
                worst[op] = max(worst.get(op, 0.0), ratio)
                assert ratio <= 1.0, f"{op} {shape} N {N} C {C} scale {scale}: {ratio:.3f} of K u sum |W| |a|, K = {K}"
                assert float(err.max()) <= rtol(dtype) * float(np.abs(want).max()), (op, N, C, scale)
                assert np.array_equal(h, native), f"{op} {shape} N {N} C {C}: not the bits of the header's order"
                assert torch.equal(got, run(lm, op, ad, shape, scale))   # no atomics: the same bits
                assert torch.equal(ad, dev(a))                           # the input is left alone
    print(f"pyramid {shape} {np.dtype(dtype).name}: of K u sum |W| |a| at most " + ", ".join(f"{o} {r:.3f}" for o, r in worst.items()))


@both_dtypes
@ops
def test_same_bits_on_a_second_stream(op, dtype):
    import lagomorph_amd as lm

    for shape in ((18, 19, 130), (130, 66)):
        a = dev(ref.real_field(2, 3, ref.in_shape(op, shape), np.dtype(dtype), seed=5))
        keep = a.clone()
        first = run(lm, op, a, shape, 2.0)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            second = run(lm, op, a, shape, 2.0)
        s.synchronize()
        assert torch.equal(first, second) and torch.equal(a, keep)


@pytest.mark.parametrize("op", ["reduce", "expand"])
def test_adjoint_identity(op):
    """<M a, b> = <a, M^T b> in float64, to 1e-12 relative (positive inputs: nothing cancels)."""
    import lagomorph_amd as lm

    for shape in ref.CASES:
        a = dev(ref.real_field(2, 2, ref.in_shape(op, shape), np.float64, seed=1))
        b = dev(ref.real_field(2, 2, ref.out_shape(op, shape), np.float64, seed=2))
        lhs = float((run(lm, op, a, shape, 1.0) * b).sum())
        rhs = float((a * run(lm, op + "_adjoint", b, shape, 1.0)).sum())
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs) and lhs > 0, (op, shape, lhs, rhs)


@pytest.mark.parametrize("shape", [(5, 4, 7), (6, 7)], ids=str)
def test_gradcheck(shape):
    import lagomorph_amd as lm

    cs = ref.coarse_shape(shape)
    x = dev(ref.real_field(1, 2, shape, np.float64, seed=3)).requires_grad_(True)
    c = dev(ref.real_field(1, 2, cs, np.float64, seed=4)).requires_grad_(True)
    fns = ((lm.pyramid_reduce, x), (lambda t: lm.pyramid_expand_adjoint(t, 1.5), x),
           (lambda t: lm.pyramid_expand(t, shape, 2.0), c), (lambda t: lm.pyramid_restrict_adjoint(t, shape), c),
           (lambda t: lm.pyramid_expand(lm.pyramid_reduce(t), shape), x))
    for f, t in fns:
        assert torch.autograd.gradcheck(f, (t,), eps=1e-6, atol=1e-8, rtol=1e-6)
        assert torch.autograd.gradgradcheck(lambda t: f(t) ** 2, (t,), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_image_pyramid():
    import lagomorph_amd as lm

    for shape in ((9, 8, 11), (12, 9)):
        x = dev(ref.real_field(1, 2, shape, np.float64, seed=6)).requires_grad_(True)

        def levels(t):
            return tuple(lm.image_pyramid(t, levels=3, min_size=1))

        out = levels(x)
        assert len(out) == 3 and out[0] is x
        want = host(x)
        for level in out[1:]:
            want = ref.reference("reduce", want, tuple(want.shape[2:]))
            assert tuple(level.shape[2:]) == tuple(want.shape[2:]) and np.abs(host(level) - want).max() <= 1e-12
        assert torch.autograd.gradcheck(lambda t: levels(t)[1:], (x,), eps=1e-6, atol=1e-8, rtol=1e-6)
        assert torch.autograd.gradgradcheck(lambda t: levels(t)[2] ** 2, (x,), eps=1e-6, atol=1e-7, rtol=1e-5)
    big = dev(ref.real_field(1, 1, (40, 33, 17), np.float32))
    assert [tuple(t.shape[2:]) for t in lm.image_pyramid(big)] == [(40, 33, 17), (20, 17, 9)]   # 9 -> 5 < 8
    assert [tuple(t.shape[2:]) for t in lm.image_pyramid(big, levels=4, min_size=3)] == [(40, 33, 17), (20, 17, 9), (10, 9, 5), (5, 5, 3)]
    assert [tuple(t.shape[2:]) for t in lm.image_pyramid(big, levels=2, min_size=1)] == [(40, 33, 17), (20, 17, 9)]
    x = big.clone().requires_grad_(True)
    assert not lm.pyramid_reduce(big).requires_grad and lm.pyramid_reduce(x).requires_grad


@both_dtypes
@ops
def test_inputs_one_element_off_the_alignment(op, dtype):
    import lagomorph_amd as lm

    for shape in ((9, 17, 65), (65, 127)):
        a = dev(ref.real_field(2, 1, ref.in_shape(op, shape), np.dtype(dtype), seed=9))
        want = run(lm, op, a, shape, 2.0)
        view, buf = offset_view(a, 1)
        got = run(lm, op, view, shape, 2.0)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and poisoned(got) == 0
        assert margins_intact(buf, view) == [] and torch.equal(view, a)


@both_dtypes
def test_round_trip_of_a_ramp(dtype):
    import lagomorph_amd as lm

    for shape in ((18, 19, 130), (17, 10, 129), (65, 127), (130, 66)):
        grid = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
        ramp = (sum(c * g for c, g in zip((3.0, -2.0, 5.0), grid)) + 7.0)[None, None].astype(dtype)
        back = host(lm.pyramid_expand(lm.pyramid_reduce(dev(ramp)), shape))
        inner = (0, 0) + tuple(slice(4, n - 4) for n in shape)
        assert back.shape == ramp.shape and np.array_equal(back[inner], ramp[inner]) and ramp[inner].size > 0
