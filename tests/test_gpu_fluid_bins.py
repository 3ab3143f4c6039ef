"""GPU: every implementation of the fluid metric judged bin by bin in Fourier space (tests/fluid_bins.py) -- every x
length, every one-kernel (ny, nz) plane and every rows + columns length of the tuned passes, their tuning variants, the
21 fused 2D shapes, the generic passes in both precisions (odd extents, a Bluestein line, radix 13, in-place and ping-pong
stages, fused and separate x pass) and the rocFFT forms -- at the smallest shapes that reach each instantiation.

The older FFT tests judge with max |out - ref| / max |ref| <= 2e-6 on white input, which an error confined to a bin, a
row or a plane of the spectrum passes (tests/test_fluid_bins_host.py plants such errors).  Here the output's spectrum is
compared with the float64 symbol applied to the input's spectrum, per batch item, component and bin, in units of what
float32 (float64) resolves at that bin, and held to 4 x what an independent pipeline of the same precision (pocketfft +
the oracle's operator) shows ON THE SAME INPUT, in the largest bin and at the 99.9th percentile.  Every case asserts the
path counter of the implementation it is after and runs two parameter sets in both directions: (0.1, 0.05, 1.0), well
conditioned, where the per-bin resolution is sharpest, and the suite's usual (0.1, 0.05, 0.01), whose sharp is looser
(its symbol spans four decades; the reference itself reaches tens of units there).

LAGO_BIN_REPORT=<file>: the observed figures of the run as JSON (tools/fluid_bin_report.py turns it into
profiles/fluid_bin_units.md).
"""
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import fluid_bins as fb

pytestmark = pytest.mark.gpu

OBSERVED = {}
PARAM_SETS = (fb.PARAMS_WELL, fb.PARAMS_USUAL)
POOL = ThreadPoolExecutor(4)   # the four (parameter set, direction) combinations of a case are judged side by side (numpy and pocketfft release the GIL)


@pytest.fixture(scope="module")
def ext():
    import lagomorph_amd

    e = lagomorph_amd.lagomorph_ext
    try:
        yield e
    finally:
        e.set_fluid_mode(3)
        e.set_fluid_tuning()
        out = os.environ.get("LAGO_BIN_REPORT")
        if out:
            json.dump(dict(sorted(OBSERVED.items())), open(out, "w"), indent=1)


def combo_name(params, inverse):
    return f"{'sharp' if inverse else 'flat'} gamma={params[2]:g}"


def run_operator(ext, m, mode, path, tuning=None):
    """{(params, inverse): output as numpy} of one device input through lm.FluidMetric, the path counter asserted per call."""
    import lagomorph_amd as lm

    outs = {}
    ext.set_fluid_mode(mode)
    if tuning:
        ext.set_fluid_tuning(**tuning)
    try:
        for params in PARAM_SETS:
            met = lm.FluidMetric(list(params))
            for inverse in (False, True):
                before = ext.path_launches(path)
                out = met.sharp(m) if inverse else met.flat(m)
                assert ext.path_launches(path) == before + 1, f"not the {path} path ({combo_name(params, inverse)})"
                assert out.dtype == m.dtype and out.shape == m.shape
                outs[(params, inverse)] = out
    finally:
        ext.set_fluid_mode(3)
        ext.set_fluid_tuning()
    return outs


def judge(tag, m, outs, white=True):
    """The acceptance rule on every (params, direction) of one input; all figures go to OBSERVED before anything is
    asserted, and a failure names every failing combination with its worst bin."""
    eps = fb.EPS32 if m.dtype == np.float32 else fb.EPS64
    Mhat = fb.spectrum(m)
    t0 = time.time()

    def one(key):
        params, inverse = key
        J = fb.Judge(m, params, inverse, eps, Mhat, pairs[params], coherent=not white)
        assert np.isfinite(outs[key]).all(), (tag, combo_name(params, inverse))
        return params, inverse, J.figures(outs[key]), J.figures(fb.reference(m, params, inverse))

    pairs = dict(zip(PARAM_SETS, POOL.map(lambda params: fb.symbol_pair(m.shape[2:], params), PARAM_SETS)))
    failures = []
    for params, inverse, got, ref in POOL.map(one, [(p, i) for p in PARAM_SETS for i in (False, True)]):
        name = combo_name(params, inverse)
        # two-bin input: units with the coherent noise level (fluid_bins.Judge).  pocketfft leaves the empty bins EXACTLY
        # zero on power-of-two extents (equal numbers cancel in its butterflies), a property of that input and not of the
        # format; a reference figure below one unit -- by construction the rounding level of the format at a bin --
        # counts as one unit
        ok, rmax, rp = fb.verdict(got, ref, floor=0.0 if white else 1.0)
        OBSERVED.setdefault(tag, {})[name] = {
            "ratio_max": rmax, "ratio_p999": rp, "max": got["max"], "p999": got["p999"], "median": got["median"],
            "worst": list(got["worst"]), "ref_max": ref["max"], "ref_p999": ref["p999"]}
        print(fb.describe(f"{tag} {name}: {rmax:.2f} x / {rp:.2f} x the reference", got, ref))
        if white and fb.well_conditioned(params, inverse) and not fb.reference_guard(ref, m.dtype, Mhat.size):
            failures.append(f"reference outside its own conditions: {tag} {name} {ref}")
        if not ok:
            failures.append(fb.describe(f"{tag} {name}: {rmax:.2f} x / {rp:.2f} x the reference (allowed {fb.MARGIN:g})", got, ref))
    OBSERVED[tag]["seconds"] = round(time.time() - t0, 2)
    assert not failures, "\n".join(failures)


def to_host(outs):
    return {k: v.cpu().numpy() for k, v in outs.items()}


WHITE = fb.white_cases()


@pytest.mark.parametrize("case", WHITE, ids=[c[0] for c in WHITE])
def test_white_input_bin_by_bin(ext, case):
    tag, sp, dt, mode, path = case
    m = fb.white_input(sp, 2, np.dtype(dt), fb.case_seed(sp))
    outs = to_host(run_operator(ext, torch.from_numpy(m).cuda(), mode, path))
    judge(tag, m, outs)


@pytest.mark.parametrize("sp", fb.VARIANT_SHAPES, ids=["x".join(map(str, s)) for s in fb.VARIANT_SHAPES])
def test_tuning_variants_have_the_bits_of_the_default(ext, sp):
    """xpass_persist = 2 (the persistent x-pass grid whatever the size of the launch), xpass_wide = 0 (256 threads where
    the default takes 512) and zy_persist = 0 (one-shot zy kernels for planes above 80 KB): speed-only settings, so each
    has the bits of the default, and the bits of the default pass the bin rule."""
    m = fb.white_input(sp, 2, np.float32, fb.case_seed(sp))
    md = torch.from_numpy(m).cuda()
    base = run_operator(ext, md, 3, "fluid_lds")
    for tuning in fb.VARIANTS:
        var = run_operator(ext, md, 3, "fluid_lds", tuning)
        for key in base:
            assert torch.equal(var[key], base[key]), (sp, tuning, combo_name(*key))
    judge("variants-" + "x".join(map(str, sp)), m, to_host(base))


@pytest.mark.parametrize("case", fb.TWO_BIN_CASES, ids=[f"{c[3]}-mode{c[2]}-{'x'.join(map(str, c[0]))}-{c[1]}" for c in fb.TWO_BIN_CASES])
def test_two_bin_input_bin_by_bin(ext, case):
    """m = a + b (-1)^(x + y + z) per component: the expected output is K(0) a + K(pi, pi, pi) b (-1)^(x + y + z), the DC
    bin and the far Nyquist corner alone, which under white input sit below the noise of every other bin."""
    sp, dt, mode, path = case
    m = fb.two_bin_input(sp, 2, np.dtype(dt), fb.case_seed(sp))
    outs = to_host(run_operator(ext, torch.from_numpy(m).cuda(), mode, path))
    judge(f"twobin-{path}-mode{mode}-{'x'.join(map(str, sp))}-{dt}", m, outs, white=False)
