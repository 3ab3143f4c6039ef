#!/usr/bin/env python3
"""gaussian_smooth: the separable kernels (whole and pass by pass) against the two ways a user had to blur a field
before them, and the multi-Gaussian `sharp` with and without the accumulate epilogue; arms alternating in one process,
HIP events around every call, JSON on stdout.

    python tools/time_gauss.py [--calls 30] [--warmup 5] [--rounds 3] [--shape 8x128] [--sigmas 1,2,4] [--only-gauss] [--no-conv]

Arms (N x 3 x S^3 float32 noise, periodic border), per sigma s:
  gauss_s        lagomorph_amd.gaussian_smooth(x, s)                                (three launches)
  pass_x_s ...   gaussian_smooth(x, (s, 0, 0)) / (0, s, 0) / (0, 0, s)              (one launch each)
  fft_s          the torch FFT blur: rfftn, three per-axis multipliers, irfftn      (bench.gaussian_blur's formula, copied)
  conv_s         three torch.nn.functional.conv3d calls with 1-D kernels on a circularly padded field
and once:
  sharp3_acc     GaussianMetric([1, 2, 4]).sharp(x): nine launches, the sum in the epilogue of every term's last pass
  sharp3_sum     the same three gaussian_smooth calls added with torch (nine launches + two elementwise passes)
Every round times each arm `calls` times, the arms taking turns; the figure of a round is the median over its calls, and
the spread quoted is that of the rounds' medians ((max - min) / median).  Before anything is timed the three forms are
compared: gauss against conv (the same truncated kernel) at 1e-5 of max|.|, and against the untruncated FFT blur, whose
difference is reported only.  --only-gauss runs the library's arms alone (a target for `rocprofv3 --kernel-trace --stats`).
Fractions of HBM peak use 8 TB/s and the algorithmic traffic of 8 bytes per voxel and pass.
The GPU is idle when the first event is recorded, so an event time holds the host work the call does before its first
launch (tap vectors, argument checks, allocations) as well as the kernels; `host_ms_in_call` is the median wall time the
host spends inside the call (an upper bound of that share).  Kernel times proper need the rocprofv3 run.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lagomorph_amd as lm  # noqa: E402

HBM_PEAK = 8.0e12


def fft_blur(x, sigma):
    """Periodic Gaussian blur over the spatial axes via FFT (the formula of bench.gaussian_blur)."""
    dims = tuple(range(2, x.dim()))
    F = torch.fft.rfftn(x, dim=dims)
    for d in dims:
        n = x.shape[d]
        k = torch.fft.rfftfreq(n, device=x.device) if d == dims[-1] else torch.fft.fftfreq(n, device=x.device)
        g = torch.exp(-2.0 * (torch.pi * k * sigma) ** 2)
        shape = [1] * F.dim()
        shape[d] = g.numel()
        F = F * g.view(shape)
    return torch.fft.irfftn(F, s=[x.shape[d] for d in dims], dim=dims)


def conv_blur(x, sigma):
    """Three conv3d calls with 1-D kernels and circular padding, on (N C, 1, *sp)."""
    w = torch.from_numpy(lm.gaussian_taps(sigma)).to(x.dtype).to(x.device)
    r = (w.numel() - 1) // 2
    y = x.reshape(-1, 1, *x.shape[2:])
    for a in range(3):
        pad = [0] * 6
        pad[2 * (2 - a)] = pad[2 * (2 - a) + 1] = r
        ksh = [1, 1, 1, 1, 1]
        ksh[2 + a] = w.numel()
        y = torch.nn.functional.conv3d(torch.nn.functional.pad(y, pad, mode="circular"), w.view(ksh))
    return y.reshape(x.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shape", default="8x128")
    ap.add_argument("--sigmas", default="1,2,4")
    ap.add_argument("--only-gauss", action="store_true")
    ap.add_argument("--no-conv", action="store_true", help="leave the conv3d arms out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_gauss.py needs a GPU")
    N, S = (int(v) for v in a.shape.split("x"))
    sigmas = [float(s) for s in a.sigmas.split(",")]
    x = torch.randn((N, 3, S, S, S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    vox = x.numel()

    arms, agree = {}, {}
    for s in sigmas:
        t = f"{s:g}"
        arms[f"gauss_{t}"] = lambda s=s: lm.gaussian_smooth(x, s)
        for ax, name in enumerate("xyz"):
            sig = tuple(s if i == ax else 0.0 for i in range(3))
            arms[f"pass_{name}_{t}"] = lambda sig=sig: lm.gaussian_smooth(x, sig)
        if not a.only_gauss:
            arms[f"fft_{t}"] = lambda s=s: fft_blur(x, s)
            g = lm.gaussian_smooth(x, s)
            scale = float(g.abs().max())
            agree[t] = {"gauss_vs_fft_untruncated": float((g - fft_blur(x, s)).abs().max()) / scale}
            if not a.no_conv:
                arms[f"conv_{t}"] = lambda s=s: conv_blur(x, s)
                agree[t]["gauss_vs_conv"] = float((g - conv_blur(x, s)).abs().max()) / scale
                if agree[t]["gauss_vs_conv"] > 1e-5:
                    sys.exit(f"gaussian_smooth and the conv3d form differ at sigma = {s}: {agree[t]}")
            del g
    metric = lm.GaussianMetric(sigmas)
    arms["sharp3_acc"] = lambda: metric.sharp(x)
    if not a.only_gauss:
        def summed():
            out = lm.gaussian_smooth(x, sigmas[0])
            for s in sigmas[1:]:
                out = out + lm.gaussian_smooth(x, s)
            return out
        arms["sharp3_sum"] = summed
        if not torch.equal(metric.sharp(x), summed()):
            sys.exit("the accumulate epilogue and the torch sum give different bits")

    host = {k: [] for k in arms}

    def run(f, k=None):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        h0 = time.perf_counter()
        f()
        h1 = time.perf_counter()
        t1.record()
        t1.synchronize()
        if k is not None:
            host[k].append((h1 - h0) * 1e3)
        return t0.elapsed_time(t1)

    for _ in range(a.warmup):
        for f in arms.values():
            f()
    torch.cuda.synchronize()
    rounds = {k: [] for k in arms}
    for _ in range(a.rounds):
        times = {k: [] for k in arms}
        for _ in range(a.calls):   # alternate the arms: every pass runs each once
            for k, f in arms.items():
                times[k].append(run(f, k))
        for k, t in times.items():
            rounds[k].append(sorted(t)[len(t) // 2])
    med = {k: sorted(r)[len(r) // 2] for k, r in rounds.items()}
    spread = {k: (max(r) - min(r)) / med[k] for k, r in rounds.items()}

    def peak_fraction(k):
        passes = 3 if k.startswith("gauss_") else 1 if k.startswith("pass_") else None
        return None if passes is None else round(8.0 * vox * passes / (med[k] * 1e-3) / HBM_PEAK, 3)

    r = {"shape": f"{N}x3x{S}^3", "dtype": "float32", "mode": "wrap", "calls": a.calls, "warmup": a.warmup,
         "rounds": a.rounds, "voxels": vox,
         "median_ms": {k: round(t, 4) for k, t in med.items()},
         "round_medians_ms": {k: [round(t, 4) for t in ts] for k, ts in rounds.items()},
         "spread_of_round_medians": {k: round(s, 4) for k, s in spread.items()},
         "host_ms_in_call": {k: round(sorted(t)[len(t) // 2], 4) for k, t in host.items()},
         "fraction_of_hbm_peak": {k: peak_fraction(k) for k in med if peak_fraction(k) is not None}}
    if not a.only_gauss:
        r["max_abs_difference_over_max"] = agree
        for other in ("fft",) if a.no_conv else ("fft", "conv"):
            r[f"ratio_{other}_over_gauss"] = {f"{s:g}": round(med[f"{other}_{s:g}"] / med[f"gauss_{s:g}"], 2) for s in sigmas}
            # the worst case the rounds allow: the other form's fastest round over the new path's slowest
            r[f"ratio_{other}_over_gauss_worst_rounds"] = {
                f"{s:g}": round(min(rounds[f"{other}_{s:g}"]) / max(rounds[f"gauss_{s:g}"]), 2) for s in sigmas}
        r["ratio_sharp3_sum_over_acc"] = round(med["sharp3_sum"] / med["sharp3_acc"], 3)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
