#!/usr/bin/env python3
"""bspline_prefilter, interp_bspline and its backward (csrc/bspline.hip) against gaussian_smooth, interp and
interp_backward at the same shape, arms alternating in one process, HIP events around batches of back-to-back calls;
writes the tables of profiles/bspline_timing.md.

    python tools/time_bspline.py [--calls 20] [--batch 10] [--warmup 5] [--shape 8x128] [--channels 1,3] [--out profiles/bspline_timing.md]

Inputs: I of N x C x S^3 float32 standard normal noise; a SMOOTH displacement of up to three voxels (trilinear
upsampling of 6^3 uniform noise) and a RANDOM one (independent uniform +-3 voxels per voxel and component).
Arms, per channel count C:
  prefilter, prefilter_adj   lagomorph_ext.bspline_prefilter(I, adjoint): three passes (x, y, z)
  prefilter_yz, prefilter_z  the same call on the tensor viewed as (N C S, 1, 1, S, S) and (N C S S, 1, 1, 1, S): extents
                             of 1 are skipped, so these are the (y, z) passes and the z pass alone on the same memory with
                             the same launches; x = prefilter - prefilter_yz and y = prefilter_yz - prefilter_z are
                             DERIVED (the passes run back to back on one stream; the tensor fits the Infinity Cache at
                             C = 1, so a pass alone may find more of its input cached than inside the full call)
  gauss, gauss_x/_y/_z       lagomorph_ext.gaussian_smooth_forward with sigma = 2 on all axes / on one axis (mode wrap)
  fwd_smooth, fwd_random     lagomorph_ext.interp_bspline_forward(C, u, 1.0)
  fwd_*_nogather             the same with the tap loads removed (profiling build only: lago_debug_bspline_gather(0);
                             results are wrong): forward minus this is the time of the 64 gathers
  interp_smooth/_random      lagomorph_ext.interp_forward(I, u, 1.0)
  cubic_smooth               lagomorph_amd.interp_cubic(I, u): prefilter + forward
  bwd_C / bwd_u / bwd_Cu     lagomorph_ext.interp_bspline_backward(g, C, u, 1.0, need_C, need_u), smooth u
  interp_bwd_I / _u          lagomorph_ext.interp_backward(g, I, u, 1.0, ...) (d_I through the LDS-privatised splat)
  interp_bwd_I_global        the same with splat_mode 0: d_I by eight global float atomics per voxel and channel
The figure of an arm is the median over --calls batches of the time of one call; a batch is --batch calls between two
device events.  --warmup passes over all arms come first.  A prefilter pass moves 8 bytes per element (one load, one
store): its two-stream floor is 8 N C S^3 bytes over the achieved streaming rate; the tables give the achieved GB/s.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import lagomorph_amd as lm  # noqa: E402
from lagomorph_amd import lagomorph_ext as ext  # noqa: E402
from lagomorph_amd.smooth import gaussian_taps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default="8x128")
    ap.add_argument("--channels", default="1,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bspline_timing.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_bspline.py needs a GPU")
    N, S = (int(v) for v in a.shape.split("x"))
    sp = (S, S, S)
    nvox = S ** 3
    gen = torch.Generator(device="cuda").manual_seed(1)
    coarse = torch.rand((N, 3, 6, 6, 6), device="cuda", generator=gen) * 2 - 1
    fields = {"smooth": (3.0 * torch.nn.functional.interpolate(coarse, size=sp, mode="trilinear", align_corners=True)).contiguous(),
              "random": (6.0 * torch.rand((N, 3) + sp, device="cuda", generator=gen) - 3.0).contiguous()}
    knob = getattr(ext._lib, "lago_debug_bspline_gather", None)   # profiling build only
    sections, results = [], {}
    for C in (int(c) for c in a.channels.split(",")):
        I = torch.randn((N, C) + sp, device="cuda", generator=gen)
        Cf = ext.bspline_prefilter(I)
        g = torch.randn((N, C) + sp, device="cuda", generator=gen)
        u = fields["smooth"]
        back = ext.interp_bspline_forward(Cf, torch.zeros_like(u), 1.0)
        err = float((back - I).abs().max() / I.abs().max())
        if err > 1e-5:
            sys.exit(f"interp_cubic(I, 0) differs from I by {err:.2e} max|I|")
        arms = {"prefilter": lambda: ext.bspline_prefilter(I), "prefilter_adj": lambda: ext.bspline_prefilter(I, True),
                "prefilter_yz": lambda: ext.bspline_prefilter(I.view(N * C * S, 1, 1, S, S)),
                "prefilter_z": lambda: ext.bspline_prefilter(I.view(N * C * S * S, 1, 1, 1, S))}
        taps2 = gaussian_taps(2.0)
        one = gaussian_taps(0.0)
        r2 = (len(taps2) - 1) // 2
        for tag, on in (("gauss", (1, 1, 1)), ("gauss_x", (1, 0, 0)), ("gauss_y", (0, 1, 0)), ("gauss_z", (0, 0, 1))):
            radii = [r2 if o else 0 for o in on]
            taps = [taps2 if o else one for o in on]
            arms[tag] = (lambda radii, taps: lambda: ext.gaussian_smooth_forward(I, radii, taps, "wrap"))(radii, taps)
        for k, uu in fields.items():
            arms[f"fwd_{k}"] = (lambda uu: lambda: ext.interp_bspline_forward(Cf, uu, 1.0))(uu)
            if knob is not None:
                arms[f"fwd_{k}_nogather"] = arms[f"fwd_{k}"]
            arms[f"interp_{k}"] = (lambda uu: lambda: ext.interp_forward(I, uu, 1.0))(uu)
        arms["cubic_smooth"] = lambda: lm.interp_cubic(I, u)
        need = {"C": (True, False), "u": (False, True), "Cu": (True, True)}
        for tag, (nc_, nu_) in need.items():
            arms[f"bwd_{tag}"] = (lambda nc_, nu_: lambda: ext.interp_bspline_backward(g, Cf, u, 1.0, nc_, nu_))(nc_, nu_)
        arms["interp_bwd_I"] = lambda: ext.interp_backward(g, I, u, 1.0, True, False)
        arms["interp_bwd_u"] = lambda: ext.interp_backward(g, I, u, 1.0, False, True)
        arms["interp_bwd_I_global"] = arms["interp_bwd_I"]

        def run(k, f):
            if k.endswith("_nogather"):
                knob(0)
            if k == "interp_bwd_I_global":
                ext.set_splat_mode(0)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.batch):
                f()
            t1.record()
            t1.synchronize()
            if k.endswith("_nogather"):
                knob(1)
            if k == "interp_bwd_I_global":
                ext.set_splat_mode(1)
            return t0.elapsed_time(t1) / a.batch

        with torch.no_grad():
            for _ in range(a.warmup):
                for k, f in arms.items():
                    run(k, f)
            torch.cuda.synchronize()
            times = {k: [] for k in arms}
            for _ in range(a.calls):   # alternate the arms: every pass runs a batch of each
                for k, f in arms.items():
                    times[k].append(run(k, f))
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}   # ms
        results[f"C{C}"] = {"median_us": {k: round(1e3 * t, 2) for k, t in med.items()},
                            "min_max_us": {k: [round(1e3 * min(t), 2), round(1e3 * max(t), 2)] for k, t in times.items()}}
        passbytes = 8.0 * N * C * nvox
        stream = {"prefilter": 3, "prefilter_adj": 3, "prefilter_yz": 2, "prefilter_z": 1, "gauss": 3, "gauss_x": 1,
                  "gauss_y": 1, "gauss_z": 1}
        rows = [f"## {N} x {C} x {S}^3 float32", "", "| arm | median | min - max | GB/s at 8 B per element and pass |",
                "|---|---:|---:|---:|"]
        for k in arms:
            rate = f"{stream[k] * passbytes / (med[k] * 1e-3) / 1e9:.0f}" if k in stream else ""
            rows.append(f"| `{k}` | {1e3 * med[k]:.1f} us | {1e3 * min(times[k]):.1f} - {1e3 * max(times[k]):.1f} us | {rate} |")
        px, py, pz = med["prefilter"] - med["prefilter_yz"], med["prefilter_yz"] - med["prefilter_z"], med["prefilter_z"]
        rows += ["", "Prefilter passes (x and y derived by subtraction): " +
                 ", ".join(f"{n} {1e3 * t:.1f} us = {passbytes / (t * 1e-3) / 1e9:.0f} GB/s, {t / med['gauss_' + n]:.2f} x `gauss_{n}`"
                           for n, t in (("x", px), ("y", py), ("z", pz))) +
                 f"; all three {med['prefilter'] / med['gauss']:.2f} x `gauss`.",
                 "Forward against `interp`: " + ", ".join(f"{k} {med['fwd_' + k] / med['interp_' + k]:.2f} x" for k in fields) + "."]
        if knob is not None:
            rows.append("The 64 gathers (forward minus the forward without its tap loads): " +
                        ", ".join(f"{k} {1e3 * (med['fwd_' + k] - med['fwd_' + k + '_nogather']):.1f} of {1e3 * med['fwd_' + k]:.1f} us "
                                  f"({100 * (1 - med['fwd_' + k + '_nogather'] / med['fwd_' + k]):.0f} %)" for k in fields) + ".")
        rows.append("Backward: " + ", ".join(f"`bwd_{p}` / `interp_bwd_{q}` {med['bwd_' + p] / med['interp_bwd_' + q]:.2f}"
                                              for p, q in (("C", "I_global"), ("C", "I"), ("u", "u"))) + ".")
        sections.append("\n".join(rows))
    head = [f"# Cubic B-spline interpolation: measured times (MI355X, float32, {N} x C x {S}^3)", "",
            f"`python tools/time_bspline.py --calls {a.calls} --batch {a.batch} --warmup {a.warmup} --shape {a.shape} --channels {a.channels}`"
            f" (library: {os.path.basename(ext.LIB_PATH)}): every figure is the MEDIAN over {a.calls} timed batches of the time of one "
            f"call, a batch being {a.batch} back-to-back calls between two device events, after {a.warmup} warm-up batches of every "
            "arm; the arms alternate in one process, `gaussian_smooth`, `interp` and `interp_backward` among them (unchanged from "
            "the parent commit).  smooth = a displacement of up to three voxels upsampled from 6^3 noise, random = independent "
            "uniform +-3 voxels.  The arms are described in the tool's docstring.", ""]
    text = "\n".join(head) + "\n" + "\n\n".join(sections) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"shape": f"{N}x{S}^3", "calls": a.calls, "batch": a.batch, "warmup": a.warmup,
                      "library": os.path.basename(ext.LIB_PATH), **results}))


if __name__ == "__main__":
    main()
