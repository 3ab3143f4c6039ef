#!/usr/bin/env python3
"""mutual information: the kernels of csrc/mi.hip (joint_histogram and its backward) against the same P and gradients
from plain torch operations -- dense (voxels, B) weight matrices of the two images, one bmm, autograd for the backward;
arms alternating in one process, HIP events around every call, JSON on stdout.

    python tools/time_mi.py [--calls 20] [--warmup 5] [--shape 8x128] [--bins 32] [--skip-torch]

Inputs (N x 1 x S^3 float32, ranges passed explicitly so that no call synchronises with the host):
  smooth   a sum of slow sines and J = cos(3 I): a wave's voxels share their 16 bins, the worst same-address contention
  noise    I normal, J = cos(3 I) + 0.3 N
Arms, per input:
  mi_fwd        lagomorph_amd.joint_histogram(I, J)                         (no gradient recorded)
  torch_fwd     the same table from dense weight matrices and torch.bmm, in float64
  mi_fwdbwd     joint_histogram with both inputs requiring a gradient, then backward of sum(G P)
  torch_fwdbwd  the composition through autograd
The figure of an arm is the median over its calls.  Before anything is timed the two forms are compared: P at 1e-9
absolute (the fixed-point table is within 2^-33 of the float one), dI and dJ at 1e-5 of max|.|.
Traffic bound at 8 TB/s: the forward reads I and J once (8 bytes a voxel), the backward reads both and writes both
gradients (16 bytes a voxel); `fraction_of_traffic_bound` is bound / measured, for the forward and for forward plus
backward (24 bytes a voxel).  An event time holds the host work of the call as well as its kernels.
--skip-torch times the two kernel arms alone (A/B builds of the library, selected with LAGO_HIP_LIBRARY; kernel traces).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lagomorph_amd as lm  # noqa: E402

HBM_PEAK = 8.0e12


def dense_weights(x, rng, B):
    """(rows, voxels, B) float64: the four cubic B-spline weights of every voxel scattered into its row of bins."""
    lo, hi = rng
    rows = x.shape[0] * x.shape[1]
    s = (B - 3) / (hi - lo)
    c = (x.double().reshape(rows, -1).clamp(lo, hi) - lo) * s + 1.0
    k = (c.detach().floor().clamp(max=B - 3) - 1.0).long().clamp(0, B - 4)
    t = c - (k + 1).double()
    u = 1.0 - t
    w = torch.stack([u * u * u / 6.0, ((3.0 * t - 6.0) * t * t + 4.0) / 6.0, (((-3.0 * t + 3.0) * t + 3.0) * t + 1.0) / 6.0,
                     t * t * t / 6.0], dim=-1)
    idx = k[..., None] + torch.arange(4, device=x.device)
    return torch.zeros(c.shape + (B,), dtype=torch.float64, device=x.device).scatter(2, idx, w)


def composed(I, J, B, rI, rJ):
    """joint_histogram from plain torch operations."""
    WI, WJ = dense_weights(I, rI, B), dense_weights(J, rJ, B)
    P = torch.bmm(WI.transpose(1, 2), WJ) / WI.shape[1]
    return P.reshape(I.shape[:2] + (B, B))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default="8x128")
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mi.py needs a GPU")
    N, S = (int(v) for v in a.shape.split("x"))
    B = a.bins
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.arange(S, device="cuda", dtype=torch.float32)
    smooth = (torch.sin(0.11 * x)[:, None, None] + torch.sin(0.22 * x + 0.3)[None, :, None] + torch.sin(0.33 * x + 0.6)[None, None, :])
    smooth = (smooth[None, None] + 0.05 * torch.arange(N, device="cuda", dtype=torch.float32).reshape(N, 1, 1, 1, 1)).contiguous()
    noise = torch.randn((N, 1, S, S, S), device="cuda", generator=gen)
    pairs = {"smooth": (smooth, torch.cos(3.0 * smooth)),
             "noise": (noise, torch.cos(3.0 * noise) + 0.3 * torch.randn((N, 1, S, S, S), device="cuda", generator=gen))}
    G = torch.randn((N, 1, B, B), device="cuda", dtype=torch.float64, generator=gen)
    results = []
    for name, (I, J) in pairs.items():
        rI, rJ = tuple(float(v) for v in torch.aminmax(I)), tuple(float(v) for v in torch.aminmax(J))
        Ig, Jg = I.clone().requires_grad_(True), J.clone().requires_grad_(True)
        vox = I.numel()
        mine = lambda p, q: lm.joint_histogram(p, q, bins=B, range_I=rI, range_J=rJ)
        theirs = lambda p, q: composed(p, q, B, rI, rJ)

        def fwdbwd(f):
            Ig.grad = Jg.grad = None
            f(Ig, Jg).backward(G)
            return Ig.grad, Jg.grad

        def no_grad(f):
            with torch.no_grad():
                return f(I, J)

        arms = {"mi_fwd": lambda: no_grad(mine), "torch_fwd": lambda: no_grad(theirs),
                "mi_fwdbwd": lambda: fwdbwd(mine), "torch_fwdbwd": lambda: fwdbwd(theirs)}
        agree = None
        if a.skip_torch:
            arms = {k: f for k, f in arms.items() if k.startswith("mi_")}
        else:
            agree = {"P_abs": float((arms["mi_fwd"]() - arms["torch_fwd"]()).abs().max())}
            (xi, xj), (yi, yj) = arms["mi_fwdbwd"](), arms["torch_fwdbwd"]()
            agree["dI"] = float((xi - yi).abs().max()) / float(yi.abs().max())
            agree["dJ"] = float((xj - yj).abs().max()) / float(yj.abs().max())
            if agree["P_abs"] > 1e-9 or max(agree["dI"], agree["dJ"]) > 1e-5:
                sys.exit(f"joint_histogram and the composition differ on the {name} pair: {agree}")
            del xi, xj, yi, yj

        def run(f):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1)

        for _ in range(a.warmup):
            for f in arms.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.calls):   # alternate the arms: every pass runs each once
            for k, f in arms.items():
                times[k].append(run(f))
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
        bound_ms = {"mi_fwd": 8.0 * vox / HBM_PEAK * 1e3, "mi_fwdbwd": 24.0 * vox / HBM_PEAK * 1e3}
        results.append({
            "input": name, "shape": f"{N}x1x{S}^3", "dtype": "float32", "bins": B, "calls": a.calls, "warmup": a.warmup,
            "voxels": vox,
            "median_ms": {k: round(t, 4) for k, t in med.items()},
            "min_max_ms": {k: [round(min(t), 4), round(max(t), 4)] for k, t in times.items()},
            "backward_ms_by_difference": round(med["mi_fwdbwd"] - med["mi_fwd"], 4),
            "traffic_bound_ms": {k: round(t, 4) for k, t in bound_ms.items()},
            "fraction_of_traffic_bound": {k: round(bound_ms[k] / med[k], 4) for k in bound_ms},
            "ratio_torch_over_mi": None if a.skip_torch else {"fwd": round(med["torch_fwd"] / med["mi_fwd"], 2),
                                                              "fwdbwd": round(med["torch_fwdbwd"] / med["mi_fwdbwd"], 2)},
            "difference": agree})
        del Ig, Jg
        torch.cuda.empty_cache()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
