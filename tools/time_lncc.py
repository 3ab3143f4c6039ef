#!/usr/bin/env python3
"""lncc: the kernels of csrc/lncc.hip against the composition from public ops a user had before them -- three torch
products, five gaussian_smooth calls, torch elementwise, autograd for the backward; arms alternating in one process, HIP
events around every call, JSON on stdout.

    python tools/time_lncc.py [--calls 20] [--warmup 5] [--rounds 3] [--shapes 2x128,8x128] [--sigma 2.0]

Arms (N x 1 x S^3 float32, periodic border), per shape:
  lncc_fwd        lagomorph_amd.lncc(I, J, sigma)                              (no gradient recorded)
  composed_fwd    the same map from gaussian_smooth and torch
  lncc_fwdbwd     lncc with both inputs requiring a gradient, then backward of sum(g cc)
  composed_fwdbwd the composition through autograd
Every round times each arm `calls` times, the arms taking turns; the figure of a round is the median over its calls, and
the spread quoted is that of the rounds' medians ((max - min) / median).  Before anything is timed the two forms are
compared at 1e-4 of max|.| (cc, dI and dJ; both are float32 evaluations of the same formula).
Traffic bound: the volumes the new path has to move per field, 4 bytes x voxels each, at 8 TB/s --
  forward  7 (moments pass) + 20 (two stacked passes) + 6 (cc)                                              = 33
  backward 11 (five moments, g in; five fields out) + 30 (three stacked passes) + 9 (five fields, I, J in; dI, dJ out) = 50
`fraction_of_traffic_bound` is bound / measured.  The GPU is idle when the first event is recorded, so an event time
holds the host work of the call as well as its kernels; `host_ms_in_call` is the median wall time the host spends inside
the call.
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
FWD_VOLUMES, BWD_VOLUMES = 33, 50


def composed(I, J, sigma, eps=1e-5):
    """lncc from the public ops of the parent commit."""
    G = lambda x: lm.gaussian_smooth(x, sigma)
    A, B, C, D, E = G(I), G(J), G(I * I), G(I * J), G(J * J)
    sI, sJ, sX = C - A * A, E - B * B, D - A * B
    return sX * sX / (sI * sJ + eps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="2x128,8x128")
    ap.add_argument("--sigma", type=float, default=2.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_lncc.py needs a GPU")
    results = []
    for shape in a.shapes.split(","):
        N, S = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device="cuda").manual_seed(1)
        I = torch.randn((N, 1, S, S, S), device="cuda", generator=gen)
        J = 0.8 * I + 0.6 * torch.randn((N, 1, S, S, S), device="cuda", generator=gen)
        g = torch.randn((N, 1, S, S, S), device="cuda", generator=gen)
        Ig, Jg = I.clone().requires_grad_(True), J.clone().requires_grad_(True)
        vox = I.numel()

        def fwdbwd(f):
            Ig.grad = Jg.grad = None
            f(Ig, Jg, a.sigma).backward(g)
            return Ig.grad, Jg.grad

        def no_grad(f):
            with torch.no_grad():
                return f(I, J, a.sigma)

        arms = {"lncc_fwd": lambda: no_grad(lm.lncc), "composed_fwd": lambda: no_grad(composed),
                "lncc_fwdbwd": lambda: fwdbwd(lm.lncc), "composed_fwdbwd": lambda: fwdbwd(composed)}
        agree = {}
        x, y = arms["lncc_fwd"](), arms["composed_fwd"]()
        agree["cc"] = float((x - y).abs().max()) / float(y.abs().max())
        (xi, xj), (yi, yj) = arms["lncc_fwdbwd"](), arms["composed_fwdbwd"]()
        agree["dI"] = float((xi - yi).abs().max()) / float(yi.abs().max())
        agree["dJ"] = float((xj - yj).abs().max()) / float(yj.abs().max())
        if max(agree.values()) > 1e-4:
            sys.exit(f"lncc and the composition differ at {shape}: {agree}")
        del x, y, xi, xj, yi, yj

        host = {k: [] for k in arms}

        def run(f, k):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            h0 = time.perf_counter()
            f()
            h1 = time.perf_counter()
            t1.record()
            t1.synchronize()
            host[k].append((h1 - h0) * 1e3)
            return t0.elapsed_time(t1)

        for _ in range(a.warmup):
            for f in arms.values():
                f()
        torch.cuda.synchronize()
        host = {k: [] for k in arms}
        rounds = {k: [] for k in arms}
        for _ in range(a.rounds):
            times = {k: [] for k in arms}
            for _ in range(a.calls):   # alternate the arms: every pass runs each once
                for k, f in arms.items():
                    times[k].append(run(f, k))
            for k, t in times.items():
                rounds[k].append(sorted(t)[len(t) // 2])
        med = {k: sorted(r)[len(r) // 2] for k, r in rounds.items()}
        bound_ms = {"lncc_fwd": FWD_VOLUMES * 4.0 * vox / HBM_PEAK * 1e3,
                    "lncc_fwdbwd": (FWD_VOLUMES + BWD_VOLUMES) * 4.0 * vox / HBM_PEAK * 1e3}
        results.append({
            "shape": f"{N}x1x{S}^3", "dtype": "float32", "mode": "wrap", "sigma": a.sigma, "calls": a.calls,
            "warmup": a.warmup, "rounds": a.rounds, "voxels": vox,
            "median_ms": {k: round(t, 4) for k, t in med.items()},
            "round_medians_ms": {k: [round(t, 4) for t in ts] for k, ts in rounds.items()},
            "spread_of_round_medians": {k: round((max(r) - min(r)) / med[k], 4) for k, r in rounds.items()},
            "host_ms_in_call": {k: round(sorted(t)[len(t) // 2], 4) for k, t in host.items()},
            "traffic_bound_ms": {k: round(t, 4) for k, t in bound_ms.items()},
            "fraction_of_traffic_bound": {k: round(bound_ms[k] / med[k], 3) for k in bound_ms},
            "ratio_composed_over_lncc": {"fwd": round(med["composed_fwd"] / med["lncc_fwd"], 3),
                                         "fwdbwd": round(med["composed_fwdbwd"] / med["lncc_fwdbwd"], 3)},
            # the worst case the rounds allow: the composition's fastest round over the new path's slowest
            "ratio_composed_over_lncc_worst_rounds": {
                "fwd": round(min(rounds["composed_fwd"]) / max(rounds["lncc_fwd"]), 3),
                "fwdbwd": round(min(rounds["composed_fwdbwd"]) / max(rounds["lncc_fwdbwd"]), 3)},
            "max_abs_difference_over_max": agree})
        del I, J, g, Ig, Jg
        torch.cuda.empty_cache()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
