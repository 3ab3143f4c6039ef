#!/usr/bin/env python3
"""invert_displacement: the fused fixed-point kernel against the same iteration written with the operators the library
had before it, and the backward (adjoint solve + splat) against the splat alone; arms alternating in one process, HIP
events around every call, JSON on stdout.

    python tools/time_invert.py [--calls 30] [--warmup 5] [--rounds 3] [--shape 8x128] [--iters 5,10,20] [--only-fused]

Arms (N x 3 x S^3 float32, smooth displacement of amplitude 2 voxels):
  fused_K      lagomorph_ext.invert_displacement_forward(u, K)
  loop_K       v = -u, then K times v = -lagomorph_ext.interp_forward(u, v, 1.0)   (2K + 1 launches)
  bwd          invert_displacement_adjoint + interp_backward(need_I): the backward of InvertDisplacementFunction
  splat        interp_backward(need_I) alone on the same fields
Every round times each arm `calls` times, the arms taking turns; the figure of a round is the median over its calls,
and the spread quoted is that of the rounds' medians ((max - min) / median).  The fused result is compared with the
loop's bit for bit before anything is timed.  --only-fused runs the fused arms alone (a target for
`rocprofv3 --kernel-trace --stats`).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
import lagomorph_amd as lm  # noqa: E402


def smooth(shape, sigma, seed, amp):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = bench.gaussian_blur(torch.randn(shape, device="cuda", generator=g), sigma)
    return (x * (amp / x.abs().max())).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shape", default="8x128")
    ap.add_argument("--iters", default="5,10,20")
    ap.add_argument("--only-fused", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_invert.py needs a GPU")
    ext = lm.lagomorph_ext
    N, S = (int(x) for x in a.shape.split("x"))
    iters = [int(k) for k in a.iters.split(",")]
    u = smooth((N, 3, S, S, S), 8.0, 1, 2.0)
    go = torch.randn((N, 3, S, S, S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))

    def loop(K):
        v = -u
        for _ in range(K):
            v = -ext.interp_forward(u, v, 1.0)
        return v

    v = ext.invert_displacement_forward(u, max(iters))
    residual = {}
    arms = {}
    for K in iters:
        arms[f"fused_{K}"] = lambda K=K: ext.invert_displacement_forward(u, K)
        if not a.only_fused:
            arms[f"loop_{K}"] = lambda K=K: loop(K)
            vk = ext.invert_displacement_forward(u, K)
            if not torch.equal(vk, loop(K)):
                sys.exit(f"fused and unfused results differ at iters = {K}")
            residual[K] = float(lm.compose(vk, u).abs().max())
    arms["bwd"] = lambda: ext.interp_backward(ext.invert_displacement_adjoint(go, u, v), u, v, 1.0, True, False)
    if not a.only_fused:
        arms["splat"] = lambda: ext.interp_backward(go, u, v, 1.0, True, False)

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
    rounds = {k: [] for k in arms}
    for _ in range(a.rounds):
        times = {k: [] for k in arms}
        for _ in range(a.calls):   # alternate the arms: every pass runs each once
            for k, f in arms.items():
                times[k].append(run(f))
        for k, t in times.items():
            rounds[k].append(sorted(t)[len(t) // 2])
    med = {k: sorted(r)[len(r) // 2] for k, r in rounds.items()}
    spread = {k: (max(r) - min(r)) / med[k] for k, r in rounds.items()}
    r = {"shape": f"{N}x3x{S}^3", "dtype": "float32", "calls": a.calls, "warmup": a.warmup, "rounds": a.rounds,
         "max_abs_u": float(u.abs().max()),
         "median_ms": {k: round(t, 4) for k, t in med.items()},
         "round_medians_ms": {k: [round(t, 4) for t in ts] for k, ts in rounds.items()},
         "spread_of_round_medians": {k: round(s, 4) for k, s in spread.items()}}
    if not a.only_fused:
        r["residual_max_abs"] = {str(K): residual[K] for K in iters}
        r["ratio_loop_over_fused"] = {str(K): round(med[f"loop_{K}"] / med[f"fused_{K}"], 2) for K in iters}
        # the worst case the rounds allow: the loop's fastest round over the fused kernel's slowest
        r["ratio_loop_over_fused_worst_rounds"] = {
            str(K): round(min(rounds[f"loop_{K}"]) / max(rounds[f"fused_{K}"]), 2) for K in iters}
        r["ratio_bwd_over_splat"] = round(med["bwd"] / med["splat"], 3)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
