#!/usr/bin/env python3
"""jacobian_determinant: the fused kernels against what the public operators offered before them, and against their
stencil siblings, alternating the arms in one process (HIP events around every call; JSON on stdout).

    python tools/time_jacdet.py [--calls 50] [--warmup 10] [--shapes 8x128,8x160] [--only-fused]

Arms per shape (N x 3 x S^3 float32, smooth displacement of 3 voxels amplitude):
  fused_fwd / fused_fwd_bwd    lagomorph_amd.jacobian_determinant (and .backward)
  composed_fwd / composed_fwd_bwd
                               three jacobian_times_vectorfield(u, e_a) calls, stack / permute, torch.linalg.det (and its
                               autograd backward)
  jtv_fwd, jtv_bwd             lagomorph_ext.jacobian_times_vectorfield_forward(u, w) / _backward on the same box
--only-fused runs the two fused kernels alone (a target for `rocprofv3 --kernel-trace --stats`).
Algorithmic bytes per voxel: forward 16 (three components read, one scalar written), backward 28 (u and grad_out read,
d_u written); the shares of HBM peak in the output use these over the event time of the call (kernel time from a
profiler run of its own is a little shorter).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
import lagomorph_amd as lm  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (MI355X)


def smooth(shape, sigma, seed, amp):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = bench.gaussian_blur(torch.randn(shape, device="cuda", generator=g), sigma)
    return (x * (amp / x.abs().max())).contiguous()


def composed(u, units):
    cols = [lm.jacobian_times_vectorfield(u, e, True, False) for e in units]   # cols[a][:, c] = J[c][a]
    J = torch.stack(cols, dim=-1)                                               # (N, c, sp..., a)
    return torch.linalg.det(J.permute(0, 2, 3, 4, 1, 5))[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shapes", default="8x128,8x160")
    ap.add_argument("--only-fused", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_jacdet.py needs a GPU")
    ext = lm.lagomorph_ext
    results = []
    for spec in a.shapes.split(","):
        N, S = (int(x) for x in spec.split("x"))
        u = smooth((N, 3, S, S, S), 8.0, 1, 3.0)
        w = smooth((N, 3, S, S, S), 4.0, 2, 1.0)
        go = torch.randn((N, 1, S, S, S), device="cuda")
        go3 = torch.randn((N, 3, S, S, S), device="cuda")
        units = []
        for d in range(3):
            e = torch.zeros_like(u)
            e[:, d] = 1
            units.append(e)
        ug = u.clone().requires_grad_(True)

        def fused_fwd_bwd():
            ug.grad = None
            lm.jacobian_determinant(ug).backward(go)

        def composed_fwd_bwd():
            ug.grad = None
            composed(ug, units).backward(go)

        arms = {
            "fused_fwd": lambda: ext.jacobian_determinant_forward(u, True),
            "fused_bwd": lambda: ext.jacobian_determinant_backward(go, u, True),
            "fused_fwd_bwd": fused_fwd_bwd,
        }
        if not a.only_fused:
            arms.update({
                "composed_fwd": lambda: composed(u, units),
                "composed_fwd_bwd": composed_fwd_bwd,
                "jtv_fwd": lambda: ext.jacobian_times_vectorfield_forward(u, w, True, False),
                "jtv_bwd": lambda: ext.jacobian_times_vectorfield_backward(go3, u, w, True, False, True, True),
            })
            # same numbers first: the composed route against the fused one
            want = composed(u, units)
            got = ext.jacobian_determinant_forward(u, True)
            dev_fwd = float((got - want).abs().max() / want.abs().max())

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
        for _ in range(a.calls):   # alternate the arms: every round runs each once
            for k, f in arms.items():
                times[k].append(run(f))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        vox = N * S ** 3
        r = {"shape": f"{N}x3x{S}^3", "dtype": "float32", "calls": a.calls, "warmup": a.warmup,
             "median_ms": {k: round(v, 4) for k, v in med.items()},
             "min_ms": {k: round(min(v), 4) for k, v in times.items()},
             "hbm_share_fwd_16B": round(16 * vox / (med["fused_fwd"] * 1e-3) / HBM_PEAK, 3),
             "hbm_share_bwd_28B": round(28 * vox / (med["fused_bwd"] * 1e-3) / HBM_PEAK, 3)}
        if not a.only_fused:
            r["composed_vs_fused_max_rel_dev"] = dev_fwd
            r["ratio_composed_over_fused_fwd"] = round(med["composed_fwd"] / med["fused_fwd"], 2)
            r["ratio_composed_over_fused_fwd_bwd"] = round(med["composed_fwd_bwd"] / med["fused_fwd_bwd"], 2)
            r["ratio_fused_fwd_over_jtv_fwd"] = round(med["fused_fwd"] / med["jtv_fwd"], 3)
            r["ratio_fused_bwd_over_jtv_bwd"] = round(med["fused_bwd"] / med["jtv_bwd"], 3)
        results.append(r)
        del units, u, w, go, go3, ug
        torch.cuda.empty_cache()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
