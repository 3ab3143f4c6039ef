#!/usr/bin/env python3
"""pyramid_reduce, pyramid_expand and their transposes (csrc/pyramid.hip) against (a) what could be written without
them, (b) torch's pooling and interpolation and (c) a copy of the same algorithmic bytes; arms alternating in one
process, HIP events around batches of back-to-back calls; writes profiles/pyramid_timing.md.

    python tools/time_pyramid.py [--calls 20] [--batch 10] [--warmup 5] [--shapes 8x3x128,8x1x160] [--out profiles/pyramid_timing.md]

Without --one the tool is a driver: it measures every shape in a fresh child process of its own (`--one SHAPE`), each
under its own time limit (--limit seconds), stops at the first child that fails, and assembles the tables.  A child
prints one JSON line.

Input: a fine field I of N x C x S^3 float32 uniform noise and a coarse field c of N x C x (S/2)^3.  V = N C S^3.  Arms:
  reduce              lagomorph_amd.pyramid_reduce(I)                          loads 4 V bytes, stores 4 V / 8
  expand_adjoint      lagomorph_amd.pyramid_expand_adjoint(I)                  the same kernel with the other matrix
  expand              lagomorph_amd.pyramid_expand(c, shape, 2.0)              loads 4 V / 8 bytes, stores 4 V
  restrict_adjoint    lagomorph_amd.pyramid_restrict_adjoint(c, shape)         the same kernel with the other matrix
  smooth_slice        (a) gaussian_smooth(I, sigma=1, mode="zero")[..., ::2, ::2, ::2].contiguous()
  regrid              (a) regrid(c, shape=shape): the multilinear gather to the fine grid
  avg_pool            (b) F.avg_pool3d(I, 2)
  interpolate         (b) F.interpolate(c, size=shape, mode="trilinear", align_corners=True)
  copy                (c) copy_ of 9 V / 16 elements: loads and stores 4 V (1 + 1/8) bytes in all, as one pyramid kernel
The figure of an arm is the median over --calls batches of the time of one call; a batch is --batch calls between two
device events.  --warmup passes over all arms come first.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ARMS = ("reduce", "expand_adjoint", "expand", "restrict_adjoint", "smooth_slice", "regrid", "avg_pool", "interpolate", "copy")
OURS = ARMS[:4]


def measure(a, shape):
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ROOT)
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    if not torch.cuda.is_available():
        sys.exit("time_pyramid.py needs a GPU")
    N, C, S = (int(v) for v in shape.split("x"))
    fine = (S, S, S)
    gen = torch.Generator(device="cuda").manual_seed(1)
    I = torch.rand((N, C) + fine, device="cuda", generator=gen)
    c = torch.rand((N, C) + lm.pyramid_shape(fine), device="cuda", generator=gen)
    n_copy = 9 * I.numel() // 16
    src, dst = torch.rand(n_copy, device="cuda", generator=gen), torch.empty(n_copy, device="cuda")

    # the arms compute comparable things: away from the border, avg_pool and the smoothed slice are other low-pass
    # filters of the same field, and regrid / interpolate of a ramp are the ramp (corner-aligned, so only for odd S)
    err = float((lm.pyramid_reduce(torch.ones_like(I)) - 1).abs().max() + (lm.pyramid_expand(torch.ones_like(c), fine, 2.0) - 2).abs().max())
    if err != 0.0:
        sys.exit(f"constants are not preserved: {err:.2e}")

    arms = {"reduce": lambda: lm.pyramid_reduce(I), "expand_adjoint": lambda: lm.pyramid_expand_adjoint(I),
            "expand": lambda: lm.pyramid_expand(c, fine, 2.0), "restrict_adjoint": lambda: lm.pyramid_restrict_adjoint(c, fine),
            "smooth_slice": lambda: lm.gaussian_smooth(I, 1.0, mode="zero")[..., ::2, ::2, ::2].contiguous(),
            "regrid": lambda: lm.regrid(c, shape=fine),
            "avg_pool": lambda: F.avg_pool3d(I, 2), "interpolate": lambda: F.interpolate(c, size=fine, mode="trilinear", align_corners=True),
            "copy": lambda: dst.copy_(src)}
    assert tuple(arms) == ARMS

    def run(f):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.batch):
            f()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.batch

    for _ in range(a.warmup):
        for f in arms.values():
            run(f)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.calls):   # alternate the arms: every pass runs a batch of each
        for k, f in arms.items():
            times[k].append(run(f))
    print(json.dumps({"shape": shape, "library": os.path.basename(ext.LIB_PATH),
                      "median_us": {k: round(1e3 * sorted(t)[len(t) // 2], 2) for k, t in times.items()},
                      "min_max_us": {k: [round(1e3 * min(t), 2), round(1e3 * max(t), 2)] for k, t in times.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="8x3x128,8x1x160")
    ap.add_argument("--limit", type=int, default=200, help="seconds a child may take")
    ap.add_argument("--one", default="", help="measure this shape in this process and print one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_timing.md"))
    a = ap.parse_args()
    if a.one:
        return measure(a, a.one)
    results = []
    for shape in a.shapes.split(","):   # one fresh process per shape, each under its own limit
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", shape, "--calls", str(a.calls),
               "--batch", str(a.batch), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"{shape}: exit status {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    text = ["# pyramid_reduce, pyramid_expand and their transposes: measured times (MI355X, float32)", "",
            f"`python tools/time_pyramid.py --calls {a.calls} --batch {a.batch} --warmup {a.warmup} --shapes {a.shapes}`"
            f" (library: {results[0]['library']}): every figure is the MEDIAN over {a.calls} timed batches of the time of one call, a batch"
            f" being {a.batch} back-to-back calls between two device events, after {a.warmup} warm-up batches of every arm; the arms"
            " alternate in one process, one fresh process per shape.  The arms are described in the tool's docstring.  GB/s counts"
            " the algorithmic bytes only, 4 V (1 + 1/8) for V = N C S^3 fine voxels: one pass over the fine field and one over the"
            " coarse one, not the halo.  Whole calls: the allocation of the output is included.", ""]
    for r in results:
        N, C, S = (int(v) for v in r["shape"].split("x"))
        nbytes = 4.0 * N * C * S ** 3 * 9 / 8
        med, mm = r["median_us"], r["min_max_us"]
        text += [f"## {N} x {C} x {S}^3: {nbytes / 1e6:.0f} MB per call", "",
                 "| arm | median | min - max | GB/s of algorithmic bytes | of the copy's rate |", "|---|---:|---:|---:|---:|"]
        for k in ARMS:
            ours = k in OURS or k == "copy"
            rate = f"{nbytes / (med[k] * 1e-6) / 1e9:.0f}" if ours else ""
            frac = f"{med['copy'] / med[k]:.2f}" if ours else ""
            text.append(f"| `{k}` | {med[k]:.1f} us | {mm[k][0]:.1f} - {mm[k][1]:.1f} us | {rate} | {frac} |")
        text += ["", f"Against (a), what the parent commit offers: `reduce` {med['smooth_slice'] / med['reduce']:.1f} x faster than `smooth_slice`; "
                 f"`expand` {med['regrid'] / med['expand']:.1f} x faster than `regrid`.",
                 f"Against (b), torch: `reduce` {med['avg_pool'] / med['reduce']:.2f} x the speed of `avg_pool`; `expand` "
                 f"{med['interpolate'] / med['expand']:.2f} x the speed of `interpolate`.",
                 f"Against (c), a copy of the same bytes: `reduce` {med['reduce'] / med['copy']:.2f} x its time, `expand_adjoint` "
                 f"{med['expand_adjoint'] / med['copy']:.2f} x, `expand` {med['expand'] / med['copy']:.2f} x, `restrict_adjoint` "
                 f"{med['restrict_adjoint'] / med['copy']:.2f} x.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print(json.dumps({"shapes": a.shapes, "calls": a.calls, "batch": a.batch, "warmup": a.warmup, "results": results}))


if __name__ == "__main__":
    main()
