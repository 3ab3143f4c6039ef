#!/usr/bin/env python3
"""interp_points, its backward and deform_points (csrc/points.hip) against interp on the same samples, arms alternating
in one process, HIP events around batches of back-to-back calls; writes the tables of profiles/points_timing.md.

    python tools/time_points.py [--calls 20] [--batch 10] [--warmup 5] [--shape 8x128] [--channels 1,3] [--out profiles/points_timing.md]

Inputs: F of N x C x S^3 float32 standard normal noise, a smooth displacement u of up to three voxels.
Point sets (N, 3, P):
  a   identity + u in grid order, P = S^3: the samples `interp(F, u)` takes, so the two are compared like for like (12
      bytes of position replace 12 bytes of u; the outputs are compared bit for bit before anything is timed)
  b   the same positions randomly permuted (one permutation per item)
  c   P = 100000 per item, uniform random in the grid: landmark and mesh scale
Arms, per channel count C:
  fwd_<set>                      lagomorph_ext.interp_points_forward(F, x)
  interp                         lagomorph_ext.interp_forward(F, u): the slab-unrolled kernel at C = 1, the LDS window at C >= 2
  interp_plain                   the same with the LDS window switched off (C >= 2): the slab-unrolled pair-gather kernel
  bwd_<set>_F / _x / _Fx         lagomorph_ext.interp_points_backward(g, F, x, need_F, need_x)
  interp_bwd_I / _u / _Iu        lagomorph_ext.interp_backward(g, F, u, 1.0, need_I, need_u) on the samples of set a (d_I
                                 through the LDS-privatised splat kernels)
  interp_bwd_I_global            the same with splat_mode 0: d_I by eight global float atomics per sample and channel, the form
                                 interp_points_backward has
  deform_a, deform_a_half,       deform_points(x, w) with dt = 1 (one elementwise pass: x + (.)) and dt = -0.5 (two: the product
  deform_a_interp                and the sum), and interp_points(w, x) alone, w a displacement field (C = 3 only)
The figure of an arm is the median over --calls batches of the time of one call; a batch is --batch calls between two
device events, so the host's work per call is hidden wherever the device is the slower of the two.  --warmup passes over
all arms come first.  "Of HBM peak" (set a only) is the algorithmic traffic over the time against 8 TB/s: per point 12
bytes of position (or of u), 4 C of output and 4 C for reading every voxel of F once.
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

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default="8x128")
    ap.add_argument("--channels", default="1,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_timing.md"))
    a = ap.parse_args()
    if a.calls < 20 or a.warmup < 5:
        sys.exit("time_points.py: at least 20 timed calls and 5 warm-ups")
    if not torch.cuda.is_available():
        sys.exit("time_points.py needs a GPU")
    N, S = (int(v) for v in a.shape.split("x"))
    sp = (S, S, S)
    nvox = S ** 3
    gen = torch.Generator(device="cuda").manual_seed(1)
    coarse = torch.rand((N, 3, 6, 6, 6), device="cuda", generator=gen) * 2 - 1
    u = (3.0 * torch.nn.functional.interpolate(coarse, size=sp, mode="trilinear", align_corners=True)).contiguous()
    ident = torch.from_numpy(lm.identity((1, 3) + sp)).cuda()
    xa = (ident + u).reshape(N, 3, nvox).contiguous()
    perm = torch.stack([torch.randperm(nvox, device="cuda", generator=gen) for _ in range(N)])
    xb = torch.gather(xa, 2, perm[:, None, :].expand(N, 3, nvox)).contiguous()
    Pc = 100000
    xc = (torch.rand((N, 3, Pc), device="cuda", generator=gen) * (S - 1)).contiguous()
    sets = {"a": xa, "b": xb, "c": xc}
    sections, results = [], {}
    for C in (int(c) for c in a.channels.split(",")):
        F = torch.randn((N, C) + sp, device="cuda", generator=gen)
        got, want = ext.interp_points_forward(F, xa), ext.interp_forward(F, u, 1.0).reshape(N, C, nvox)
        if not torch.equal(got, want):
            sys.exit(f"interp_points and interp differ on set a (C = {C})")
        arms, nbytes = {}, {}
        for k, x in sets.items():
            arms[f"fwd_{k}"] = (lambda x: lambda: ext.interp_points_forward(F, x))(x)
        arms["interp"] = lambda: ext.interp_forward(F, u, 1.0)
        nbytes["fwd_a"] = nbytes["interp"] = (12 + 8 * C) * N * nvox
        if C >= 2:
            arms["interp_plain"] = lambda: ext.interp_forward(F, u, 1.0)
            nbytes["interp_plain"] = nbytes["interp"]
        need = {"F": (True, False), "x": (False, True), "Fx": (True, True)}
        for k, x in sets.items():
            g = torch.randn((N, C, x.size(2)), device="cuda", generator=gen)
            for tag, (nf, nx) in need.items():
                arms[f"bwd_{k}_{tag}"] = (lambda g, x, nf, nx: lambda: ext.interp_points_backward(g, F, x, nf, nx))(g, x, nf, nx)
        g3 = torch.randn((N, C) + sp, device="cuda", generator=gen)
        for tag, (nf, nx) in zip(("I", "u", "Iu"), need.values()):
            arms[f"interp_bwd_{tag}"] = (lambda nf, nx: lambda: ext.interp_backward(g3, F, u, 1.0, nf, nx))(nf, nx)
        arms["interp_bwd_I_global"] = lambda: ext.interp_backward(g3, F, u, 1.0, True, False)
        if C == 3:
            arms["deform_a"] = lambda: lm.deform_points(xa, F)
            arms["deform_a_half"] = lambda: lm.deform_points(xa, F, -0.5)
            arms["deform_a_interp"] = lambda: lm.interp_points(F, xa)

        def run(k, f):
            if k == "interp_plain":
                ext.set_gather_window(0)
            if k == "interp_bwd_I_global":
                ext.set_splat_mode(0)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.batch):
                f()
            t1.record()
            t1.synchronize()
            if k == "interp_plain":
                ext.set_gather_window(1)
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
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
        results[f"C{C}"] = {"median_us": {k: round(1e3 * t, 2) for k, t in med.items()},
                            "min_max_us": {k: [round(1e3 * min(t), 2), round(1e3 * max(t), 2)] for k, t in times.items()}}
        rows = [f"## {N} x {C} x {S}^3 float32", "",
                "| arm | points per item | median | min - max | of HBM peak |", "|---|---:|---:|---:|---:|"]
        for k in arms:
            pts = sets[k.split("_")[1]].size(2) if k.startswith(("fwd_", "bwd_")) else nvox
            frac = f"{nbytes[k] / (med[k] * 1e-3) / HBM_PEAK:.2f}" if k in nbytes else ""
            rows.append(f"| `{k}` | {pts} | {1e3 * med[k]:.1f} us | {1e3 * min(times[k]):.1f} - {1e3 * max(times[k]):.1f} us | {frac} |")
        rows += ["", f"`fwd_a` / `interp`: {med['fwd_a'] / med['interp']:.2f}" +
                 (f"; `fwd_a` / `interp_plain`: {med['fwd_a'] / med['interp_plain']:.2f}" if C >= 2 else " (at C = 1 `interp` is the plain kernel)") +
                 f"; `fwd_b` / `fwd_a`: {med['fwd_b'] / med['fwd_a']:.2f}.",
                 "Backward, set a, against `interp_backward`: " +
                 ", ".join(f"`bwd_a_{p}` / `interp_bwd_{q}` {med['bwd_a_' + p] / med['interp_bwd_' + q]:.2f}"
                           for p, q in (("F", "I"), ("F", "I_global"), ("x", "u"), ("Fx", "Iu"))) + "."]
        if C == 3:
            for k, what in (("deform_a", "dt = 1, the elementwise `x + (.)`"), ("deform_a_half", "dt = -0.5, the elementwise `x + dt * (.)`")):
                extra = med[k] - med["deform_a_interp"]
                rows.append(f"`deform_points`, set a, {what}: {1e3 * med[k]:.1f} us, of which the elementwise part is "
                            f"{1e3 * extra:.1f} us ({100 * extra / med[k]:.0f} %).")
        sections.append("\n".join(rows))
    head = [f"# interp_points: measured times (MI355X, float32, {N} x C x {S}^3)", "",
            f"`python tools/time_points.py --calls {a.calls} --batch {a.batch} --warmup {a.warmup} --shape {a.shape} --channels {a.channels}`: "
            f"every figure is the MEDIAN over {a.calls} timed batches of the time of one call, a batch being {a.batch} back-to-back "
            f"calls between two device events, after {a.warmup} warm-up batches of every arm; the arms alternate in one process, "
            "`interp` and `interp_backward` among them (unchanged from the parent commit).  Point sets: a = identity + u in grid "
            "order (the samples `interp(F, u)` takes; outputs compared bit for bit before timing), b = the same positions randomly "
            f"permuted, c = {Pc} uniform random positions per item.  `_F` / `_x` / `_Fx`: the gradients wanted.  \"Of HBM peak\": "
            "(12 + 8 C) bytes per point -- position or u, output, every voxel of F read once -- over the time, against 8 TB/s.", ""]
    text = "\n".join(head) + "\n" + "\n\n".join(sections) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"shape": f"{N}x{S}^3", "calls": a.calls, "batch": a.batch, "warmup": a.warmup,
                      "library": os.path.basename(ext.LIB_PATH), **results}))


if __name__ == "__main__":
    main()
