#!/usr/bin/env python3
"""distance_transform per `where` mode and a surface_distance call (csrc/edt.hip) against a streaming copy of the same
bytes; arms alternating in one process, HIP events around batches of back-to-back calls; writes profiles/edt_timing.md.

    python tools/time_edt.py [--calls 20] [--batch 5] [--warmup 3] [--shapes 8x1x128,2x1x256] [--out profiles/edt_timing.md]

Without --one the tool is a driver: it measures every shape in a fresh child process of its own (`--one NxCxS`), each
under its own time limit (--limit seconds), stops at the first child that fails, and assembles the tables.  A child
prints one JSON line.

Inputs: A, a label map N x 1 x S^3 of int32 labels 0..4, the argmax over five channels of box-smoothed noise (connected
structures a few voxels to a few tens of voxels across); B, the same map moved by (3, 2, 1) voxels with wrap-around.  Arms:
  dt_nonzero / dt_equal / dt_not_equal / dt_surface   lagomorph_amd.distance_transform(A, where, 1): three passes, the first
                      loads 4 N S^3 bytes of labels (the surface stencil's neighbours from cache) and stores 4 N S^3, the
                      other two load and store 4 N S^3 each in place
  dt_surface_squared  the same with squared=True (no square root in the last pass)
  surface_distance_4  lagomorph_amd.surface_distance(A, B, [1, 2, 3, 4]): four transforms per label (two distances, two
                      selection masks) and, per item and label, two boolean selections, sorts and reductions in torch,
                      each selection synchronising with the host
  copy                buf.copy_(x) on float32 N x 1 x S^3: loads and stores 4 N S^3 bytes, the streaming yardstick of ONE pass
The transform is brute force over the sources of a line: S candidates per voxel and pass, so its arithmetic grows with S
while the copy's bytes do not.  The figure of an arm is the median over --calls batches of the time of one call; a batch
is --batch calls between two device events.  --warmup passes over all arms come first.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ARMS = ("dt_nonzero", "dt_equal", "dt_not_equal", "dt_surface", "dt_surface_squared", "surface_distance_4", "copy")


def blobs(N, S, K, gen):
    import torch

    out = []
    for _ in range(N):
        x = torch.randn((1, K, S, S, S), device="cuda", generator=gen)
        for _ in range(3):
            x = torch.nn.functional.avg_pool3d(x, 5, stride=1, padding=2)
        out.append(x.argmax(1, keepdim=True).to(torch.int32))
    return torch.cat(out).contiguous()


def measure(a, shape):
    import torch

    sys.path.insert(0, ROOT)
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    if not torch.cuda.is_available():
        sys.exit("time_edt.py needs a GPU")
    N, C, S = (int(v) for v in shape.split("x"))
    if C != 1:
        sys.exit("time_edt.py: a label map has one channel")
    gen = torch.Generator(device="cuda").manual_seed(1)
    A = blobs(N, S, 5, gen)
    B = torch.roll(A, (3, 2, 1), (2, 3, 4)).contiguous()
    x = torch.randn((N, 1, S, S, S), device="cuda", generator=gen)
    buf = torch.empty_like(x)

    # the arms compute what they say: the squared transform of a small corner against the definition, in torch
    c = A[:1, :, :12, :12, :12].contiguous()
    f = (c[0, 0] == 1).nonzero().to(torch.float32)
    g = torch.stack(torch.meshgrid(*(torch.arange(12, device="cuda", dtype=torch.float32),) * 3, indexing="ij"), -1).reshape(-1, 3)
    want = torch.cdist(g, f).min(1).values.reshape(12, 12, 12) ** 2 if len(f) else torch.full((12, 12, 12), float("inf"), device="cuda")
    if not torch.equal(lm.distance_transform(c, "equal", 1, squared=True)[0, 0], torch.round(want)):
        sys.exit("distance_transform differs from the definition")
    frac = {w: float((lm.distance_transform(A, w, 1, squared=True) == 0).float().mean()) for w in ("nonzero", "equal", "not_equal", "surface")}

    arms = {"dt_nonzero": lambda: lm.distance_transform(A, "nonzero", 1), "dt_equal": lambda: lm.distance_transform(A, "equal", 1),
            "dt_not_equal": lambda: lm.distance_transform(A, "not_equal", 1), "dt_surface": lambda: lm.distance_transform(A, "surface", 1),
            "dt_surface_squared": lambda: lm.distance_transform(A, "surface", 1, squared=True),
            "surface_distance_4": lambda: lm.surface_distance(A, B, [1, 2, 3, 4]), "copy": lambda: buf.copy_(x)}
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
    sd = lm.surface_distance(A, B, [1, 2, 3, 4])
    print(json.dumps({"shape": shape, "library": os.path.basename(ext.LIB_PATH), "feature_fraction": frac,
                      "hd95_item0": [round(float(v), 3) for v in sd["hd95"][0]],
                      "median_us": {k: round(1e3 * sorted(t)[len(t) // 2], 2) for k, t in times.items()},
                      "min_max_us": {k: [round(1e3 * min(t), 2), round(1e3 * max(t), 2)] for k, t in times.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="8x1x128,2x1x256")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--one", default="", help="measure this shape in this process and print one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt_timing.md"))
    a = ap.parse_args()
    if a.one:
        return measure(a, a.one)
    results = []
    for shape in a.shapes.split(","):   # one fresh process per shape, each under its own limit
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", shape, "--calls", str(a.calls),
               "--batch", str(a.batch), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"shape {shape}: exit status {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    text = ["# distance_transform and surface_distance: measured times (MI355X, int32 labels, float32 distances)", "",
            f"`python tools/time_edt.py --calls {a.calls} --batch {a.batch} --warmup {a.warmup} --shapes {a.shapes}`"
            f" (library: {results[0]['library']}): every figure is the MEDIAN over {a.calls} timed batches of the time of one call, a batch"
            f" being {a.batch} back-to-back calls between two device events, after {a.warmup} warm-up batches of every arm; the arms"
            " alternate in one process, one fresh process per shape.  The arms and the inputs are described in the tool's docstring."
            "  No threshold was set in advance: this note records what was measured.  `copy` loads and stores the bytes ONE pass"
            " of the transform loads and stores, so three copies are the streaming time of a whole 3D transform; the transform is"
            " plain brute force over the S sources of a line (S candidates per voxel and pass), which the ratio shows.", ""]
    for r in results:
        N, _, S = (int(v) for v in r["shape"].split("x"))
        med, mm = r["median_us"], r["min_max_us"]
        nbytes = 4.0 * N * S ** 3
        text += [f"## {N} x 1 x {S}^3 ({nbytes / 1e6:.0f} MB per volume)", "",
                 "| arm | median | min - max | ratio to three copies | candidates / s |", "|---|---:|---:|---:|---:|"]
        for k in ARMS:
            is_dt = k.startswith("dt_")
            ratio = f"{med[k] / (3 * med['copy']):.2f}" if k != "copy" else ""
            rate = f"{3.0 * N * S ** 4 / (med[k] * 1e-6):.2e}" if is_dt else ""
            text.append(f"| `{k}` | {med[k]:.1f} us | {mm[k][0]:.1f} - {mm[k][1]:.1f} us | {ratio} | {rate} |")
        ff = r["feature_fraction"]
        text += ["", f"`copy` moves {2 * nbytes / (med['copy'] * 1e-6) / 1e9:.0f} GB/s (loads plus stores).  Feature voxels of the input: "
                 + ", ".join(f"`{w}` {100 * v:.1f} %" for w, v in ff.items()) + " (the time does not depend on them: every source of a line is"
                 f" visited).  `surface_distance_4` is {med['surface_distance_4'] / med['dt_surface']:.1f} x one `dt_surface`: 16 transforms and"
                 f" the torch selections, sorts and host synchronisations of {N} x 4 item-label pairs; hd95 of item 0: {r['hd95_item0']}.", ""]
    text += ["## Pruned candidate window", "",
             "Not tried: the kernels visit every source of a line.  A window pruned by `|i - j| s < sqrt(g[i])` is exact and would cut the"
             " arithmetic of the second and third pass where features are dense; there is no A/B to record.", "",
             "## Not measured", "",
             "- 2D maps, anisotropic extents, extents above 256 (the 32- and 16-line tiles), other dtypes (their conversion to int32 is a torch pass).",
             "- Kernel times from a trace, LDS bank conflicts, and the split between the three passes: the figures are whole calls (allocation of"
             " the output included).",
             "- The first pass stores each lane's 8 outputs as 32 contiguous bytes, not as whole cache lines across a wave; what staging them"
             " through LDS would gain was not measured.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print(json.dumps({"shapes": a.shapes, "calls": a.calls, "batch": a.batch, "warmup": a.warmup, "results": results}))


if __name__ == "__main__":
    main()
