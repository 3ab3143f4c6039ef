#!/usr/bin/env python3
"""ffd_expand, ffd_restrict and the pair through autograd (csrc/ffd.hip) against (a) what can be written without them,
three dense contractions with the per-axis matrices W_a on the GPU, and (b) streaming kernels of the same bytes; arms
alternating in one process, HIP events around batches of back-to-back calls; writes profiles/ffd_timing.md.

    python tools/time_ffd.py [--calls 20] [--batch 10] [--warmup 5] [--shape 8x3x128] [--spacings 4,8] [--out profiles/ffd_timing.md]

Without --one the tool is a driver: it measures every spacing in a fresh child process of its own (`--one S`), each under
its own time limit (--limit seconds), stops at the first child that fails, and assembles the tables.  A child prints one
JSON line.

Inputs: a control lattice of N x C x m^3 float32 standard normal noise, m = (S - 1) // s + 4, and a field g of
N x C x S^3 noise.  Arms:
  expand              lagomorph_ext.ffd_expand(c, shape, s)                      stores 4 N C S^3 bytes
  restrict            lagomorph_ext.ffd_expand_adjoint(g, s)                     loads 4 N C S^3 bytes (plus the partials)
  pair_autograd       lagomorph_amd.ffd_expand(c) with c.requires_grad, .backward(g): forward + adjoint through autograd
  dense_fwd           (a) three torch.einsum contractions with dense W_z, W_y, W_x (S x m, float32) on the GPU
  dense_pair          (a) the same with autograd: forward + backward
  lincomb_1           (b) lagomorph_ext.lincomb([(1.0, x)]): loads and stores 4 N C S^3 bytes each
  fill                (b) out.fill_(1.0): stores 4 N C S^3 bytes and loads nothing
  sum                 (b) torch.sum(g): loads 4 N C S^3 bytes
The figure of an arm is the median over --calls batches of the time of one call; a batch is --batch calls between two
device events.  --warmup passes over all arms come first.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ARMS = ("expand", "restrict", "pair_autograd", "dense_fwd", "dense_pair", "lincomb_1", "fill", "sum")


def dense_w(n, s, device):
    """The (n, m) float32 matrix of one axis, built with torch from the definition (t = r / s in float32)."""
    import torch

    x = torch.arange(n, device=device)
    t = (x % s).to(torch.float32) / float(s)
    u = 1 - t
    w = torch.stack([u ** 3, 3 * t ** 3 - 6 * t ** 2 + 4, -3 * t ** 3 + 3 * t ** 2 + 3 * t + 1, t ** 3], 1) / 6
    W = torch.zeros((n, (n - 1) // s + 4), device=device)
    W.scatter_(1, (x // s)[:, None] + torch.arange(4, device=device)[None, :], w)
    return W


def measure(a, s):
    import torch

    sys.path.insert(0, ROOT)
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    if not torch.cuda.is_available():
        sys.exit("time_ffd.py needs a GPU")
    N, C, S = (int(v) for v in a.shape.split("x"))
    shape = (S, S, S)
    m = lm.ffd_grid_shape(shape, s)
    gen = torch.Generator(device="cuda").manual_seed(1)
    c = torch.randn((N, C) + m, device="cuda", generator=gen)
    g = torch.randn((N, C) + shape, device="cuda", generator=gen)
    W = dense_w(S, s, "cuda")
    cg = c.clone().requires_grad_(True)
    cd = c.clone().requires_grad_(True)
    buf = torch.empty_like(g)

    def dense(x):
        x = torch.einsum("zc,nkabc->nkabz", W, x)
        x = torch.einsum("yb,nkabz->nkayz", W, x)
        return torch.einsum("xa,nkayz->nkxyz", W, x)

    # the arms compute the same thing
    want = dense(c)
    err = float((ext.ffd_expand(c, shape, s) - want).abs().max() / want.abs().max())
    cd.grad = None
    dense(cd).backward(g)
    errb = float((ext.ffd_expand_adjoint(g, s) - cd.grad).abs().max() / cd.grad.abs().max())
    if err > 1e-5 or errb > 1e-4:
        sys.exit(f"ffd_expand / ffd_restrict differ from the dense contractions by {err:.2e} / {errb:.2e}")

    def pair():
        cg.grad = None
        lm.ffd_expand(cg, shape, s).backward(g)

    def dense_pair():
        cd.grad = None
        dense(cd).backward(g)

    def dense_fwd():
        with torch.no_grad():
            dense(c)

    arms = {"expand": lambda: ext.ffd_expand(c, shape, s), "restrict": lambda: ext.ffd_expand_adjoint(g, s), "pair_autograd": pair,
            "dense_fwd": dense_fwd, "dense_pair": dense_pair, "lincomb_1": lambda: ext.lincomb([(1.0, g)], out=buf),
            "fill": lambda: buf.fill_(1.0), "sum": lambda: torch.sum(g)}
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
    print(json.dumps({"spacing": s, "lattice": list(m), "library": os.path.basename(ext.LIB_PATH),
                      "scratch_elems": int(ext._lib.lago_ffd_scratch_elems(3, N * C, S, S, S, s, s, s)),
                      "max_rel_err": [err, errb],
                      "median_us": {k: round(1e3 * sorted(t)[len(t) // 2], 2) for k, t in times.items()},
                      "min_max_us": {k: [round(1e3 * min(t), 2), round(1e3 * max(t), 2)] for k, t in times.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default="8x3x128")
    ap.add_argument("--spacings", default="4,8")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--one", type=int, default=0, help="measure this spacing in this process and print one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffd_timing.md"))
    a = ap.parse_args()
    if a.one:
        return measure(a, a.one)
    N, C, S = (int(v) for v in a.shape.split("x"))
    nbytes = 4.0 * N * C * S ** 3
    results = []
    for s in (int(v) for v in a.spacings.split(",")):   # one fresh process per spacing, each under its own limit
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(s), "--calls", str(a.calls),
               "--batch", str(a.batch), "--warmup", str(a.warmup), "--shape", a.shape]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"spacing {s}: exit status {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    streamed = {"expand": 1, "restrict": 1, "pair_autograd": 2, "lincomb_1": 2, "fill": 1, "sum": 1}
    text = [f"# ffd_expand and ffd_restrict: measured times (MI355X, float32, {N} x {C} x {S}^3)", "",
            f"`python tools/time_ffd.py --calls {a.calls} --batch {a.batch} --warmup {a.warmup} --shape {a.shape} --spacings {a.spacings}`"
            f" (library: {results[0]['library']}): every figure is the MEDIAN over {a.calls} timed batches of the time of one call, a batch"
            f" being {a.batch} back-to-back calls between two device events, after {a.warmup} warm-up batches of every arm; the arms"
            " alternate in one process, one fresh process per spacing.  The arms are described in the tool's docstring.  GB/s counts"
            f" the algorithmic bytes only: {nbytes / 1e6:.0f} MB per streamed pass over the field (4 N C S^3), not the lattice and not"
            " the adjoint's partial sums.", ""]
    for r in results:
        med, mm = r["median_us"], r["min_max_us"]
        text += [f"## spacing {r['spacing']}: lattice {' x '.join(str(v) for v in r['lattice'])}, adjoint scratch "
                 f"{4 * r['scratch_elems'] / 1e6:.1f} MB", "", "| arm | median | min - max | GB/s of field bytes |", "|---|---:|---:|---:|"]
        for k in ARMS:
            rate = f"{streamed[k] * nbytes / (med[k] * 1e-6) / 1e9:.0f}" if k in streamed else ""
            text.append(f"| `{k}` | {med[k]:.1f} us | {mm[k][0]:.1f} - {mm[k][1]:.1f} us | {rate} |")
        text += ["", f"Against (a), the dense contractions: `expand` {med['dense_fwd'] / med['expand']:.2f} x faster than `dense_fwd` "
                 f"({med['expand'] / med['dense_fwd']:.3f} of its time); `pair_autograd` {med['dense_pair'] / med['pair_autograd']:.2f} x "
                 "faster than `dense_pair`.",
                 f"Against (b), streaming kernels of the same bytes: `expand` {med['expand'] / med['fill']:.2f} x `fill` and "
                 f"{med['expand'] / med['lincomb_1']:.2f} x `lincomb_1` (which also loads what it stores); `restrict` "
                 f"{med['restrict'] / med['sum']:.2f} x `sum`, i.e. `fill` runs in {med['fill'] / med['expand']:.2f} and `sum` in "
                 f"{med['sum'] / med['restrict']:.2f} of their times.",
                 f"Largest difference from the dense contractions: forward {r['max_rel_err'][0]:.1e}, adjoint {r['max_rel_err'][1]:.1e} "
                 "(of the largest magnitude).", ""]
    text += ["## Not measured", "",
             "- float64, 2D fields, spacings other than the above (s = 1 and s = 2 stage much larger LDS boxes and write much larger partials), "
             "anisotropic spacings, and shapes that are no multiple of the tiles.",
             "- Kernel times from a trace, LDS bank conflicts and the split of the adjoint between its tile kernel and its sum kernel: the figures "
             "are whole calls (allocation of the output and, for `restrict`, of the scratch included).",
             "- The same operators inside a registration loop (`interp` of the expanded field, a similarity, an optimiser).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print(json.dumps({"shape": a.shape, "calls": a.calls, "batch": a.batch, "warmup": a.warmup, "results": results}))


if __name__ == "__main__":
    main()
