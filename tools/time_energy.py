#!/usr/bin/env python3
"""diffusion_energy, bending_energy, energy_operator and the energies with their backward through autograd
(csrc/energy.hip) against (a) what could be written without them, a chain of torch slicing differences with torch
autograd's backward, and (b) streaming kernels of the same bytes; arms alternating in one process, HIP events around
batches of back-to-back calls; writes profiles/energy_timing.md.

    python tools/time_energy.py [--calls 20] [--batch 10] [--warmup 5] [--shape 8x3x128] [--kinds diffusion,bending] [--out profiles/energy_timing.md]

Without --one the tool is a driver: it measures every kind in a fresh child process of its own (`--one KIND`), each under
its own time limit (--limit seconds), stops at the first child that fails, and assembles the tables.  A child prints one
JSON line.

Input: a field u of N x C x S^3 float32 standard normal noise, unit spacing.  Arms:
  operator            lagomorph_amd.energy_operator(u, kind)                      loads and stores 4 N C S^3 bytes each
  energy              lagomorph_amd.field_energy(u, kind)                         loads 4 N C S^3 bytes (plus the partials)
  pair_autograd       field_energy(u, kind).sum().backward() with u.requires_grad: energy kernels + operator kernel
  torch_energy        (a) the energy from torch slicing differences, no autograd
  torch_pair          (a) the same with autograd: forward + backward
  lincomb_1           (b) lagomorph_ext.lincomb([(1.0, u)]): loads and stores 4 N C S^3 bytes each
  sum                 (b) torch.sum(u): loads 4 N C S^3 bytes
The figure of an arm is the median over --calls batches of the time of one call; a batch is --batch calls between two
device events.  --warmup passes over all arms come first.
"""
import argparse
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ARMS = ("operator", "energy", "pair_autograd", "torch_energy", "torch_pair", "lincomb_1", "sum")


def torch_energy(u, kind):
    """E (N,) at unit spacing from slicing differences: the definition, one tensor per difference."""
    d = u.dim() - 2

    def fwd(t, a):
        n = t.size(2 + a)
        return t.narrow(2 + a, 1, n - 1) - t.narrow(2 + a, 0, n - 1)

    def sec(t, a):
        n = t.size(2 + a)
        return t.narrow(2 + a, 2, n - 2) - 2 * t.narrow(2 + a, 1, n - 2) + t.narrow(2 + a, 0, n - 2)

    def ssq(t):
        return t.pow(2).flatten(1).sum(1)

    if kind == "diffusion":
        e = sum(ssq(fwd(u, a)) for a in range(d))
    else:
        e = sum(ssq(sec(u, a)) for a in range(d))
        for a, b in itertools.combinations(range(d), 2):
            e = e + 2 * ssq(fwd(fwd(u, a), b))
    return e / float(u[0, 0].numel())


def measure(a, kind):
    import torch

    sys.path.insert(0, ROOT)
    import lagomorph_amd as lm
    from lagomorph_amd import lagomorph_ext as ext

    if not torch.cuda.is_available():
        sys.exit("time_energy.py needs a GPU")
    N, C, S = (int(v) for v in a.shape.split("x"))
    gen = torch.Generator(device="cuda").manual_seed(1)
    u = torch.randn((N, C, S, S, S), device="cuda", generator=gen)
    ug = u.clone().requires_grad_(True)
    ut = u.clone().requires_grad_(True)
    buf = torch.empty_like(u)

    # the arms compute the same thing
    want = torch_energy(u, kind)
    err = float(((lm.field_energy(u, kind) - want).abs() / want).max())
    torch_energy(ut, kind).sum().backward()
    lm.field_energy(ug, kind).sum().backward()
    errb = float((ug.grad - ut.grad).abs().max() / ut.grad.abs().max())
    if err > 1e-5 or errb > 1e-5:
        sys.exit(f"field_energy / its gradient differ from the torch restatement by {err:.2e} / {errb:.2e}")

    def pair():
        ug.grad = None
        lm.field_energy(ug, kind).sum().backward()

    def torch_pair():
        ut.grad = None
        torch_energy(ut, kind).sum().backward()

    def torch_fwd():
        with torch.no_grad():
            torch_energy(u, kind)

    arms = {"operator": lambda: lm.energy_operator(u, kind), "energy": lambda: lm.field_energy(u, kind), "pair_autograd": pair,
            "torch_energy": torch_fwd, "torch_pair": torch_pair, "lincomb_1": lambda: ext.lincomb([(1.0, u)], out=buf),
            "sum": lambda: torch.sum(u)}
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
    print(json.dumps({"kind": kind, "library": os.path.basename(ext.LIB_PATH),
                      "scratch_elems": int(ext._lib.lago_field_energy_scratch_elems(0 if kind == "diffusion" else 1, 3, N, C, S, S, S)),
                      "max_rel_err": [err, errb],
                      "median_us": {k: round(1e3 * sorted(t)[len(t) // 2], 2) for k, t in times.items()},
                      "min_max_us": {k: [round(1e3 * min(t), 2), round(1e3 * max(t), 2)] for k, t in times.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default="8x3x128")
    ap.add_argument("--kinds", default="diffusion,bending")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--one", default="", help="measure this kind in this process and print one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "energy_timing.md"))
    a = ap.parse_args()
    if a.one:
        return measure(a, a.one)
    N, C, S = (int(v) for v in a.shape.split("x"))
    nbytes = 4.0 * N * C * S ** 3
    results = []
    for kind in a.kinds.split(","):   # one fresh process per kind, each under its own limit
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", kind, "--calls", str(a.calls),
               "--batch", str(a.batch), "--warmup", str(a.warmup), "--shape", a.shape]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"{kind}: exit status {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    streamed = {"operator": 2, "energy": 1, "pair_autograd": 3, "lincomb_1": 2, "sum": 1}
    text = [f"# diffusion_energy, bending_energy and energy_operator: measured times (MI355X, float32, {N} x {C} x {S}^3)", "",
            f"`python tools/time_energy.py --calls {a.calls} --batch {a.batch} --warmup {a.warmup} --shape {a.shape} --kinds {a.kinds}`"
            f" (library: {results[0]['library']}): every figure is the MEDIAN over {a.calls} timed batches of the time of one call, a batch"
            f" being {a.batch} back-to-back calls between two device events, after {a.warmup} warm-up batches of every arm; the arms"
            " alternate in one process, one fresh process per kind.  The arms are described in the tool's docstring.  GB/s counts"
            f" the algorithmic bytes only: {nbytes / 1e6:.0f} MB per streamed pass over the field (4 N C S^3), not the halo and not"
            " the energy's partial sums.", ""]
    for r in results:
        med, mm = r["median_us"], r["min_max_us"]
        text += [f"## {r['kind']}: energy scratch {4 * r['scratch_elems'] / 1e3:.1f} KB", "",
                 "| arm | median | min - max | GB/s of field bytes |", "|---|---:|---:|---:|"]
        for k in ARMS:
            rate = f"{streamed[k] * nbytes / (med[k] * 1e-6) / 1e9:.0f}" if k in streamed else ""
            text.append(f"| `{k}` | {med[k]:.1f} us | {mm[k][0]:.1f} - {mm[k][1]:.1f} us | {rate} |")
        text += ["", f"Against (b), streaming kernels of the same bytes: `operator` {med['operator'] / med['lincomb_1']:.2f} x `lincomb_1`; "
                 f"`energy` {med['energy'] / med['sum']:.2f} x `sum`.",
                 f"Against (a), the torch slicing restatement: `energy` {med['torch_energy'] / med['energy']:.1f} x faster than `torch_energy`; "
                 f"`pair_autograd` {med['torch_pair'] / med['pair_autograd']:.1f} x faster than `torch_pair` "
                 f"({med['pair_autograd'] / med['torch_pair']:.3f} of its time).",
                 f"Largest difference from the restatement: energy {r['max_rel_err'][0]:.1e} (relative), gradient {r['max_rel_err'][1]:.1e} "
                 "(of the largest magnitude).", ""]
    text += ["## Not measured", "",
             "- float64, 2D fields, anisotropic spacing (the weights are kernel arguments: the instruction count is the same), and shapes "
             "that are no multiple of the tiles.",
             "- Kernel times from a trace, LDS bank conflicts and occupancy counters: the figures are whole calls (allocation of the output "
             "and, for `energy`, of the scratch included).",
             "- The penalties inside a registration loop (with `interp`, a similarity and an optimiser).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print(json.dumps({"shape": a.shape, "calls": a.calls, "batch": a.batch, "warmup": a.warmup, "results": results}))


if __name__ == "__main__":
    main()
