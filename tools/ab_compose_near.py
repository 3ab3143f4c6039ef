#!/usr/bin/env python3
"""A/B of the near-identity arm of compose (lago_tuning.compose_near, csrc/fused.hip: compose3_near_kernel) on the
headline shoot (bench.py's workload: expmap, 10 Euler steps, batch 32 x 3 x 128^3, momentum scaled to a 5-voxel
deformation, default configuration), on compose alone with the fields of that shoot's last step, and -- the cost of a
wrong hint -- on compose with the smooth field of bench.py's micro_ops (batch 8, max |u| = 4 voxels) both as micro_ops
calls it (ds = -0.1: 0.4-voxel offsets) and with ds = 1 (4-voxel offsets: every tile leaves the small window).

Usage: python tools/ab_compose_near.py [rounds] [reps]
Knob off and on alternate inside one process, `rounds` times each.  Run against a library without the knob (an older
build: LAGO_HIP_LIBRARY / another checkout on PYTHONPATH) it times the "off" rounds only, so that two builds can be
alternated process by process on one machine.  One line per figure, then a JSON line with the raw rounds."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lagomorph_amd as lm
from lagomorph_amd import lddmm
from bench import gaussian_blur

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ext = lm.lagomorph_ext
has_knob = hasattr(ext, "set_compose_near")
modes = (0, 1) if has_knob else (0,)
dev = torch.device("cuda")
metric = lm.FluidMetric([0.1, 0.0, 0.01])
B, S, E = 32, 128, 10


def set_mode(mode):
    if has_knob:
        ext.set_compose_near(mode)


def timed(f, warm=2):
    for _ in range(warm):
        r = f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, r


def compose(u, v, ds, dt):
    return ext.compose(u, v, ds, dt, near_identity=True) if has_knob else ext.compose(u, v, ds, dt)


res = {k: {m: [] for m in modes} for k in ("shoot_ms", "compose_step_ms", "compose_micro_ms", "compose_4voxel_ms")}
same = {}
torch.manual_seed(1234)
with torch.no_grad():
    m = gaussian_blur(torch.randn((B, 3, S, S, S), device=dev), 4.0)
    m *= 5.0 / metric.sharp(m).abs().max()
    outs = {}
    for r in range(rounds):
        for mode in modes:
            set_mode(mode)
            t, outs[mode] = timed(lambda: lm.expmap(metric, m, num_steps=E))
            res["shoot_ms"][mode].append(t)
    same["shoot"] = all(torch.equal(outs[0], o) for o in outs.values())
    hmax = float(outs[0].abs().max())
    del outs
    # the operands of the shoot's last compose: phi_9 and v_9
    set_mode(0)
    phi, steps, _ = lddmm._shoot(metric, m, None, 1.0 / E, E - 1, None, False)
    v = metric.sharp(ext.Ad_star(phi, m))
    del m, steps
    dt = 1.0 / E
    outs = {}
    for r in range(rounds):
        for mode in modes:
            set_mode(mode)
            t, outs[mode] = timed(lambda: compose(v, phi, -dt, 1.0), warm=3)
            res["compose_step_ms"][mode].append(t)
    same["compose_step"] = all(torch.equal(outs[0], o) for o in outs.values())
    step_max = float((dt * v).abs().max())
    del outs, phi
    # micro_ops' operands: batch 8, smooth displacement with max |u| = 4 voxels
    del v
    g = torch.Generator(device=dev).manual_seed(99)
    sh = (8, 3, S, S, S)
    v = torch.randn(sh, device=dev, generator=g)
    u = gaussian_blur(torch.randn(sh, device=dev, generator=g), 8.0)
    u = u * (4.0 / u.abs().max())
    for key, ds in (("compose_micro_ms", -0.1), ("compose_4voxel_ms", 1.0)):
        outs = {}
        for r in range(rounds):
            for mode in modes:
                set_mode(mode)
                t, outs[mode] = timed(lambda: compose(u, v, ds, 1.0), warm=3)
                res[key][mode].append(t)
        same[key[:-3]] = all(torch.equal(outs[0], o) for o in outs.values())
tag = {0: "off", 1: "near"}
for name, by_mode in res.items():
    print(name + ": " + " | ".join(f"{tag[k]} " + " ".join(f"{x:.3f}" for x in xs) for k, xs in by_mode.items()), flush=True)
print(f"|h|max {hmax:.2f} voxels, max |dt v| of the last step {step_max:.3f} voxels, same bits {same}")
print(json.dumps({"knob": has_knob, "rounds": {k: {tag[m]: xs for m, xs in v.items()} for k, v in res.items()}, "same_bits": same}))
