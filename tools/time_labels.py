#!/usr/bin/env python3
"""warp_labels and label_overlap (csrc/labels.hip) against their yardsticks, arms alternating in one process, HIP events
around batches of back-to-back calls, JSON on stdout.

    python tools/time_labels.py [--calls 20] [--batch 20] [--warmup 3] [--shape 8x128] [--labels 200] [--only warp|overlap] [--skip-torch]

Inputs (N x S^3, float32 displacement):
  blobs    a segmentation of K labels in structures about S / 16 voxels across (a coarse random label grid, enlarged and
           carried through a smooth deformation): the interior of a structure is most of the volume
  random   every voxel its own random label: the vote runs on every voxel, no two lanes of a wave agree
  zeros    all background
  u        a smooth displacement of up to three voxels
Arms:
  warp_vote_<input>, warp_nearest_<input>   lagomorph_ext.warp_labels(L, u)
  interp_c1                                 lagomorph_ext.interp_forward of a one-channel float32 image with the same u: the
                                            same algorithmic bytes (12 of u, 4 out, 4 in per voxel)
  overlap_<input>                           lagomorph_ext.label_overlap(A, B, K), B = A carried through u
  bincount_<input>                          torch.bincount(A * K + B, minlength = K * K) per item, the same counts from torch
The figure of an arm is the median over --calls batches of the time of one call (a batch is --batch calls between two
events, so the host's work per call is hidden wherever the device is the slower of the two; one call for the bincount
arms, which take milliseconds).  --skip-torch leaves the bincount arms out (A/B builds).  Traffic bounds at 8 TB/s:
20 bytes a voxel for the warp and interp_c1, 8 for the overlap.  Select an A/B build of the library with LAGO_HIP_LIBRARY.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lagomorph_amd as lm  # noqa: E402
from lagomorph_amd import lagomorph_ext as ext  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", default="8x128")
    ap.add_argument("--labels", type=int, default=200)
    ap.add_argument("--only", choices=("warp", "overlap"), default=None)
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_labels.py needs a GPU")
    N, S = (int(v) for v in a.shape.split("x"))
    K = a.labels
    sp = (S, S, S)
    gen = torch.Generator(device="cuda").manual_seed(1)
    up = lambda x, mode: torch.nn.functional.interpolate(x, size=sp, mode=mode, **({} if mode == "nearest" else {"align_corners": True}))
    u = (3.0 * up(torch.rand((N, 3, 6, 6, 6), device="cuda", generator=gen) * 2 - 1, "trilinear")).contiguous()
    coarse = torch.randint(0, K, (N, 1, 16, 16, 16), device="cuda", generator=gen)
    coarse[:, :, :2] = 0   # some background
    blobs = lm.warp_labels(up(coarse.float(), "nearest").to(torch.int32).contiguous(), u.flip(1).contiguous(), 2.0)
    maps = {"blobs": blobs, "random": torch.randint(0, K, (N, 1) + sp, device="cuda", generator=gen, dtype=torch.int32),
            "zeros": torch.zeros((N, 1) + sp, device="cuda", dtype=torch.int32)}
    img = torch.randn((N, 1) + sp, device="cuda", generator=gen)
    vox = N * S ** 3
    arms, bound, info = {}, {}, {}
    if a.only != "overlap":
        for name in ("blobs", "random"):
            for mode in ("vote", "nearest"):
                arms[f"warp_{mode}_{name}"] = (lambda L, m: lambda: ext.warp_labels(L, u, 1.0, m))(maps[name], mode)
                bound[f"warp_{mode}_{name}"] = 20.0 * vox / HBM_PEAK * 1e3
        arms["interp_c1"] = lambda: ext.interp_forward(img, u, 1.0)
        bound["interp_c1"] = 20.0 * vox / HBM_PEAK * 1e3
        w = ext.warp_labels(blobs, u, 1.0, "vote")
        info["voxels_changed_by_the_warp_of_blobs"] = round(float((w != blobs).float().mean()), 4)
        c = blobs[0, 0]
        edge = (c[1:, 1:, 1:] != c[:-1, :-1, :-1]) | (c[1:, 1:, 1:] != c[:-1, 1:, 1:]) | (c[1:, 1:, 1:] != c[1:, :-1, 1:]) | (c[1:, 1:, 1:] != c[1:, 1:, :-1])
        info["blob_voxels_next_to_another_label"] = round(float(edge.float().mean()), 4)
    if a.only != "warp":
        for name, A in maps.items():
            B = ext.warp_labels(A, u, 1.0, "vote")
            arms[f"overlap_{name}"] = (lambda p, q: lambda: ext.label_overlap(p, q, K))(A, B)
            bound[f"overlap_{name}"] = 8.0 * vox / HBM_PEAK * 1e3
            if a.skip_torch:
                continue
            A64, B64 = A.reshape(N, -1).long(), B.reshape(N, -1).long()
            torch_counts = lambda p=A64, q=B64: torch.stack([torch.bincount(p[n] * K + q[n], minlength=K * K) for n in range(N)])
            arms[f"bincount_{name}"] = torch_counts
            joint = torch_counts().reshape(N, K, K)   # the two forms agree before anything is timed
            want = torch.stack([joint.sum(2), joint.sum(1), joint.diagonal(dim1=1, dim2=2)], -1)
            if not torch.equal(ext.label_overlap(A, B, K), want):
                sys.exit(f"label_overlap and torch.bincount differ on the {name} pair")

    def run(k, f):
        batch = 1 if k.startswith("bincount") else a.batch   # (milliseconds a call: the host does not show)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(batch):
            f()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / batch

    for _ in range(a.warmup):
        for k, f in arms.items():
            run(k, f)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.calls):   # alternate the arms: every pass runs a batch of each
        for k, f in arms.items():
            times[k].append(run(k, f))
    med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
    print(json.dumps({
        "shape": f"{N}x{S}^3", "labels": K, "calls": a.calls, "batch": a.batch, "warmup": a.warmup, "voxels": vox,
        "library": os.path.basename(ext.LIB_PATH), **info,
        "median_us": {k: round(1e3 * t, 2) for k, t in med.items()},
        "min_max_us": {k: [round(1e3 * min(t), 2), round(1e3 * max(t), 2)] for k, t in times.items()},
        "traffic_bound_us": {k: round(1e3 * t, 2) for k, t in bound.items()},
        "fraction_of_traffic_bound": {k: round(bound[k] / med[k], 4) for k in bound}}))


if __name__ == "__main__":
    main()
