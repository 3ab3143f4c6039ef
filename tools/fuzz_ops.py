#!/usr/bin/env python3
"""Randomised sweep on the GPU over the operator families that tools/fuzz_parity.py does not cover: the cases,
references and judges of tests/fuzz_ops_cases.py (every family's own rule, unchanged), and on top of them

  * a second call that starts in the OTHER launch direction (the direction alternates from launch to launch, common.hpp
    next_direction; a probe launch reads it from reversed_launches() and the difference is asserted) must have the bits of
    the first for every output the family's tests call reproducible;
  * one item of a batch run alone must equal its slice of the batch, bit for bit where the family's tests assert or
    imply it and within the family's rule otherwise;
  * every third case runs again with set_vector_kernels(0) and set_launch_order(0): the same bits / the same rule.

Debug mode is on throughout, so a launch error surfaces at its call.  The first mismatch raises SystemExit with the
family, (seed, index), shape, parameters and tags; `--case` replays it.

usage: python tools/fuzz_ops.py [seconds] [seed]          the long form, the families in turn
       python tools/fuzz_ops.py --case FAMILY SEED INDEX  one case: its tags and errors"""
import os
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))
import numpy as np
import torch

import fuzz_ops_cases as fc
import lagomorph_amd as lm

ext = lm.lagomorph_ext


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def execute(c):
    """name -> tensor on the GPU: the library's outputs for the case."""
    f, p = c["family"], c["params"]
    x = {k: _dev(v) for k, v in c["inputs"].items()}
    if f == "jacobian_determinant":
        return {"forward": ext.jacobian_determinant_forward(x["u"], p["displacement"]),
                "backward": ext.jacobian_determinant_backward(x["go"], x["u"], p["displacement"])}
    if f == "invert_displacement":
        v = ext.invert_displacement_forward(x["rough"], p["rough_iters"])
        loop = -x["rough"]
        for _ in range(p["rough_iters"]):   # the unfused iteration over the existing operator
            loop = -ext.interp_forward(x["rough"], loop, 1.0)
        return {"v": ext.invert_displacement_forward(x["u"], p["iters"]), "rough": v, "rough_loop": loop,
                "lam": ext.invert_displacement_adjoint(x["go"], x["u"], _dev(fc.reference(c)["_v60"]))}
    if f == "gaussian_smooth":
        if p["form"] == "new":
            return {"out": lm.gaussian_smooth(x["x"], p["sigma"], truncate=p["truncate"], mode=p["mode"], alpha=p["alpha"])}
        taps = [lm.gaussian_taps(s, p["truncate"]) for s in p["sigma"]]
        return {"out": ext.gaussian_smooth_forward(x["x"], p["radii"], taps, p["mode"], alpha=p["alpha"], out=x["out0"],
                                                   accumulate=p["form"] == "accumulate")}
    if f == "ffd_expand":
        return {"forward": lm.ffd_expand(x["ctrl"], c["sp"], p["spacing"]), "adjoint": lm.ffd_restrict(x["g"], p["spacing"])}
    if f == "energy":
        return {"E": lm.field_energy(x["u"], p["kind"], p["spacing"]), "A": lm.energy_operator(x["u"], p["kind"], p["spacing"], scale=x.get("scale"))}
    if f == "surface_distance":
        return lm.surface_distance(x["A"], x["B"], p["labels"], p["spacing"])
    if f == "lncc":
        I, J = x["I"].requires_grad_(True), x["J"].requires_grad_(True)
        cc = lm.lncc(I, J, p["sigma"], mode=p["mode"])
        dI, dJ = torch.autograd.grad(cc, (I, J), x["g"])
        return {"cc": cc.detach(), "dI": dI, "dJ": dJ}
    if f == "bspline":
        out = {"prefilter": lm.bspline_prefilter(x["I"], adjoint=p["adjoint"]), "values": ext.interp_bspline_forward(x["C"], x["u"], p["dt"])}
        if p["need"] == "both":
            out["d_C"], out["d_u"] = ext.interp_bspline_backward(x["go"], x["C"], x["u"], p["dt"], True, True)
        else:   # each gradient alone: the other is neither computed nor written
            out["d_C"] = ext.interp_bspline_backward(x["go"], x["C"], x["u"], p["dt"], True, False)[0]
            out["d_u"] = ext.interp_bspline_backward(x["go"], x["C"], x["u"], p["dt"], False, True)[1]
        return out
    if f == "joint_histogram":
        rI, rJ = fc._mi_ranges(c)   # the backward entry point takes no automatic range
        dI, dJ = ext.mi_backward(x["G"], x["I"], x["J"], p["bins"], rI, rJ, True, True)
        return {"P": lm.joint_histogram(x["I"], x["J"], bins=p["bins"], range_I=p["range_I"], range_J=p["range_J"]), "dI": dI, "dJ": dJ}
    if f == "warp_labels":
        return {"out": lm.warp_labels(x["L"], x["u"], p["dt"], p["mode"])}
    if f == "label_overlap":
        return {"counts": lm.label_overlap(x["A"], x["B"], p["num_labels"])}
    if f == "distance_transform":
        return {"squared": lm.distance_transform(x["L"], p["where"], p["label"], p["spacing"], squared=True),
                "root": lm.distance_transform(x["L"], p["where"], p["label"], p["spacing"])}
    if f == "interp_points":
        d_F, d_x = ext.interp_points_backward(x["go"], x["F"], x["x"], True, True)
        return {"out": ext.interp_points_forward(x["F"], x["x"]), "d_x": d_x, "d_F": d_F}
    raise KeyError(f)


def _same_bits(a, b):
    """torch.equal with NaN equal to NaN (surface_distance answers nan where a surface is empty)."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def _host(outs):
    return {k: v.detach().cpu().numpy() for k, v in outs.items()}


_TINY = {}


def _probe():
    """One launch of a gather kernel; 1 if it walked its workgroups in descending order, else 0.  The launch after it
    walks the other way (common.hpp next_direction)."""
    if not _TINY:
        _TINY["I"], _TINY["u"] = torch.zeros((1, 1, 4, 4), device="cuda"), torch.zeros((1, 2, 4, 4), device="cuda")
    before = ext.reversed_launches()
    ext.interp_forward(_TINY["I"], _TINY["u"], 1.0)
    return ext.reversed_launches() - before


def check_case(c, knobs, worst=None):
    """Every failure of the case as a string."""
    f = c["family"]
    first = _probe()
    outs = execute(c)
    fails = fc.judge(f, c, _host(outs), worst)
    # the second call starts in the other launch direction than the first did: an execute() makes a number of launches
    # that depends on the family, so the probe is read, and repeated once where the parity came out the same
    second = _probe()
    if second == first:
        second = _probe()
    if second == first:
        fails.append("the launch direction did not alternate between the two calls (launch_order off?)")
    again = execute(c)
    fails += [f"{k}: a second call in the other launch direction differs" for k in fc.REPRODUCIBLE[f] if not _same_bits(again[k], outs[k])]
    if c["N"] >= 2:
        n = c["index"] % c["N"]
        sub = fc.item_case(c, n)
        alone = execute(sub)
        part = fc.item_slice(c, outs, n)
        fails += [f"{k}: item {n} alone differs from its slice of the batch" for k in fc.ITEM_BITS[f] if not _same_bits(alone[k], part[k])]
        if set(alone) - set(fc.ITEM_BITS[f]):
            fails += [f"item {n} alone: {m}" for m in fc.judge(f, sub, _host(alone))]
    if knobs:
        ext.set_vector_kernels(0)
        ext.set_launch_order(0)
        try:
            plain = execute(c)
        finally:
            ext.set_vector_kernels(1)
            ext.set_launch_order(1)
        fails += [f"{k}: differs with vector_kernels = 0 and launch_order = 0" for k in fc.REPRODUCIBLE[f] if not _same_bits(plain[k], outs[k])]
        fails += [f"vector_kernels = 0, launch_order = 0: {m}" for m in fc.judge(f, c, _host(plain))]
    return fails


def describe(c):
    return (f"{c['family']} (seed, index) = ({c['seed']}, {c['index']}) shape {c['sp']} N {c['N']} {c['dtype'].name} "
            f"inputs { {k: (v.shape, v.dtype.name) for k, v in c['inputs'].items()} } params {c['params']} tags {sorted(c['tags'])}")


def run(families=None, cases=None, budget=None, seed=0, say=None):
    """(counts, worst): counts[family] = {"judged": n, "unjudged": {reason: n}}, worst[family][output] = the largest
    fraction of its bound.  `cases`: a count, or a dict of counts per family (default: fc.COUNTS); `budget`: seconds
    instead, the families taking turns; `say`: called with a progress line about once a minute.  SystemExit at the
    first mismatch."""
    families = tuple(fc.FAMILIES if families is None else families)
    counts = {f: {"judged": 0, "unjudged": {}} for f in families}
    worst = {f: {} for f in families}
    todo = {f: (cases if isinstance(cases, int) else (cases or fc.COUNTS)[f]) for f in families} if budget is None else None
    t0, index = time.time(), 0
    told = t0
    lm.set_debug_mode(True)
    try:
        while True:
            live = [f for f in families if budget is not None or index < todo[f]]
            if not live or (budget is not None and time.time() - t0 >= budget):
                break
            if say is not None and time.time() - told >= 60.0:
                told = time.time()
                say(f"{told - t0:.0f} s: index {index}, judged {sum(n['judged'] for n in counts.values())}")
            for f in live:
                c = fc.case(f, seed, index)
                why = None
                bad = fc.valid(c)
                if bad:
                    why = "the generator made what the entry point rejects: " + ", ".join(bad)
                else:
                    try:
                        fc.reference(c)
                    except Exception as e:   # a reference that cannot be evaluated: counted, and the test wants none
                        why = f"no reference: {type(e).__name__}: {e}"
                if why is not None:
                    counts[f]["unjudged"][why] = counts[f]["unjudged"].get(why, 0) + 1
                    continue
                fails = check_case(c, knobs=index % 3 == 2, worst=worst[f])
                if fails:
                    raise SystemExit("MISMATCH " + describe(c) + ":\n  " + "\n  ".join(fails) +
                                     f"\nreplay: python tools/fuzz_ops.py --case {f} {seed} {index}")
                counts[f]["judged"] += 1
            index += 1
    finally:
        lm.set_debug_mode(False)
    return counts, worst


def report(counts, worst):
    return "\n".join(f"{f}: {n['judged']} cases judged, {sum(n['unjudged'].values())} not judged {n['unjudged'] or ''}; largest fraction "
                     f"of a bound: " + (", ".join(f"{k} {v:.3g}" for k, v in sorted(worst[f].items())) or "(bit for bit only)")
                     for f, n in counts.items())


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        family, seed, index = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        c = fc.case(family, seed, index)
        print(describe(c))
        lm.set_debug_mode(True)
        w = {}
        fails = check_case(c, knobs=True, worst=w)
        print("fractions of the bounds:", w)
        print("\n".join(fails) if fails else "no mismatch")
        sys.exit(1 if fails else 0)
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    counts, worst = run(budget=budget, seed=seed, say=lambda line: print(line, flush=True))
    print(f"{budget:.0f} s, seed {seed}, no mismatch")
    print(report(counts, worst))
