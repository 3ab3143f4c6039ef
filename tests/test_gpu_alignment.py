"""GPU: every tensor-taking entry point of lagomorph_ext on tensors that start off the vector alignment.

The library takes raw data pointers of any contiguous tensor.  Its kernels treat a base that is only element-aligned in
three ways ("Alignment contract"): a host-side gate sends it to a sibling kernel; the kernel needs element
alignment only (pair loads, row tiles, splat flush rows); or a row is cut into a scalar head, vectors and a scalar tail.
Every other test hands the library 16-byte aligned tensors, so the siblings behind the gates, a gate that tests the wrong
pointer, and a store that rounds its address down would all go unseen.

Each case of the table below is one call with its tensor arguments, its reference and its expected path.  `run_case`

 1. runs the call on offset-0 views (tests/offset_views.py: the control goes through the same helper) and judges the
    control against the reference the op's own test uses;
 2. runs it with each tensor argument in turn, and all of them together, 1, 2 and 3 elements past a 16-byte boundary
    (plus one run with two arguments at different offsets where the case names a pair);
 3. wants the bits of the control wherever no atomic and no FFT is involved;
 4. judges scatter-adds and FFT results against the reference by `assert_close` of tests/test_gpu_parity.py -- the
    fluid metric too: its float32 bound is the one of tests/test_gpu_dispatch.py, its float64 bound the tighter 1e-12;
 5. wants every margin bit of every argument's buffer untouched and no NaN (no poison label) in any output;
 6. wants the path counters to say what the gates say: the fast path in the control, the sibling when the gated pointer
    is off, no change otherwise.

Shapes are the smallest that reach each path (tests/test_gpu_launch_arms.py, tests/test_gpu_dispatch.py)."""
import functools
import inspect
import itertools
import json
import os

import numpy as np
import pytest
import torch

import bspline_ref
import edt_ref
import ffd_ref
import gauss_ref
import gpu_util
import invert_ref
import jacdet_ref
import labels_ref
import lncc_ref
import mi_ref
import points_ref
from offset_views import OFFSETS, margins_intact, offset_view, poisoned
from oracle import lago_oracle as orc
from gpu_util import OBSERVED, assert_close, dev, displacement, host, rnd

pytestmark = pytest.mark.gpu
assert_bits = functools.partial(gpu_util.assert_bits, check_dtype=False)   # these sites compare shape and bits, as they always did

F32, F64 = torch.float32, torch.float64
BOTH = (F32, F64)
NP = {F32: np.float32, F64: np.float64}
PARAMS = [0.1, 0.05, 0.01]


@pytest.fixture(scope="module")
def ext():
    import lagomorph_amd

    lagomorph_amd.set_debug_mode(True)
    shim = lagomorph_amd.lagomorph_ext
    saved = shim.get_tuning()
    try:
        yield shim
    finally:
        shim.tune(**saved)
        lagomorph_amd.set_debug_mode(False)
        print(f"alignment: {RAN['cases']} cases, {RAN['calls']} calls")
        out = os.environ.get("LAGO_TOL_REPORT")
        if out:  # observed errors of the tolerance-based comparisons, in units of the bound
            json.dump(dict(sorted(OBSERVED.items())), open(out, "w"), indent=1)


# ---------------------------------------------------------------------------------------------------- the driver

class Case:
    """One call.  make(dtype, ext) -> {name: array or list of arrays}: the tensor arguments on the host;
    call(ext, t) -> {output name: tensor} for t = {name: device view(s)} (an argument the callee writes is returned
    under its own name); ref(a) -> {output name: want or (want, scale)} for the host arrays a.

    outs: output name -> how it is judged
        "bits"        control == ref bit for bit; offset runs == control bit for bit
        "close_bits"  control within assert_close of ref; offset runs == control bit for bit
        "close"       every run within assert_close of ref (atomics, FFT: the summation order is free)
        "same"        offset runs == control bit for bit (the reference judges another output of the case)
    path(dtype, offs) -> the expected `path_launches` delta with the arguments `offs` (a set of names) off alignment,
    or None: whatever the control took, unchanged.  pair: two arguments that feed one vector loop."""

    def __init__(self, name, entries, make, call, ref, outs, dtypes=BOTH, path=None, pair=None, tune=None, attrs=None,
                 offsets=None, pads=None):
        self.name, self.entries, self.make, self.call, self.ref, self.outs = name, tuple(entries), make, call, ref, outs
        self.dtypes, self.path, self.pair, self.tune, self.attrs = dtypes, path, pair, tune or {}, attrs or {}
        self.offsets, self.pads = offsets or {}, pads or {}


CASES = []


def add(*args, **kw):
    CASES.append(Case(*args, **kw))


def _tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def _views(case, arrays, offs):
    """Device views of every argument at its offset (0: aligned), and every (buffer, view) pair for the margin check."""
    t, guards = {}, []
    for name, a in arrays.items():
        if name.startswith("_"):
            continue   # host-side data of the reference, no argument of the call
        items = a if isinstance(a, list) else [a]
        pad = case.pads.get(name, 8)
        made = [offset_view(_tensor(x).cuda(), offs.get(name, 0), pad=pad) for x in items]
        guards += [(name, buf, v) for v, buf in made]
        t[name] = [v for v, _ in made] if isinstance(a, list) else made[0][0]
    return t, guards


def _run_once(ext, case, arrays, offs):
    """(outputs on the host, path delta) of one call; the margins and the outputs' freedom from poison are judged here."""
    t, guards = _views(case, arrays, offs)
    before = ext.path_launches()
    outs = case.call(ext, t)
    torch.cuda.synchronize()
    after = ext.path_launches()
    what = f"{case.name} offsets {offs}"
    for name, buf, v in guards:
        touched = margins_intact(buf, v)
        assert touched == [], f"{what}: the call changed elements {touched[:8]} of the margins around {name}"
    got = {}
    for k, o in outs.items():
        assert o.is_contiguous(), f"{what}: {k} is not contiguous"
        if o.dtype.is_floating_point:
            assert not torch.isnan(o).any(), f"{what}: {int(torch.isnan(o).sum())} NaN in {k} (a read out of the margins?)"
        else:
            assert poisoned(o) == 0, f"{what}: {k} holds the poison label (a read out of the margins)"
        got[k] = o.detach().cpu()
    return got, {k: after[k] - before[k] for k in after if after[k] != before[k]}


def _schedule(case, names):
    """The offset runs: each argument alone, all together, and the pair at different offsets."""
    def allowed(name):
        return case.offsets.get(name, OFFSETS)

    runs = [{n: o} for n in names for o in allowed(n)]
    if len(names) > 1:
        runs += [{n: allowed(n)[i % len(allowed(n))] for n in names} for i in range(len(OFFSETS))]
    if case.pair:
        a, b = case.pair
        runs.append({a: allowed(a)[0], b: allowed(b)[-1] if allowed(b)[-1] != allowed(a)[0] else allowed(b)[0]})
    return runs


def _judge_against_ref(case, dtype, got, want, what, modes):
    for k, mode in case.outs.items():
        if mode not in modes:
            continue
        w, scale = want[k] if isinstance(want[k], tuple) else (want[k], None)
        w = host(w) if isinstance(w, torch.Tensor) else np.asarray(w)
        if mode == "bits":
            assert_bits(got[k], w, f"{what}: {k}")
        else:
            real = F64 if got[k].dtype == torch.float64 else F32
            assert_close(got[k], w, real, f"alignment {case.entries[0]} {k} ({what})", scale=scale)


def run_case(ext, case, dtype):
    saved_tuning = ext.get_tuning()
    saved_attrs = {k: getattr(ext, k) for k in case.attrs}
    try:
        ext.tune(**case.tune)
        for k, v in case.attrs.items():
            setattr(ext, k, v)
        arrays = case.make(dtype, ext)
        want = case.ref(arrays)
        assert set(want) >= {k for k, m in case.outs.items() if m != "same"}
        names = [n for n in arrays if not n.startswith("_")]
        control, took0 = _run_once(ext, case, arrays, {})
        assert set(control) == set(case.outs), (sorted(control), sorted(case.outs))
        if case.path is not None and case.path(dtype, frozenset()) is not None:
            assert took0 == case.path(dtype, frozenset()), f"{case.name}: the control took {took0}"
        _judge_against_ref(case, dtype, control, want, f"{case.name} control", ("bits", "close_bits", "close"))
        runs = _schedule(case, names)
        for offs in runs:
            what = f"{case.name} offsets {offs}"
            got, took = _run_once(ext, case, arrays, offs)
            expect = case.path(dtype, frozenset(offs)) if case.path is not None else None
            assert took == (took0 if expect is None else expect), f"{what}: took {took}, the control {took0}"
            for k, mode in case.outs.items():
                if mode != "close":
                    assert got[k].dtype == control[k].dtype and got[k].shape == control[k].shape
                    same = torch.equal(got[k], control[k])
                    assert same, f"{what}: {k} differs from the aligned call in {int((got[k] != control[k]).sum())} values"
            _judge_against_ref(case, dtype, got, want, what, ("close",))
        return 1 + len(runs)
    finally:
        for k, v in saved_attrs.items():
            setattr(ext, k, v)
        ext.tune(**saved_tuning)


def _seed(*key):
    return np.random.default_rng([int(k) for k in key])


# ---------------------------------------------------------------------------------------------------- gathers, splats

def _gated(fast, sibling, pointer):
    """float32: `fast` while `pointer` is aligned, `sibling` otherwise; float64 has no gate here."""
    def path(dtype, offs):
        if dtype != F32:
            return None
        return {(sibling if pointer in offs else fast): 1}
    return path


def _fixed(f32=None, f64=None):
    def path(dtype, offs):
        p = f32 if dtype == F32 else f64
        return None if p is None else ({p: 1} if p else {})
    return path


def _interp_inputs(sp, nc, bc, smooth, seed):
    def make(dtype, ext):
        rng = _seed(1, seed, *sp)
        u = rnd(rng, (2, len(sp)) + sp, dtype, 0.5) if smooth else displacement(rng, 2, sp, dtype)
        return {"I": rnd(rng, ((1 if bc else 2), nc) + sp, dtype), "u": u, "go": rnd(rng, (2, nc) + sp, dtype)}
    return make


for sp, nc, bc, smooth, path in (((5, 6, 7), 2, False, False, _fixed("", "")), ((7, 9), 2, True, False, _fixed("", "")),
                                 ((8, 16, 32), 1, False, True, _fixed("vector_gather")),
                                 ((32, 32, 32), 2, False, True, _gated("gather_window", "vector_gather", "I")),
                                 ((32, 32, 32), 3, True, True, _gated("gather_window", "vector_gather", "I"))):
    for dt in (1.0, -0.3):
        def make(dtype, ext, inner=_interp_inputs(sp, nc, bc, smooth, 1)):
            a = inner(dtype, ext)
            return {"I": a["I"], "u": a["u"]}
        add(f"interp_forward {sp} nc={nc} bc={bc} dt={dt}", ["interp_forward"], make,
            lambda ext, t, dt=dt: {"out": ext.interp_forward(t["I"], t["u"], dt)},
            lambda a, dt=dt: {"out": orc.interp_forward(a["I"], a["u"], dt)}, {"out": "bits"}, path=path)

for sp, nc, bc, tune, path in (((5, 6, 7), 2, False, None, None), ((7, 9), 2, True, None, None),
                               ((8, 16, 32), 1, False, None, None),
                               ((16, 16, 16), 1, False, None, _fixed("splat_shear", "splat_tiled")),
                               ((16, 16, 16), 3, True, None, _fixed("splat_shear_mc", "splat_tiled")),
                               ((16, 16, 16), 3, False, {"splat_shear": [0, 8, 6, 0, 1, 1, 4, 1024]},
                                _fixed("splat_tiled", "splat_tiled")),
                               ((128, 128), 2, False, None, _fixed("splat_2d", "splat_2d"))):
    add(f"interp_backward {sp} nc={nc} bc={bc} tune={tune}", ["interp_backward"], _interp_inputs(sp, nc, bc, False, 2),
        lambda ext, t: dict(zip(("d_I", "d_u"), ext.interp_backward(t["go"], t["I"], t["u"], -0.3, True, True))),
        lambda a: dict(zip(("d_I", "d_u"), orc.interp_backward(a["go"], a["I"], a["u"], -0.3, True, True))),
        {"d_I": "close", "d_u": "bits"}, path=path, tune=tune)


def _fused_make(sp, nc, bc, seed):
    def make(dtype, ext):
        a = _interp_inputs(sp, nc, bc, False, seed)(dtype, ext)
        rng = _seed(3, seed, *sp)
        a["d_u"] = rnd(rng, a["u"].shape, dtype)
        a["d_I"] = rnd(rng, a["I"].shape, dtype)
        return a
    return make


def _fused_ref(a):
    oI, ou = orc.interp_backward(a["go"], a["I"], a["u"], 0.8, True, True)
    return {"d_I": (a["d_I"].astype(np.float64) + oI, np.abs(oI).max() + np.abs(a["d_I"]).max()),
            "d_u": (a["d_u"].astype(np.float64) + ou, np.abs(ou).max() + np.abs(a["d_u"]).max())}


def _addgo_ref(a):
    oI, ou = orc.interp_backward(a["go"], a["I"], a["u"], 0.8, True, True)
    k = a["go"].dtype.type
    return {"d_I": oI, "d_u": ((k(0.37) * a["go"]).astype(np.float64) + ou, np.abs(ou).max() + np.abs(a["go"]).max())}


for sp, bc, path in (((5, 6, 7), False, None), ((7, 9), True, None), ((16, 16, 16), False, None),
                     ((128, 128), False, _fixed("splat_2d", "splat_2d"))):
    # the reverse sweep of lddmm.py accumulates through d_u= and d_I=: caller-owned outputs
    add(f"interp_backward_fused d_u= d_I= {sp} bc={bc}", ["interp_backward_fused"], _fused_make(sp, len(sp), bc, 4),
        lambda ext, t: dict(zip(("d_I", "d_u"), ext.interp_backward_fused(t["go"], t["I"], t["u"], 0.8, True, d_u=t["d_u"],
                                                                          d_I=t["d_I"]))),
        _fused_ref, {"d_I": "close", "d_u": "close_bits"}, path=path)
    add(f"interp_backward_fused addgo {sp} bc={bc}", ["interp_backward_fused"], _interp_inputs(sp, len(sp), bc, False, 5),
        lambda ext, t: dict(zip(("d_I", "d_u"), ext.interp_backward_fused(t["go"], t["I"], t["u"], 0.8, True, addgo=0.37))),
        _addgo_ref, {"d_I": "close", "d_u": "close_bits"}, path=path)

for sp in ((9, 8), (128, 128)):
    def make(dtype, ext, sp=sp):
        rng = _seed(6, *sp)
        return {"I": rnd(rng, (2, 3) + sp, dtype), "u": displacement(rng, 2, sp, dtype)}
    add(f"interp_hessian_diagonal_image {sp}", ["interp_hessian_diagonal_image"], make,
        lambda ext, t: {"out": ext.interp_hessian_diagonal_image(t["I"], t["u"], 0.6)},
        lambda a: {"out": orc.interp_hessian_diagonal_image(a["I"], a["u"], 0.6)}, {"out": "close"})


# ---------------------------------------------------------------------------------------------------- compose, Ad*

def _fields_make(sp, names, seed, first_scale=None, with_out=False):
    """Vector fields (2, d) + sp; the first is a displacement: the clamp / floor / integer mix, or smooth at first_scale."""
    def make(dtype, ext):
        rng = _seed(7, seed, *sp)
        a = {}
        for i, n in enumerate(names):
            if i == 0 and first_scale is None:
                a[n] = displacement(rng, 2, sp, dtype)
            else:
                a[n] = rnd(rng, (2, len(sp)) + sp, dtype, first_scale if i == 0 else 1.0)
        if with_out:
            a["out"] = np.zeros_like(a[names[0]])
        return a
    return make


def _compose_ref(ds, dt):
    def ref(a):
        k = a["u"].dtype.type
        return {"out": k(ds) * a["u"] + k(dt) * orc.interp_forward(a["v"], a["u"], ds)}
    return ref


for sp, scale, near, with_out, ds, path in (
        ((5, 6, 7), None, False, False, 0.7, _fixed("", "")), ((7, 9), None, False, True, 1.0, _fixed("", "")),
        ((32, 32, 32), 0.5, False, False, 1.0, _gated("gather_window", "vector_gather", "v")),
        ((32, 32, 32), 0.5, False, True, 0.5, _gated("gather_window", "vector_gather", "v")),
        ((32, 32, 32), 6.0, True, False, -0.1, _gated("gather_window_near", "vector_gather", "v")),
        ((32, 32, 32), 6.0, True, True, -0.1, _gated("gather_window_near", "vector_gather", "v"))):
    def call(ext, t, ds=ds, near=near, with_out=with_out):
        out = ext.compose(t["u"], t["v"], ds, -0.1 if not near else 1.0, out=t.get("out"), near_identity=near)
        assert (out is t["out"]) if with_out else True
        return {"out": out}
    add(f"compose {sp} ds={ds} near={near} out={with_out}", ["compose"], _fields_make(sp, ("u", "v"), 8, scale, with_out),
        call, _compose_ref(ds, 1.0 if near else -0.1), {"out": "bits"}, path=path)


def _Ad_star_ref(a):
    mphi = orc.interp_forward(a["m"], a["phi"], 1.0)
    return {"out": orc.jacobian_times_vectorfield_forward(a["phi"], mphi, True, False), "mphi": mphi}


for sp, scale, path in (((5, 6, 7), None, None), ((7, 9), None, None), ((28, 32, 64), 0.5, _fixed("stencil_tile"))):
    add(f"Ad_star {sp}", ["Ad_star"], _fields_make(sp, ("phi", "m"), 9, scale),
        lambda ext, t: {"out": ext.Ad_star(t["phi"], t["m"])}, _Ad_star_ref, {"out": "bits"}, path=path)
    add(f"Ad_star save_resampled {sp}", ["Ad_star"], _fields_make(sp, ("phi", "m"), 9, scale),
        lambda ext, t: dict(zip(("out", "mphi"), ext.Ad_star(t["phi"], t["m"], save_resampled=True))), _Ad_star_ref,
        {"out": "bits", "mphi": "bits"}, path=path)

for sp in ((5, 6, 7), (7, 9), (8, 4, 66)):
    add(f"ad_star {sp}", ["ad_star"], _fields_make(sp, ("v", "m"), 10, 1.0),
        lambda ext, t: {"out": ext.ad_star(t["v"], t["m"])},
        lambda a: {"out": orc.jacobian_times_vectorfield_forward(a["v"], a["m"], False, True)
                   - orc.jacobian_times_vectorfield_adjoint_forward(a["m"], a["v"])}, {"out": "bits"})


# ---------------------------------------------------------------------------------------------------- Jacobian products

for sp in ((5, 6, 7), (7, 9), (8, 4, 66)):
    for disp, trans in ((True, False), (False, True)):
        add(f"jtv forward {sp} disp={disp} trans={trans}", ["jacobian_times_vectorfield_forward"],
            _fields_make(sp, ("g", "v"), 11, 1.0),
            lambda ext, t, disp=disp, trans=trans: {"out": ext.jacobian_times_vectorfield_forward(t["g"], t["v"], disp, trans)},
            lambda a, disp=disp, trans=trans: {"out": orc.jacobian_times_vectorfield_forward(a["g"], a["v"], disp, trans)},
            {"out": "bits"})
        add(f"jtv backward {sp} disp={disp} trans={trans}", ["jacobian_times_vectorfield_backward"],
            _fields_make(sp, ("go", "v", "w"), 12, 1.0),
            lambda ext, t, disp=disp, trans=trans: dict(zip(("d_v", "d_w"), ext.jacobian_times_vectorfield_backward(
                t["go"], t["v"], t["w"], disp, trans, True, True))),
            lambda a, disp=disp, trans=trans: dict(zip(("d_v", "d_w"), orc.jacobian_times_vectorfield_backward(
                a["go"], a["v"], a["w"], disp, trans))),
            {"d_v": "bits", "d_w": "bits"}, pair=("v", "w"))

    def acc_ref(a):
        ov, ow = orc.jacobian_times_vectorfield_backward(a["go"], a["v"], a["w"], True, False)
        # the gradient is added onto what d_v holds: start + d_v to rounding (one summation order differs), the
        # comparison tests/test_gpu_parity.py makes for the accumulating form of interp_backward_fused
        return {"d_v": (a["d_v"].astype(np.float64) + ov, np.abs(ov).max() + np.abs(a["d_v"]).max()), "d_w": ow}
    add(f"jtv backward d_v= {sp}", ["jacobian_times_vectorfield_backward"], _fields_make(sp, ("go", "v", "w", "d_v"), 13, 1.0),
        lambda ext, t: dict(zip(("d_v", "d_w"), ext.jacobian_times_vectorfield_backward(
            t["go"], t["v"], t["w"], True, False, True, True, d_v=t["d_v"]))),
        acc_ref, {"d_v": "close_bits", "d_w": "bits"}, pair=("v", "d_v"))
    add(f"jtv adjoint forward {sp}", ["jacobian_times_vectorfield_adjoint_forward"], _fields_make(sp, ("g", "v"), 14, 1.0),
        lambda ext, t: {"out": ext.jacobian_times_vectorfield_adjoint_forward(t["g"], t["v"])},
        lambda a: {"out": orc.jacobian_times_vectorfield_adjoint_forward(a["g"], a["v"])}, {"out": "bits"})
    add(f"jtv adjoint backward {sp}", ["jacobian_times_vectorfield_adjoint_backward"],
        _fields_make(sp, ("go", "v", "w"), 15, 1.0),
        lambda ext, t: dict(zip(("d_v", "d_w"), ext.jacobian_times_vectorfield_adjoint_backward(t["go"], t["v"], t["w"], True, True))),
        lambda a: dict(zip(("d_v", "d_w"), orc.jacobian_times_vectorfield_adjoint_backward(a["go"], a["v"], a["w"]))),
        {"d_v": "bits", "d_w": "bits"}, pair=("v", "w"))

    def jd_make(dtype, ext, sp=sp):
        rng = _seed(16, *sp)
        return {"u": rnd(rng, (2, len(sp)) + sp, dtype, 0.3), "go": rnd(rng, (2, 1) + sp, dtype)}
    add(f"jacobian_determinant_forward {sp}", ["jacobian_determinant_forward"],
        lambda dtype, ext, mk=jd_make: {"u": mk(dtype, ext)["u"]},
        lambda ext, t: {"out": ext.jacobian_determinant_forward(t["u"], True)},
        lambda a: {"out": jacdet_ref.forward(a["u"], True)}, {"out": "bits"})
    add(f"jacobian_determinant_backward {sp}", ["jacobian_determinant_backward"], jd_make,
        lambda ext, t: {"d_u": ext.jacobian_determinant_backward(t["go"], t["u"], True)},
        lambda a: {"d_u": jacdet_ref.backward(a["go"], a["u"], True)}, {"d_u": "close_bits"})


# ---------------------------------------------------------------------------------------------------- inverse

for sp in ((6, 5, 8), (7, 9)):
    def inv_make(dtype, ext, sp=sp):
        u = invert_ref.field(sp, 2, NP[dtype])
        return {"u": u, "v": invert_ref.forward(u, 60).astype(NP[dtype]), "go": rnd(_seed(17, *sp), u.shape, dtype)}
    add(f"invert_displacement_forward {sp}", ["invert_displacement_forward"],
        lambda dtype, ext, mk=inv_make: {"u": mk(dtype, ext)["u"]},
        lambda ext, t: {"v1": ext.invert_displacement_forward(t["u"], 1), "v5": ext.invert_displacement_forward(t["u"], 5)},
        lambda a: {"v1": invert_ref.forward(a["u"], 1)}, {"v1": "close_bits", "v5": "same"})
    add(f"invert_displacement_adjoint {sp}", ["invert_displacement_adjoint"], inv_make,
        lambda ext, t: {"lam": ext.invert_displacement_adjoint(t["go"], t["u"], t["v"])},
        lambda a: {"lam": invert_ref.lam(a["go"], a["u"], a["v"])}, {"lam": "close_bits"})


# ---------------------------------------------------------------------------------------------------- Gaussian, LNCC, MI

def _gauss_plan(sigma, dim):
    sig = gauss_ref.per_axis(sigma, dim)
    return [gauss_ref.radius(s) for s in sig], [gauss_ref.taps(s) for s in sig]


# (6, 5, 16): rows of n % 4 == 0, the 4-vector stores and behind their gate the masked scalar ones, three passes with the
# scratch tensor; (2, 3, 1028): a row of two segments; (9, 8): 2D
for sp, lead, sigma, mode in (((6, 5, 16), (2, 2), (1.0, 0.7, 1.5), "wrap"), ((6, 5, 16), (2, 1), (0.0, 0.0, 1.0), "zero"),
                              ((2, 3, 1028), (1, 2), (0.0, 0.0, 2.5), "wrap"), ((9, 8), (2, 2), (1.0, 1.5), "zero")):
    def g_make(dtype, ext, sp=sp, lead=lead):
        rng = _seed(18, *sp)
        return {"x": rnd(rng, lead + sp, dtype), "out": rnd(rng, lead + sp, dtype)}

    def g_ref(a, sigma=sigma, mode=mode):
        r = gauss_ref.smooth(a["x"], sigma, mode=mode)
        out = {"plain": r, "alpha": -0.5 * r}
        if "out" in a:
            out["acc"] = a["out"].astype(np.float64) - 0.5 * r
        return out
    radii, taps = _gauss_plan(sigma, len(sp))
    add(f"gaussian_smooth_forward {sp} {sigma} {mode}", ["gaussian_smooth_forward"],
        lambda dtype, ext, mk=g_make: {"x": mk(dtype, ext)["x"]},
        lambda ext, t, radii=radii, taps=taps, mode=mode: {"plain": ext.gaussian_smooth_forward(t["x"], radii, taps, mode)},
        g_ref, {"plain": "close_bits"})
    add(f"gaussian_smooth_forward out= {sp} {sigma} {mode}", ["gaussian_smooth_forward"], g_make,
        lambda ext, t, radii=radii, taps=taps, mode=mode: {
            "alpha": ext.gaussian_smooth_forward(t["x"], radii, taps, mode, alpha=-0.5, out=t["out"])},
        g_ref, {"alpha": "close_bits"})
    add(f"gaussian_smooth_forward accumulate {sp} {sigma} {mode}", ["gaussian_smooth_forward"], g_make,
        lambda ext, t, radii=radii, taps=taps, mode=mode: {
            "acc": ext.gaussian_smooth_forward(t["x"], radii, taps, mode, alpha=-0.5, out=t["out"], accumulate=True)},
        g_ref, {"acc": "close_bits"})

EPS = 1e-5
for sp, sigma, mode in (((6, 5, 16), 1.0, "wrap"), ((2, 3, 1028), (0.0, 0.0, 2.5), "zero"), ((9, 8), 1.0, "wrap")):
    radii, taps = _gauss_plan(sigma, len(sp))

    def l_make(dtype, ext, sp=sp, radii=radii, taps=taps, mode=mode):
        I, J, g = (a.astype(NP[dtype]) for a in lncc_ref.inputs(sp, "corr"))
        mom = ext.lncc_moments(dev(I), dev(J), radii, taps, mode)   # the moments the backward is handed: the library's own
        return {"go": g, "I": I, "J": J, "moments": host(mom)}

    def l_ref(a, sigma=sigma, mode=mode):
        I, J = (a[k] if k in a else a["_" + k] for k in "IJ")
        if "go" not in a:
            return {"cc": lncc_ref.lncc(I, J, sigma, mode=mode, eps=EPS)}
        cc, dI, dJ = lncc_ref.lncc_with_grads(I, J, a["go"], sigma, mode=mode, eps=EPS)
        return {"cc": cc, "d_I": dI, "d_J": dJ}

    def l_call(ext, t, radii=radii, taps=taps, mode=mode):
        mom = ext.lncc_moments(t["I"], t["J"], radii, taps, mode)
        return {"moments": mom, "cc": ext.lncc_cc(mom, EPS)}
    add(f"lncc_moments {sp} {sigma} {mode}", ["lncc_moments"],
        lambda dtype, ext, mk=l_make: {k: v for k, v in mk(dtype, ext).items() if k in ("I", "J")}, l_call, l_ref,
        {"moments": "same", "cc": "close_bits"}, pair=("I", "J"))
    add(f"lncc_cc {sp} {sigma} {mode}", ["lncc_cc"],
        lambda dtype, ext, mk=l_make: {("_" + k if k in "IJ" else k): v for k, v in mk(dtype, ext).items() if k != "go"},
        lambda ext, t: {"cc": ext.lncc_cc(t["moments"], EPS)}, l_ref, {"cc": "close_bits"})
    add(f"lncc_backward {sp} {sigma} {mode}", ["lncc_backward"], l_make,
        lambda ext, t, radii=radii, taps=taps, mode=mode: dict(zip(("d_I", "d_J"), ext.lncc_backward(
            t["go"], t["I"], t["J"], t["moments"], radii, taps, mode, EPS))),
        l_ref, {"d_I": "close_bits", "d_J": "close_bits"}, pair=("I", "J"))

for lead, sp, B in (((2, 2), (5, 6, 7), 32), ((1, 2), (9, 8), 5)):
    def m_make(dtype, ext, lead=lead, sp=sp, B=B):
        rng = _seed(19, *sp)
        I, N = (rng.standard_normal(lead + sp).astype(np.float32) for _ in range(2))
        J = (np.float32(0.8) * I + np.float32(0.6) * N).astype(np.float32)
        return {"G": rng.standard_normal(lead + (B, B)), "I": I.astype(NP[dtype]), "J": J.astype(NP[dtype])}
    rJ = (-1.0, 1.5)

    def m_ranges(a):
        return mi_ref.auto_range(a["I"].astype(np.float64)), rJ
    # P is a sum of 64-bit fixed-point integers: it equals the reference exactly, and so does every offset run
    add(f"mi_histogram {lead}+{sp} B={B}", ["mi_histogram"],
        lambda dtype, ext, mk=m_make: {k: v for k, v in mk(dtype, ext).items() if k != "G"},
        lambda ext, t, B=B: {"P": ext.mi_histogram(t["I"], t["J"], B, mi_ref.auto_range(host(t["I"]).astype(np.float64)), rJ)},
        lambda a, B=B: {"P": mi_ref.joint_histogram(a["I"].astype(np.float64), a["J"].astype(np.float64), B, *m_ranges(a))},
        {"P": "bits"}, pair=("I", "J"))
    add(f"mi_backward {lead}+{sp} B={B}", ["mi_backward"], m_make,
        lambda ext, t, B=B: dict(zip(("d_I", "d_J"), ext.mi_backward(
            t["G"], t["I"], t["J"], B, mi_ref.auto_range(host(t["I"]).astype(np.float64)), rJ))),
        lambda a, B=B: dict(zip(("d_I", "d_J"), mi_ref.backward(a["G"], a["I"].astype(np.float64), a["J"].astype(np.float64),
                                                                 B, *m_ranges(a)))),
        {"d_I": "close_bits", "d_J": "close_bits"}, pair=("I", "J"))


# ---------------------------------------------------------------------------------------------------- B-spline, points, FFD

for sp in ((5, 6, 7), (7, 9)):
    for adjoint in (False, True):
        add(f"bspline_prefilter {sp} adjoint={adjoint}", ["bspline_prefilter"],
            lambda dtype, ext, sp=sp: {"I": bspline_ref.image(1, 3, sp, NP[dtype], seed=3)},
            lambda ext, t, adjoint=adjoint: {"out": ext.bspline_prefilter(t["I"], adjoint)},
            lambda a, adjoint=adjoint: {"out": bspline_ref.prefilter(a["I"], adjoint)}, {"out": "close_bits"})
    for bc in (False, True):
        def b_make(dtype, ext, sp=sp, bc=bc):
            d = len(sp)
            return {"go": bspline_ref.image(2, d, sp, NP[dtype], seed=100 + d),
                    "C": bspline_ref.image(1 if bc else 2, d, sp, NP[dtype], seed=d),
                    "u": labels_ref.displacement("random", 2, sp, NP[dtype])}

        def b_ref(a):
            C64 = a["C"].astype(np.float64)
            kw = dict(wfun=bspline_ref.weights_wide, add_dtype=np.longdouble) if a["C"].dtype == np.float64 else {}
            if "go" not in a:
                return {"out": bspline_ref.interp(C64, a["u"], 1.0)}
            return {"d_u": bspline_ref.grad_u(a["go"], C64, a["u"], 1.0),
                    "d_C": bspline_ref.grad_C_wide(a["go"], a["C"].shape, a["u"], **kw)[0].astype(np.float64)}
        add(f"interp_bspline_forward {sp} bc={bc}", ["interp_bspline_forward"],
            lambda dtype, ext, mk=b_make: {k: v for k, v in mk(dtype, ext).items() if k != "go"},
            lambda ext, t: {"out": ext.interp_bspline_forward(t["C"], t["u"], 1.0)}, b_ref, {"out": "close_bits"})
        add(f"interp_bspline_backward {sp} bc={bc}", ["interp_bspline_backward"], b_make,
            lambda ext, t: dict(zip(("d_C", "d_u"), ext.interp_bspline_backward(t["go"], t["C"], t["u"], 1.0, True, True))),
            b_ref, {"d_C": "close", "d_u": "close_bits"})

        def p_make(dtype, ext, sp=sp, bc=bc, P=65):
            return {"g": points_ref.upstream(2, 3, P, NP[dtype]), "F": points_ref.field(1 if bc else 2, 3, sp, NP[dtype], seed=P),
                    "x": points_ref.scattered(2, sp, P, NP[dtype])[0]}

        def p_ref(a):
            val, grad = points_ref.sample(a["F"], a["x"])
            if "g" not in a:
                return {"out": val}
            return {"d_x": (a["g"][:, :, None, :].astype(np.float64) * grad).sum(1),
                    "d_F": points_ref.scatter_wide(a["g"], a["x"], a["F"].shape[2:], a["F"].shape[0])[0].astype(np.float64)}
        add(f"interp_points_forward {sp} bc={bc}", ["interp_points_forward"],
            lambda dtype, ext, mk=p_make: {k: v for k, v in mk(dtype, ext).items() if k != "g"},
            lambda ext, t: {"out": ext.interp_points_forward(t["F"], t["x"])}, p_ref, {"out": "close_bits"})
        add(f"interp_points_backward {sp} bc={bc}", ["interp_points_backward"], p_make,
            lambda ext, t: dict(zip(("d_F", "d_x"), ext.interp_points_backward(t["g"], t["F"], t["x"], True, True))),
            p_ref, {"d_F": "close", "d_x": "close_bits"})

for shape, spacing in (((5, 6, 7), (2, 3, 4)), ((9, 11), (4, 1))):
    def f_ref(a, shape=shape, spacing=spacing):
        out = {}
        if "ctrl" in a:
            work = np.longdouble if a["ctrl"].dtype == np.float64 else np.float64
            out["out"] = np.asarray(ffd_ref.expand(a["ctrl"], shape, spacing, work=work), dtype=np.float64)
        if "g" in a:
            out["d_ctrl"] = ffd_ref.adjoint(a["g"], spacing)
        return out
    add(f"ffd_expand {shape} / {spacing}", ["ffd_expand"],
        lambda dtype, ext, shape=shape, spacing=spacing: {
            "ctrl": ffd_ref.field(2, len(shape), ffd_ref.grid_shape(shape, spacing), np.dtype(NP[dtype]))},
        lambda ext, t, shape=shape, spacing=spacing: {"out": ext.ffd_expand(t["ctrl"], shape, spacing)}, f_ref,
        {"out": "close_bits"})
    add(f"ffd_expand_adjoint {shape} / {spacing}", ["ffd_expand_adjoint"],
        lambda dtype, ext, shape=shape: {"g": ffd_ref.field(2, len(shape), shape, np.dtype(NP[dtype]), seed=7)},
        lambda ext, t, spacing=spacing: {"d_ctrl": ext.ffd_expand_adjoint(t["g"], spacing)}, f_ref, {"d_ctrl": "close"})


# ---------------------------------------------------------------------------------------------------- labels, distances

K_LABELS = 5
for sp in ((5, 6, 7), (7, 9)):
    for mode, bc, ldt in (("vote", False, torch.int32), ("nearest", True, torch.int32), ("vote", False, torch.uint8)):
        def w_make(dtype, ext, sp=sp, bc=bc, ldt=ldt):
            L = labels_ref.labels("random5", 1 if bc else 2, sp)
            return {"L": torch.from_numpy(L).to(ldt), "u": labels_ref.displacement("random", 2, sp, NP[dtype])}
        add(f"warp_labels {sp} {mode} bc={bc} {ldt}", ["warp_labels"], w_make,
            lambda ext, t, mode=mode: {"out": ext.warp_labels(t["L"], t["u"], 0.7, mode)},
            lambda a, mode=mode: {"out": labels_ref.warp(host(a["L"]), a["u"], 0.7, mode)}, {"out": "bits"},
            pads={"L": 16} if ldt == torch.uint8 else None)   # (uint8: offsets 1 - 3 are byte offsets)
    for ldt in (torch.int32, torch.uint8):
        def o_make(dtype, ext, sp=sp, ldt=ldt):
            rng = _seed(20, *sp)
            lo = -1 if ldt == torch.int32 else 0
            return {n: torch.from_numpy(rng.integers(lo, K_LABELS + 2, (2, 1) + sp).astype(np.int32)).to(ldt) for n in "AB"}
        add(f"label_overlap {sp} {ldt}", ["label_overlap"], o_make,
            lambda ext, t: {"counts": ext.label_overlap(t["A"], t["B"], K_LABELS)},
            lambda a: {"counts": labels_ref.overlap(host(a["A"]).astype(np.int32), host(a["B"]).astype(np.int32), K_LABELS)},
            {"counts": "bits"}, dtypes=(F32,), pair=("A", "B"), pads={"A": 16, "B": 16} if ldt == torch.uint8 else None)
    for where, squared, ldt in (("nonzero", True, torch.int32), ("surface", False, torch.int32), ("equal", False, torch.uint8)):
        add(f"distance_transform {sp} {where} squared={squared} {ldt}", ["distance_transform"],
            lambda dtype, ext, sp=sp, ldt=ldt: {"L": torch.from_numpy(edt_ref.labels("blobs", 2, sp)).to(ldt)},
            lambda ext, t, where=where, squared=squared: {"out": ext.distance_transform(t["L"], where, 1, 1.0, squared)},
            lambda a, where=where, squared=squared: {
                "out": edt_ref.distance_transform(host(a["L"]).astype(np.int32), where, 1, 1.0, squared)},
            {"out": "bits"}, dtypes=(F32,), pads={"L": 16} if ldt == torch.uint8 else None)


# ---------------------------------------------------------------------------------------------------- affine, regrid

for sp, mild, path in (((5, 6, 7), False, _fixed("", "")), ((7, 9), False, _fixed("", "")),
                       ((2, 2, 16), True, _fixed("splat_affine_box", "splat_affine_box"))):
    for bc in (False, True):
        def a_make(dtype, ext, sp=sp, mild=mild, bc=bc):
            d, rng = len(sp), _seed(21, *sp)
            A = (np.eye(d)[None] + (0.02 if mild else 0.3) * rng.standard_normal((2, d, d))).astype(NP[dtype])
            return {"go": rnd(rng, (2, 2) + sp, dtype), "I": rnd(rng, ((1 if bc else 2), 2) + sp, dtype), "A": A,
                    "T": (1.5 * rng.standard_normal((2, d))).astype(NP[dtype])}
        add(f"affine_interp_forward {sp} bc={bc}", ["affine_interp_forward"],
            lambda dtype, ext, mk=a_make: {k: v for k, v in mk(dtype, ext).items() if k != "go"},
            lambda ext, t: {"out": ext.affine_interp_forward(t["I"], t["A"], t["T"])},
            lambda a: {"out": orc.affine_interp_forward(a["I"], a["A"], a["T"])}, {"out": "bits"})
        add(f"affine_interp_backward {sp} bc={bc}", ["affine_interp_backward"], a_make,
            lambda ext, t: dict(zip(("d_I", "d_A", "d_T"), ext.affine_interp_backward(t["go"], t["I"], t["A"], t["T"], True, True, True))),
            lambda a: dict(zip(("d_I", "d_A", "d_T"), orc.affine_interp_backward(a["go"], a["I"], a["A"], a["T"], True, True, True))),
            {"d_I": "close", "d_A": "close", "d_T": "close"}, path=path)

for sp, out in (((5, 6, 7), (7, 5, 9)), ((7, 9), (9, 4))):
    origin = [(s - 1) * 0.5 + 0.3 for s in sp]
    spacing = [(a - 1) / (b - 1) * 1.1 for a, b in zip(sp, out)]
    add(f"regrid_forward {sp} -> {out}", ["regrid_forward"],
        lambda dtype, ext, sp=sp: {"I": rnd(_seed(22, *sp), (2, 3) + sp, dtype)},
        lambda ext, t, out=out, origin=origin, spacing=spacing: {"out": ext.regrid_forward(t["I"], list(out), origin, spacing)},
        lambda a, out=out, origin=origin, spacing=spacing: {"out": orc.regrid_forward(a["I"], list(out), origin, spacing)},
        {"out": "bits"})
    for sep in (1, 0):   # axis by axis in gather form (the default), and the reference's splat
        add(f"regrid_backward {out} -> {sp} separable={sep}", ["regrid_backward"],
            lambda dtype, ext, out=out: {"go": rnd(_seed(23, *out), (2, 3) + out, dtype)},
            lambda ext, t, sp=sp, out=out, origin=origin, spacing=spacing: {
                "d_I": ext.regrid_backward(t["go"], list(sp), list(out), origin, spacing)},
            lambda a, sp=sp, out=out, origin=origin, spacing=spacing: {
                "d_I": orc.regrid_backward(a["go"], list(sp), list(out), origin, spacing)},
            {"d_I": "close"}, attrs={"REGRID_BACKWARD_SEPARABLE": sep})


# ---------------------------------------------------------------------------------------------------- fluid operator, metric

def _luts(sp, npdt):
    cos, sin = orc.fluid_luts(sp, npdt)
    return [np.ascontiguousarray(c) for c in cos], [np.ascontiguousarray(s) for s in sin]


for sp in ((6, 5, 8), (8, 6)):
    def fo_make(dtype, ext, sp=sp):
        csp = sp[:-1] + (sp[-1] // 2 + 1,)
        cos, sin = _luts(sp, NP[dtype])
        return {"F": rnd(_seed(24, *sp), (2, len(sp)) + csp + (2,), dtype), "cos": cos, "sin": sin}

    def fo_call(ext, t):
        assert ext.fluid_operator(t["F"], True, t["cos"], t["sin"], *PARAMS) is None
        return {"F": t["F"]}

    def fo_ref(a):
        F = a["F"].copy()
        orc.fluid_operator(F, True, a["cos"], a["sin"], *PARAMS)
        return {"F": F}
    # F is a buffer of complex elements: 2 is the only offset of 1 .. 3 the entry point takes (the others:
    # test_fluid_operator_rejects_a_buffer_off_the_complex_alignment)
    add(f"fluid_operator {sp}", ["fluid_operator"], fo_make, fo_call, fo_ref, {"F": "bits"}, offsets={"F": (2,)})


def _fluid_path(fast):
    def path(dtype, offs):
        if dtype == F64 or fast == "fluid_generic":
            return {"fluid_generic": 1}
        return {("fluid_generic" if "m" in offs else fast): 1}   # the gate tests m (out and work are the shim's own)
    return path


_GENERATION = {}
for sp, fast, dtypes in (((128, 128), "fluid_2d", BOTH), ((64, 64, 64), "fluid_lds", (F32,)), ((24, 20, 28), "fluid_generic", BOTH)):
    for inverse in (True, False):
        def fm_make(dtype, ext, sp=sp):
            cos, sin = _luts(sp, NP[dtype])
            return {"m": rnd(_seed(25, *sp), (2, len(sp)) + sp, dtype), "cos": cos, "sin": sin}

        def fm_call(ext, t, sp=sp, inverse=inverse):
            from lagomorph_amd import metric

            key = (sp, t["m"].dtype)   # one generation per LUT contents (include/lagomorph_hip.h)
            if key not in _GENERATION:
                _GENERATION[key] = next(metric._LUT_GENERATION)
            return {"out": ext.fluid_metric(t["m"], inverse, t["cos"], t["sin"], *PARAMS, lut_generation=_GENERATION[key])}
        add(f"fluid_metric {sp} inverse={inverse}", ["fluid_metric"], fm_make, fm_call,
            lambda a, inverse=inverse: {"out": orc.fluid_metric_apply(a["m"], PARAMS, inverse)}, {"out": "close"},
            dtypes=dtypes, path=_fluid_path(fast))


# ---------------------------------------------------------------------------------------------------- lincomb

COEFFS = [1.25, -0.37, 2.5e-3, 11.0]
for n, k, alias in itertools.product((64, 63), (1, 2, 3, 4), (False, True)):
    def lc_make(dtype, ext, n=n, k=k):
        rng = _seed(26, n, k)
        return {f"x{i}": rnd(rng, (n,), dtype) for i in range(k)}

    def lc_call(ext, t, k=k, alias=alias):
        terms = [(COEFFS[i], t[f"x{i}"]) for i in range(k)]
        if not alias:
            return {"out": ext.lincomb(terms)}
        out = ext.lincomb(terms, out=t["x0"])   # in place on the first term, as the momentum update of lddmm_step
        assert out is t["x0"]
        return {"out": out}

    def lc_ref(a, k=k):
        xs = [dev(a[f"x{i}"]) for i in range(k)]    # the left-to-right fma chain: torch's add(alpha=...) on the device
        want = COEFFS[0] * xs[0]
        for c, x in zip(COEFFS[1:k], xs[1:k]):
            want = torch.add(want, x, alpha=c)
        return {"out": want}
    add(f"lincomb K={k} n={n} alias={alias}", ["lincomb"], lc_make, lc_call, lc_ref, {"out": "bits"},
        pair=("x0", "x1") if k > 1 else None)


# ---------------------------------------------------------------------------------------------------- the tests

RAN = {"cases": 0, "calls": 0}
PAIRS = [pytest.param(c, dt, id=c.name.replace(" ", "_") + ("-f32" if dt == F32 else "-f64")) for c in CASES for dt in c.dtypes]


@pytest.mark.parametrize("case,dtype", PAIRS)
def test_offset_arguments(ext, case, dtype):
    RAN["calls"] += run_case(ext, case, dtype)
    RAN["cases"] += 1


# functions of lagomorph_ext that take no device tensor, each by name; everything else must be in the table above
NO_TENSOR = {
    "get_tuning", "default_tuning", "tune", "set_debug_mode", "set_splat_mode", "set_splat_tile", "set_splat_shear",
    "set_splat_mc", "set_splat_shear_mc", "set_fluid_tuning", "set_launch_order", "set_stencil_tile", "set_gather_window",
    "set_compose_near", "set_vector_kernels", "set_fluid_mode",                       # tuning setters and getters
    "version", "path_launches", "reversed_launches",                                 # version and counters
    "mi_bins", "mi_range", "edt_spacing", "ffd_spacing", "ffd_grid_shape",           # argument parsers
    "label_mode", "label_count", "label_overlap_chunks", "edt_where",
    "fluid_cache_clear", "fluid_cache_entries", "fft_plan_state",                    # cache and plan inspectors
}


def test_every_entry_point_has_its_case():
    from lagomorph_amd import lagomorph_ext as shim

    public = {n for n, f in vars(shim).items()
              if inspect.isfunction(f) and f.__module__ == shim.__name__ and not n.startswith("_")}
    covered = {e for c in CASES for e in c.entries}
    assert covered <= public, f"cases for entry points that do not exist: {sorted(covered - public)}"
    assert NO_TENSOR <= public, f"excluded names that do not exist: {sorted(NO_TENSOR - public)}"
    assert not covered & NO_TENSOR
    missing = public - covered - NO_TENSOR
    assert not missing, f"entry points without an alignment case: {sorted(missing)}"


def test_cases_cover_both_sides_of_every_gate():
    """For every gate of DESIGN.md's table whose paths are counted, one case whose control takes the fast path and whose
    offset run takes the sibling (the assertion itself is run_case's)."""
    for fast, pointer in (("gather_window", "I"), ("gather_window", "v"), ("gather_window_near", "v"), ("fluid_2d", "m"),
                          ("fluid_lds", "m")):
        hits = [c for c in CASES if c.path is not None and F32 in c.dtypes
                and c.path(F32, frozenset()) == {fast: 1} and c.path(F32, frozenset([pointer])) not in (None, {fast: 1})]
        assert hits, (fast, pointer)


@pytest.mark.parametrize("dtype", BOTH, ids=["f32", "f64"])
@pytest.mark.parametrize("sp", [(6, 5, 8), (8, 6)], ids=str)
def test_fluid_operator_rejects_a_buffer_off_the_complex_alignment(ext, dtype, sp):
    """An odd element offset puts the interleaved-complex buffer off its element size: the entry point refuses it
    (csrc/metric.hip: fluid_operator_impl) and touches nothing."""
    csp = sp[:-1] + (sp[-1] // 2 + 1,)
    F = rnd(_seed(24, *sp), (2, len(sp)) + csp + (2,), dtype)
    cos, sin = _luts(sp, NP[dtype])
    for off in (1, 3):
        v, buf = offset_view(dev(F), off)
        with pytest.raises(RuntimeError, match="aligned to a complex element"):
            ext.fluid_operator(v, True, [dev(c) for c in cos], [dev(s) for s in sin], *PARAMS)
        torch.cuda.synchronize()
        assert margins_intact(buf, v) == [] and torch.equal(v, dev(F))


# ---- end to end: a shoot and a matching step on momenta, images and an atlas that all sit at offset 1

def _smooth_np(rng, shape, sigma):
    from scipy.ndimage import gaussian_filter

    return gaussian_filter(rng.standard_normal(shape), sigma=[0, 0] + [sigma] * (len(shape) - 2), mode="wrap")


@pytest.mark.parametrize("dtype,tol", [(F64, 1e-12), (F32, 1e-5)], ids=["f64", "f32"])
@pytest.mark.parametrize("sp", [(16, 18, 20), (20, 24)], ids=str)
def test_expmap_and_lddmm_step_at_offset_one(ext, sp, dtype, tol):
    """expmap (5 steps; B = 3, so that the stream-split forward shoot cuts its sub-batch views out of the offset tensor)
    has the bits of the same call on aligned copies, split or not, with and without autograd; one lddmm_step agrees
    with the aligned step at the bound tests/test_gpu_lddmm_step.py uses for the same formulas in another summation
    order (the step's scatter-adds), its in-place momentum update stays inside the view, and no margin changes."""
    import lagomorph_amd as lm
    from lagomorph_amd import lddmm

    rng = np.random.default_rng([27, *sp])
    d, B = len(sp), 3
    met = lm.FluidMetric([0.1, 0.0, 0.01])
    base = torch.from_numpy(_smooth_np(rng, (1, 1) + sp, 1.5)).to(dtype).cuda()
    base = (base / base.std()).contiguous()
    imgs = (base + 0.2 * torch.from_numpy(_smooth_np(rng, (B, 1) + sp, 1.0)).to(dtype).cuda()).contiguous()
    m = torch.from_numpy(_smooth_np(rng, (B, d) + sp, 1.5)).to(dtype).cuda()
    m = (m * (1.5 / met.sharp(m).abs().max())).contiguous()

    def placed(off):
        return [offset_view(x, off) for x in (m, imgs, base)]

    def intact(views, what):
        for v, buf in views:
            assert margins_intact(buf, v) == [], what

    default = lddmm.EXPMAP_STREAMS
    shots = {}
    try:
        for off in (0, 1):
            views = placed(off)
            mo = views[0][0]
            assert mo.data_ptr() % 16 == (off * mo.element_size()) % 16
            with torch.no_grad():
                lddmm.EXPMAP_STREAMS = 1
                one = lm.expmap(met, mo, num_steps=5)
                lddmm.EXPMAP_STREAMS = 2
                two = lm.expmap(met, mo, num_steps=5)    # sub-batches [0:1] and [1:3] on streams of their own
            lddmm.EXPMAP_STREAMS = default
            mg, gbuf = offset_view(m, off)
            grad = lm.expmap(met, mg.requires_grad_(True), num_steps=5).detach()
            torch.cuda.synchronize()
            intact(views + [(mg.detach(), gbuf)], f"expmap offset {off}")
            assert torch.equal(two, one), f"the stream-split shoot differs from the unsplit one at offset {off}"
            assert torch.equal(grad, one)
            assert not torch.isnan(one).any()
            shots[off] = one
    finally:
        lddmm.EXPMAP_STREAMS = default
    assert torch.equal(shots[1], shots[0]), "expmap at offset 1 differs from the aligned call"

    steps = {}
    for off in (0, 1):
        views = placed(off)
        (mo, _), (io, _), (bo, bbuf) = views
        I = bo.requires_grad_(True)
        out, loss, reg = lm.lddmm_step(I, mo, io, lm.FluidMetric([0.1, 0.0, 0.01]), 2 * B, integration_steps=5,
                                       reg_weight=1e-2, learning_rate_pose=1e-3)
        torch.cuda.synchronize()
        assert out.data_ptr() == mo.data_ptr()    # updated in place, inside the view
        intact([(v.detach(), b) for v, b in views], f"lddmm_step offset {off}")
        steps[off] = (loss.detach(), reg.detach(), out.detach().clone(), I.grad.clone())
        for x in steps[off]:
            assert not torch.isnan(x).any()
    for name, a, b in zip(("loss", "reg", "m", "I.grad"), steps[1], steps[0]):
        err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
        assert err <= tol, (name, err)
    assert float((steps[1][2] - m).abs().max()) > 0    # the step moved the momenta


# ---- the guarded rocFFT plan: what a caller reaches by default.  Last in the file.

def test_zz_rocfft_default_shape_at_offset_one_is_right_or_loud(ext):
    """(8192, 4) float32 is the one shape class the default mode hands to the guarded rocFFT plan
    (tests/test_gpu_dispatch.py): with m one element off the alignment the call either returns what the oracle returns
    or the spot check's RuntimeError comes back, as in test_rocfft_fallback_is_right_or_loud."""
    import lagomorph_amd as lm

    sp = (8192, 4)
    m = rnd(_seed(28, *sp), (1, 2) + sp, F32)
    met = lm.FluidMetric([0.1, 0.0, 0.01])
    want = orc.fluid_metric_apply(m, [0.1, 0.0, 0.01], True)
    for off in (0, 1):
        v, buf = offset_view(dev(m), off)
        before = ext.path_launches("fluid_rocfft")
        try:
            got = met.sharp(v)
        except RuntimeError as e:
            assert "rocFFT returned a WRONG" in str(e), e
            print(f"NOTE rocFFT guard fired for {sp} at offset {off}: {e}")
            continue
        finally:
            torch.cuda.synchronize()
        assert ext.path_launches("fluid_rocfft") == before + 1
        assert margins_intact(buf, v) == []
        assert_close(got, want, F32, f"alignment rocFFT default shape offset {off}")
        print(f"rocFFT default shape {sp} at offset {off}: within the bound")
