"""Host walk of the affine box splat's candidate / ownership code (no GPU needed).

affine_splat_box_kernel (lagomorph_amd/csrc/affine.hip) gives every box of target cells the source voxels of a
candidate range and drops, silently, a source whose owner box does not list it.  The range comes from the inverse
matrix in double plus a slack of a few hundredths of a voxel (affine_box.hpp: affine_box_slack).
tests/native/affine_box_emul.hip includes that header and walks every source voxel of a grid through the functions
the kernel calls; these tests feed it the matrices of tests/affine_box_cases.py and assert that no source is left
out, on both sides of every threshold of affine_item_regular, and that a deliberately wrong slack IS noticed.

LAGO_BOX_MARGIN_REPORT=<file>: the per-case figures as JSON (profiles/affine_box_margin.md is made from it)."""
import json
import os

import numpy as np
import pytest

import affine_box_cases as cases
import native_build

pytestmark = native_build.needs_hipcc

REPORT = {}


def _build(tmp, name, extra=()):
    return native_build.build(tmp, "affine_box_emul.hip", wall=False, werror=False, extra=("-pthread", *native_build.GFX950, *extra),
                              compiler="hipcc", name=name)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    yield _build(tmp_path_factory.mktemp("affine_box_emul"), "affine_box_emul")
    out = os.environ.get("LAGO_BOX_MARGIN_REPORT")
    if out:
        json.dump(REPORT, open(out, "w"), indent=1)


def _num(x, dtype):
    x = dtype(x)
    return float(x).hex() if np.isfinite(x) else ("nan" if np.isnan(x) else ("inf" if x > 0 else "-inf"))


def walk(exe, tmp, rows, dtype=np.float32):
    """rows: [(name, shape, A, T)] -> {name: dict(regular, sources, uncovered, misowned, needed, shipped, worst)}"""
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        for name, shape, A, T in rows:
            vals = [_num(v, dtype) for v in np.asarray(A).reshape(-1)] + [_num(v, dtype) for v in np.asarray(T).reshape(-1)]
            f.write(" ".join([name, "f32" if dtype == np.float32 else "f64", *map(str, shape), *vals]) + "\n")
    r = native_build.run(exe, path, timeout=1800)
    out = {}
    for line in r.stdout.splitlines():
        p = line.split()
        out[p[0]] = dict(regular=int(p[1]), sources=int(p[2]), uncovered=int(p[3]), misowned=int(p[4]), needed=float(p[5]),
                         shipped=float(p[6]), worst=tuple(map(int, p[7:10])))
    assert list(out) == [r_[0] for r_ in rows], "one result line per case, in order"
    return out


def _assert_covered(res, shape):
    for name, r in res.items():
        assert r["regular"] == 1, f"{name}: meant to be regular"
        assert r["sources"] == int(np.prod(shape)), name
        assert r["misowned"] == 0, f"{name}: ownership is not a partition"
        # (sources sit on integers and the range is rounded outward: a source is dropped exactly when it lies 1 + slack or
        # more outside the preimage box, so the two figures must agree)
        assert (r["uncovered"] == 0) == (r["needed"] < 1.0 + r["shipped"]), (name, r)
        assert r["uncovered"] == 0, (f"{name} {shape}: {r['uncovered']} source(s) outside their owner's candidate range; needed "
                                     f"slack {r['needed']:.4f} at source {r['worst']}, shipped {r['shipped']:.4f}")


MILD_SHAPES = [(36, 20, 70), (8, 8, 48), (9, 17, 49), (7, 9, 97), (2, 2, 16), (16, 16, 200), (64, 64, 64)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mild_family_needs_no_slack_to_speak_of(emul, tmp_path, dtype):
    """identity and the matrices of test_affine_backward_tiled_splat, at the shapes the GPU suite runs (whole boxes, one
    cell over, a single box, the smallest grid the box path takes): covered, and the exact preimage box alone -- no
    slack -- misses a source by no more than float32 rounding of a position below 200 carried through an inverse with
    rows below 4: 200 * 2^-23 * 4 * a handful of roundings < 1e-3 voxels."""
    rng = np.random.default_rng(5)
    mats = cases.mild_matrices()
    for shape in MILD_SHAPES:
        rows, want = [], {}
        for k, A in mats.items():
            for t in range(2):
                T = (2.0 * rng.standard_normal(3) * (t > 0)).astype(np.float32)
                rows.append((f"{k}_t{t}", shape, A, T))
                want[f"{k}_t{t}"] = cases.MILD_REGULAR.get(k, True)
        res = walk(emul, tmp_path, rows, dtype)
        for name, r in res.items():
            assert bool(r["regular"]) == want[name], name
        reg = {k: r for k, r in res.items() if want[k]}
        _assert_covered(reg, shape)
        worst = max(r["needed"] for r in reg.values())
        REPORT[f"mild {shape} {np.dtype(dtype).name}"] = dict(cases=len(reg), needed=worst, shipped=next(iter(reg.values()))["shipped"], uncovered=0)
        assert worst <= 1e-3, (shape, worst)


@pytest.mark.parametrize("n", cases.EXTENTS)
@pytest.mark.parametrize("name", list(cases.ADVERSARIAL))
def test_adversarial_family_is_covered(emul, tmp_path, name, n):
    """Regular float32 matrices with entries of 500 .. 999.99 that cancel on in-grid sources and inverse row sums of
    3.5 .. 3.98, with translations aimed at every corner type of a box (tests/affine_box_cases.py).  No source may be
    outside its owner's range.  The needed slack is recorded, not asserted: whether the shipped slack has margin is the
    finding of profiles/affine_box_margin.md; that nothing is dropped is the requirement."""
    A = cases.adversarial_matrices()[name]
    shape = (n, 16, n)
    tr = cases.directed_translations(A, shape)
    res = walk(emul, tmp_path, [(t[0], shape, A, t[1]) for t in tr])
    _assert_covered(res, shape)
    worst = max(res.items(), key=lambda kv: kv[1]["needed"])
    REPORT[f"adversarial {name} {n}"] = dict(cases=len(res), needed=worst[1]["needed"], shipped=worst[1]["shipped"], uncovered=0,
                                             worst_case=worst[0], worst_source=worst[1]["worst"], inv_rowsum=cases.inv_rowsum(A),
                                             ranking=sorted(((r["needed"], k) for k, r in res.items()), reverse=True)[:4])


def test_adversarial_family_third_axis_and_partial_boxes(emul, tmp_path):
    """The same matrices on grids that whole boxes do not cover, with a third axis of 40 (three-entry rows then round three
    large products per position)."""
    for name, A in cases.adversarial_matrices().items():
        for shape in [(263, 40, 263), (321, 17, 300)]:
            tr = cases.directed_translations(A, shape, offsets=(0.0, 4e-3))
            res = walk(emul, tmp_path, [(t[0], shape, A, t[1]) for t in tr])
            _assert_covered(res, shape)
            worst = max(res.items(), key=lambda kv: kv[1]["needed"])
            REPORT[f"adversarial {name} {shape}"] = dict(cases=len(res), needed=worst[1]["needed"], shipped=worst[1]["shipped"], uncovered=0,
                                                         worst_case=worst[0], worst_source=worst[1]["worst"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_regular_decision_on_both_sides_of_every_threshold(emul, tmp_path, dtype):
    """affine_item_regular at adjacent float32 values around max |a| < 1e3, |det| > 1e-3 and inverse row sum <= 4; NaN,
    Inf and the zero matrix are not regular (host only: they are never sent to a GPU).  The regular ones are covered."""
    shape = (40, 16, 64)
    th = cases.threshold_matrices()
    rows = [(k, shape, A, np.array([0.75, -1.25, 2.5], np.float32)) for k, (A, _) in th.items()]
    rows += [(k, shape, A, np.zeros(3, np.float32)) for k, A in cases.nonfinite_matrices().items()]
    res = walk(emul, tmp_path, rows, dtype)
    for k, (_, regular) in th.items():
        assert bool(res[k]["regular"]) == regular, (k, res[k])
    for k in cases.nonfinite_matrices():
        assert res[k]["regular"] == 0, k
    _assert_covered({k: r for k, r in res.items() if r["regular"]}, shape)


def test_a_wrong_slack_is_noticed(tmp_path):
    """The walk can fail: built with the slack forced to -1.5 voxels (a define that exists for this test alone), it
    reports uncovered sources for a mild rotation.  Shown on the host, not by sending a wrong kernel to a GPU."""
    exe = _build(tmp_path, "affine_box_emul_broken", ["-DLAGO_TEST_BOX_SLACK=-1.5"])
    A = cases.mild_matrices()["rotation0"]
    res = walk(exe, tmp_path, [("rotation0", (36, 20, 70), A, np.array([0.5, -0.25, 1.0], np.float32))])["rotation0"]
    assert res["regular"] == 1 and res["shipped"] == -1.5
    assert res["uncovered"] > 0 and res["misowned"] == 0
    assert 0 <= res["needed"] < 1e-3   # the sources are where they should be; only the range is too small
