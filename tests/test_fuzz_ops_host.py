"""CPU: the random cases, references and judges of tests/fuzz_ops_cases.py, which tools/fuzz_ops.py and
tests/test_gpu_fuzz.py run on the GPU.  No GPU and no import of the library here.

  * replay: a case generated alone is the case generated in a sequence;
  * coverage: over exactly the cases the GPU test runs (fuzz_ops_cases.SEED, COUNTS) every tag of every family occurs at
    least twice -- the tags are listed HERE, so a gate that stops being generated fails here;
  * validity: every case passes the restated argument checks of its entry point;
  * the judges accept the float64 reference rounded to the case's dtype and the family's native-precision restatement, on
    every case: the bounds are reachable by a correct implementation on these random inputs;
  * the judges reject a wrong result: five corruptions of the reference output, each reported.
"""
import numpy as np
import pytest

import fuzz_ops_cases as fc

EXPECTED_TAGS = {
    "surface_distance": {"2d", "3d", "unit_spacing", "anisotropic", "line_gt256", "lines_le256", "one_label", "several_labels",
                         "empty_surface", "same_structure"},
    "lncc": {"2d", "3d", "corr", "affine", "indep", "wrap", "zero", "per_axis_sigma", "scalar_sigma", "row_gt128", "row_le128",
             "strided_several_tiles", "strided_one_tile", "unfiltered_axis"},
    "bspline": {"2d", "3d", "x_staged", "x_long", "y_staged", "y_long", "z_staged", "z_long", "adjoint", "forward", "broadcast",
                "per_item", "need_both", "need_separate", "rows_70", "rows_few"},
    "energy": {"2d", "3d", "diffusion", "bending", "unit_spacing", "anisotropic", "scale", "no_scale", "thin_axis", "affine",
               "x_one_tile", "x_several_tiles", "x_whole_tiles", "x_ragged_tile", "y_one_tile", "y_several_tiles", "y_whole_tiles",
               "y_ragged_tile", "z_one_tile", "z_several_tiles", "z_whole_tiles", "z_ragged_tile"},
    "ffd_expand": {"2d", "3d", "spacing_1", "one_cell", "last_plane_unused",
                   "x_one_tile", "x_several_tiles", "x_whole_tiles", "x_ragged_tile", "y_one_tile", "y_several_tiles", "y_whole_tiles",
                   "y_ragged_tile", "z_one_tile", "z_several_tiles", "z_whole_tiles", "z_ragged_tile"},
    "invert_displacement": {"2d", "3d", "one_step", "fixed_point", "no_step", "steps", "one_block", "several_blocks"},
    "gaussian_smooth": {"axes_0", "axes_1", "axes_2", "axes_3", "wrap", "zero", "new", "out", "accumulate", "row_gt128", "row_le128",
                        "three_whole_line", "three_no_whole_line", "z_segments", "strided_one_tile", "strided_several_tiles",
                        "radius_above_extent"},
    "jacobian_determinant": {"2d", "3d", "thin_axis", "one_block", "several_blocks", "displacement", "plain_jacobian"},
    "joint_histogram": {"hist_one_chunk", "hist_several_chunks", "bwd_one_chunk", "bwd_several_chunks", "auto_range",
                        "explicit_range", "values_on_bin_edges", "values_outside_range", "rep_full", "rep_capped"},
    "warp_labels": {"2d", "plain_3d", "slab", "slab_ragged_last", "slab_whole", "slab_last_wholly_invalid", "carry_j",
                    "no_carry_j", "carry_i", "no_carry_i", "broadcast", "per_item", "vote", "nearest"},
    "label_overlap": {"one_chunk", "several_chunks", "one_reducer_group", "several_reducer_groups", "rep4", "rep2", "rep1",
                      "vector_tail", "whole_vectors"},
    "distance_transform": {"z_le256", "z_le512", "z_gt512", "y_le256", "y_le512", "y_gt512", "x_le256", "x_le512", "x_gt512",
                           "unit_spacing", "anisotropic", "2d", "3d"},
    "interp_points": {"one_workgroup", "several_workgroups", "whole_waves", "ragged_wave", "broadcast", "per_item", "crowd",
                      "on_grid_points", "2d", "3d", "thin_z"},
}
families = pytest.mark.parametrize("family", fc.FAMILIES)
HANDFUL = 12   # cases of a family that the corruptions are tried on


def _same_case(a, b):
    return (a["sp"] == b["sp"] and a["N"] == b["N"] and a["dtype"] == b["dtype"] and a["tags"] == b["tags"] and a["params"] == b["params"]
            and a["inputs"].keys() == b["inputs"].keys()
            and all(v.dtype == b["inputs"][k].dtype and np.array_equal(v, b["inputs"][k]) for k, v in a["inputs"].items()))


def test_the_families_and_their_tags_are_the_listed_ones():
    assert set(EXPECTED_TAGS) == set(fc.FAMILIES) == set(fc.COUNTS) == set(fc.CAPS) == set(fc.RULES)
    assert set(fc.FAMILIES) | set(fc.PENDING) == set(fc.FAMILY_ID) and len(set(fc.FAMILY_ID.values())) == len(fc.FAMILY_ID)
    for f in fc.FAMILIES:
        assert set(fc.TAGS[f]) == EXPECTED_TAGS[f], f


@families
def test_a_case_alone_is_the_case_of_the_sequence(family):
    seq = fc.cases(family, 3, 8)
    for i in (7, 0, 4):
        assert _same_case(fc.case(family, 3, i), seq[i]), i
    assert not _same_case(seq[0], seq[1]) and not _same_case(fc.case(family, 4, 0), seq[0])


@families
def test_every_tag_occurs_twice_in_the_cases_of_the_gpu_test(family):
    seen = {t: 0 for t in EXPECTED_TAGS[family]}
    for i in range(fc.COUNTS[family]):
        for t in fc.case(family, fc.SEED, i)["tags"]:
            seen[t] += 1          # (a tag that is not listed is a KeyError)
    assert min(seen.values()) >= 2, {t: n for t, n in seen.items() if n < 2}


@families
def test_every_case_passes_the_entry_points_checks(family):
    for i in range(fc.COUNTS[family]):
        c = fc.case(family, fc.SEED, i)
        assert fc.valid(c) == [], (i, fc.valid(c))
        assert int(np.prod(c["sp"])) <= fc.CAPS[family] and 1 <= c["N"] <= 3
        assert all(np.isfinite(v).all() for v in c["inputs"].values() if v.dtype.kind == "f"), i


@families
def test_the_judge_accepts_the_reference_and_its_native_restatement(family):
    natives, worst = 0, {}
    for i in range(fc.COUNTS[family]):
        c = fc.case(family, fc.SEED, i)
        assert fc.judge(family, c, fc.rounded(c), worst) == [], (i, c["sp"], sorted(c["tags"]))
        nat = fc.native(c)
        if nat is not None:
            natives += 1
            assert fc.judge(family, c, nat, worst) == [], (i, c["sp"], sorted(c["tags"]))
    print(f"{family}: {natives} native restatements of {fc.COUNTS[family]} cases; largest fractions of the bounds {worst}")
    assert natives >= (fc.COUNTS[family] // 2 if family != "warp_labels" else 0)   # (warp_labels' reference IS the native arithmetic)
    assert all(v <= 1.0 for v in worst.values())


def _tolerance(c, name, at):
    """The family's tolerance on entry `at` of output `name` (0 for an output judged bit for bit)."""
    import scatter_bound

    rule, ref = fc.RULES[c["family"]][name], fc.reference(c)
    if rule == "rel":
        return fc.RTOL[c["dtype"]] * float(np.abs(ref[name]).max())
    if rule == "cells":
        return float(scatter_bound.cell_bound(ref["_wide"][1], ref["_wide"][2], c["dtype"])[at])
    if rule == "surface":
        return 1e-6 * abs(float(ref[name][at]))
    if rule == "bcells":
        import bspline_ref

        return float(bspline_ref.cell_bound(ref["_wide"][1], ref["_wide"][2], c["dtype"], len(c["sp"]))[at])
    if rule == "energy":
        return 1e-12 * float(np.abs(ref["E"]).max()) if c["dtype"] == np.float64 else 1e-5 * float(ref["E"][at])
    if rule == "operator":
        s = c["inputs"].get("scale")
        if "affine" in c["tags"]:
            return float(ref["_bound"][at]) * fc.UNIT[c["dtype"]] / 2.0 ** -24
        if c["dtype"] == np.float64:
            return 1e-12 * float(np.abs(ref["_A"]).max()) * (float(np.abs(s).max()) if s is not None else 1.0)
        return float(ref["_bound"][at])
    if rule == "voxel":
        return min(float(ref["_vbound"][at]), fc.RTOL[c["dtype"]] * float(np.abs(ref[name]).max()))
    if rule == "entry":
        return 1e-12 * float(np.abs(ref[name]).max()) if c["dtype"] == np.float64 else float(ref["_ebound"][at])
    if rule == "edt" and "anisotropic" in c["tags"] and name == "squared":
        return fc.EDT_REL * float(ref["_sq64"][at])
    return 0.0


def corruptions(c, out):
    """(corruption, output name, outputs with that output corrupted) for every corruption that changes the output."""
    for name, ref in out.items():
        if name not in fc.judged(c):
            continue

        def put(kind, a):
            if not np.array_equal(a, ref, equal_nan=ref.dtype.kind == "f"):
                return [(kind, name, dict(out, **{name: a}))]
            return []

        flat = ref.reshape(-1)
        if flat.size >= 2:       # the last element of the last row of the last item takes its neighbour's value
            a = ref.copy()
            a.reshape(-1)[-1] = flat[-2]
            yield from put("last_element", a)
        if ref.shape[0] == c["N"] >= 2:
            a = ref.copy()
            a[0], a[-1] = ref[-1], ref[0]
            yield from put("items_exchanged", a)
        nz = ref.shape[-1]       # one voxel along the last axis, inside the last (ragged) tile of 64 only
        z0 = (nz - 1) // 64 * 64
        if nz - z0 >= 2:
            a = ref.copy()
            a[..., z0 + 1:] = ref[..., z0:-1]
            yield from put("shifted_in_the_last_tile", a)
        if ref.dtype.kind == "f":
            mag = np.where(np.isfinite(ref), np.abs(ref), -1.0)
            at = np.unravel_index(int(mag.argmax()), ref.shape)
            # the entry of largest |reference| moves by four tolerances (four ulps where the rule is bits); a reference
            # that is zero throughout (the plain Jacobian's determinant on a one-voxel axis) gives the rule no scale
            if mag[at] > 0:
                a = ref.copy()
                a[at] = ref[at] + max(4.0 * _tolerance(c, name, at), 4.0 * float(np.spacing(np.abs(ref[at]).astype(ref.dtype))))
                yield from put("four_tolerances", a)
        else:
            a = ref.copy()
            a.reshape(-1)[flat.size // 2] += 1
            yield from put("off_by_one", a)


@families
def test_the_judge_reports_every_corruption(family):
    done = {}
    for i in range(HANDFUL):
        c = fc.case(family, fc.SEED, i)
        out = fc.rounded(c)
        assert fc.judge(family, c, out) == []
        for kind, name, bad in corruptions(c, out):
            assert fc.judge(family, c, bad) != [], (i, kind, name, c["sp"], sorted(c["tags"]))
            done[kind] = done.get(kind, 0) + 1
    ints = any(v.dtype.kind in "iu" for v in out.values())
    floats = any(v.dtype.kind == "f" for v in out.values())
    want = {"last_element", "items_exchanged", "shifted_in_the_last_tile"} | ({"off_by_one"} if ints else set()) | ({"four_tolerances"} if floats else set())
    assert want <= set(done) and min(done.values()) >= 3, done
