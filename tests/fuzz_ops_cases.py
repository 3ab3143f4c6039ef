"""Random cases of the operator families that tools/fuzz_parity.py does not cover, their references and their judges
(tools/fuzz_ops.py runs them on the GPU, tests/test_fuzz_ops_host.py holds this module to account without one).

`case(family, seed, index)` draws ONE case from its own stream np.random.default_rng([seed, FAMILY_ID, index]): the same
case whether it is generated alone or in a sequence, replayed by the triple.  A case is a dict

    family, seed, index, sp (the spatial shape), dtype, N,
    inputs  name -> numpy array           (what goes to the GPU)
    params  name -> plain Python value    (the call's other arguments)
    tags    the set of gate sides the case lies on (TAGS[family] lists every tag of a family)

The gates are the host code's own launch decisions, restated here next to the source line they come from.
`reference(case)` evaluates the family's float64 / integer reference (tests/*_ref.py) once per case and keeps it in the
dict; `native(case)` is the family's native-precision restatement where one exists; `judge(family, case, outputs)`
applies the family's EXISTING rule (named at each judge, with the test it is taken from) and returns the failures as
strings, no new tolerance anywhere.  This module needs numpy only; the reference modules are imported when a
reference is asked for (two of them call the CPU oracle).

PENDING lists the ids of FAMILY_ID without a generator (none at present; `bspline` covers bspline_prefilter and
interp_bspline, `distance_transform` and `surface_distance` are two families of csrc/edt.hip).
"""
import numpy as np

from parity_rule import RTOL, bits, close, units   # the project's rule: max|got - ref| <= RTOL max|ref|

# fixed for good: a family's id is part of its cases' streams
FAMILY_ID = {"jacobian_determinant": 1, "invert_displacement": 2, "gaussian_smooth": 3, "lncc": 4, "joint_histogram": 5,
             "warp_labels": 6, "label_overlap": 7, "distance_transform": 8, "interp_points": 9, "bspline": 10,
             "ffd_expand": 11, "energy": 12, "surface_distance": 13}
FAMILIES = ("jacobian_determinant", "invert_displacement", "gaussian_smooth", "joint_histogram", "warp_labels", "label_overlap",
            "distance_transform", "interp_points", "ffd_expand", "energy", "surface_distance", "lncc", "bspline")
PENDING = tuple(f for f in FAMILY_ID if f not in FAMILIES)

SEED = 20          # the seed of the cases tests/test_gpu_fuzz.py runs
# cases per family in the GPU test: the smallest count at which every tag below occurs twice, rounded up to about 5 s of
# generating and evaluating references on the CPU (profiles/fuzz_ops.md has the measurements)
COUNTS = {"jacobian_determinant": 200, "invert_displacement": 120, "gaussian_smooth": 250, "joint_histogram": 120,
          "warp_labels": 200, "label_overlap": 150, "distance_transform": 200, "interp_points": 300, "ffd_expand": 300,
          "energy": 300, "surface_distance": 100, "lncc": 100, "bspline": 100}
# voxels of one item at most: the largest at which the family's reference stays at about 0.2 s a case here, and never
# below the family's gates (profiles/fuzz_ops.md)
CAPS = {"jacobian_determinant": 100_000, "invert_displacement": 20_000, "gaussian_smooth": 1_200_000, "joint_histogram": 40_000,
        "warp_labels": 55_000, "label_overlap": 2_000_000, "distance_transform": 8_000, "interp_points": 1_000_000,
        "ffd_expand": 40_000, "energy": 100_000, "surface_distance": 6_000, "lncc": 30_000, "bspline": 6_000}

EXTENTS = (1, 2, 3, 5, 8, 16, 17, 32, 33, 63, 64, 65, 70, 128, 130, 256, 257, 300, 513)   # around the tiles of 8, 16, 64, 256, 512
KBLOCK = 256       # common.hpp:27 kBlock

TAGS = {
    "surface_distance": ("2d", "3d", "unit_spacing", "anisotropic", "line_gt256", "lines_le256", "one_label", "several_labels",
                         "empty_surface", "same_structure"),
    "lncc": ("2d", "3d", "corr", "affine", "indep", "wrap", "zero", "per_axis_sigma", "scalar_sigma", "row_gt128", "row_le128",
             "strided_several_tiles", "strided_one_tile", "unfiltered_axis"),
    "bspline": ("2d", "3d", "x_staged", "x_long", "y_staged", "y_long", "z_staged", "z_long", "adjoint", "forward", "broadcast",
                "per_item", "need_both", "need_separate", "rows_70", "rows_few"),
    "energy": ("2d", "3d", "diffusion", "bending", "unit_spacing", "anisotropic", "scale", "no_scale", "thin_axis", "affine") + tuple(
        f"{a}_{t}" for a in "xyz" for t in ("one_tile", "several_tiles", "whole_tiles", "ragged_tile")),
    "ffd_expand": ("2d", "3d", "spacing_1", "one_cell", "last_plane_unused") + tuple(
        f"{a}_{t}" for a in "xyz" for t in ("one_tile", "several_tiles", "whole_tiles", "ragged_tile")),
    "invert_displacement": ("2d", "3d", "one_step", "fixed_point", "no_step", "steps", "one_block", "several_blocks"),
    "gaussian_smooth": ("axes_0", "axes_1", "axes_2", "axes_3", "wrap", "zero", "new", "out", "accumulate", "row_gt128", "row_le128",
                        "three_whole_line", "three_no_whole_line", "z_segments", "strided_one_tile", "strided_several_tiles",
                        "radius_above_extent"),
    "jacobian_determinant": ("2d", "3d", "thin_axis", "one_block", "several_blocks", "displacement", "plain_jacobian"),
    "joint_histogram": ("hist_one_chunk", "hist_several_chunks", "bwd_one_chunk", "bwd_several_chunks", "auto_range",
                        "explicit_range", "values_on_bin_edges", "values_outside_range", "rep_full", "rep_capped"),
    "warp_labels": ("2d", "plain_3d", "slab", "slab_ragged_last", "slab_whole", "slab_last_wholly_invalid", "carry_j",
                    "no_carry_j", "carry_i", "no_carry_i", "broadcast", "per_item", "vote", "nearest"),
    "label_overlap": ("one_chunk", "several_chunks", "one_reducer_group", "several_reducer_groups", "rep4", "rep2", "rep1",
                      "vector_tail", "whole_vectors"),
    "distance_transform": ("z_le256", "z_le512", "z_gt512", "y_le256", "y_le512", "y_gt512", "x_le256", "x_le512",
                           "x_gt512", "unit_spacing", "anisotropic", "2d", "3d"),
    "interp_points": ("one_workgroup", "several_workgroups", "whole_waves", "ragged_wave", "broadcast", "per_item",
                      "crowd", "on_grid_points", "2d", "3d", "thin_z"),
}


# ------------------------------------------------------------------ shared pieces

def _rng(family, seed, index):
    return np.random.default_rng([int(seed), FAMILY_ID[family], int(index)])


def _shape(rng, cap, d=None, least=0, extents=EXTENTS, low=1):
    """A 2D or 3D shape of extents from `extents` (each >= low), permuted, of `least` <= voxels <= cap."""
    d = int(rng.choice([2, 3, 3])) if d is None else d
    ext = [e for e in extents if e >= low]
    for _ in range(1000):
        sp = tuple(int(x) for x in rng.choice(ext, size=d))
        if least <= int(np.prod(sp)) <= cap:
            return tuple(int(x) for x in rng.permutation(sp))
    raise RuntimeError(f"no shape of {d} axes with {least}..{cap} voxels")


def _dtype(rng):
    return np.dtype(np.float32) if rng.random() < 0.7 else np.dtype(np.float64)


def _smooth3(x, axes):
    for a in axes:
        x = (np.roll(x, 1, a) + 2 * x + np.roll(x, -1, a)) / 4
    return x


def _displacement(rng, N, sp, dtype, amps=(0.3, 1.5, 6.0, 40.0)):
    """(N, d, *sp): normal with an amplitude from sub-voxel to far out of range; half of them smoothed once, a fifth
    rounded to integers (samples on grid points)."""
    d = len(sp)
    amp = float(rng.choice(amps))
    u = amp * rng.standard_normal((N, d) + sp)
    if rng.random() < 0.5:
        u = _smooth3(u, range(2, 2 + d))
    if rng.random() < 0.2 and amp >= 1.0:   # (a sub-voxel field would round to zero)
        u = np.round(u)
    return np.ascontiguousarray(u.astype(dtype))


def _new(family, seed, index, sp, dtype, N):
    return {"family": family, "seed": int(seed), "index": int(index), "sp": tuple(sp), "dtype": np.dtype(dtype), "N": int(N),
            "inputs": {}, "params": {}, "tags": set()}


# ------------------------------------------------------------------ jacobian_determinant  (csrc/diff.hip: jacdet_impl)

def _case_jacobian_determinant(rng, c0):
    sp = _shape(rng, CAPS["jacobian_determinant"])
    N, dtype = int(rng.integers(1, 4)), _dtype(rng)
    c = _new(*c0, sp, dtype, N)
    c["inputs"]["u"] = _displacement(rng, N, sp, dtype, amps=(0.05, 0.3, 3.0))
    c["inputs"]["go"] = rng.standard_normal((N, 1) + sp).astype(dtype)
    c["params"]["displacement"] = bool(rng.random() < 0.5)
    nvox = int(np.prod(sp))
    c["tags"] |= {f"{len(sp)}d", "displacement" if c["params"]["displacement"] else "plain_jacobian",
                  "one_block" if nvox <= KBLOCK else "several_blocks"}   # common.hpp:116 make_geom: kBlock voxels a block
    if min(sp) == 1:
        c["tags"].add("thin_axis")
    return c


def _valid_jacobian_determinant(c):
    u, go = c["inputs"]["u"], c["inputs"]["go"]
    d = len(c["sp"])
    # lagomorph_ext._check_jacdet / jacobian_determinant_backward; args.hpp:66 check_volume with kPlane29
    return [m for ok, m in ((d in (2, 3), "dim"), (u.shape == (c["N"], d) + c["sp"], "u shape"), (go.shape == (c["N"], 1) + c["sp"], "go shape"),
                            (u.dtype == go.dtype == c["dtype"], "dtype"), (min(c["sp"]) >= 1 and np.prod(c["sp"]) < 2 ** 29, "extent"),
                            (bool(np.isfinite(u).all() and np.isfinite(go).all()), "finite")) if not ok]


def _ref_jacobian_determinant(c):
    import jacdet_ref

    u, go, disp = c["inputs"]["u"], c["inputs"]["go"], c["params"]["displacement"]
    return {"forward": jacdet_ref.forward(u, disp), "backward": jacdet_ref.backward(go, u, disp)}


def _native_jacobian_determinant(c):
    import jacdet_ref

    u, go, disp = c["inputs"]["u"], c["inputs"]["go"], c["params"]["displacement"]
    return {"forward": jacdet_ref.torch_forward(u, disp), "backward": jacdet_ref.torch_backward(go, u, disp)}


def _judge_jacobian_determinant(c, out, ref, fails, worst):
    """tests/test_gpu_jacdet.py: forward bit for bit, backward within RTOL x max|reference|."""
    bits(out["forward"], ref["forward"], "forward", fails=fails)
    close(out["backward"], ref["backward"], c["dtype"], "backward", fails=fails, worst=worst)


# ------------------------------------------------------------------ joint_histogram / mi_backward  (csrc/mi.hip)

MI_CHUNK_MIN, MI_BWD_CHUNK, MI_MAX_REP = 4096, 8192, 8        # mi.hip:22, :23, :25
SLAB_BYTES, TABLE_LDS_BYTES = 8 << 20, 64 * 1024              # chunk_table.hpp:18, :19


def chunks_wanted(table_bytes, rows, nvox, chunk_min, slab_bytes=SLAB_BYTES):
    """chunk_table.hpp:24."""
    by_size = (nvox + chunk_min - 1) // chunk_min
    cap = slab_bytes // table_bytes // max(rows, 1)
    return max(min(by_size, cap), 1)


def split_row(nvox, want, least):
    """chunk_table.hpp:37: (chunks, elements per chunk)."""
    c = max(min((nvox + least - 1) // least, want), 1)
    per = ((nvox + c - 1) // c + 3) // 4 * 4
    return ((nvox + per - 1) // per if per else 1), per


def _case_joint_histogram(rng, c0):
    lead = (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
    rows = lead[0] * lead[1]
    big = rng.random() < 0.4   # (rows of one chunk are the commoner draw otherwise)
    sp = _shape(rng, CAPS["joint_histogram"], least=MI_BWD_CHUNK + 1 if big else 0)
    dtype = _dtype(rng)
    c = _new(*c0, sp, dtype, lead[0])
    B = int(rng.choice([4, 5, 8, 31, 32, 33, 64, int(rng.integers(4, 65))]))
    shape = lead + sp
    I = rng.standard_normal(shape).astype(np.float32)
    J = (np.float32(0.8) * I + np.float32(0.6) * rng.standard_normal(shape).astype(np.float32)).astype(np.float32)
    if rng.random() < 0.3:   # smooth images: neighbouring voxels share their bins
        I = _smooth3(_smooth3(I, range(2, len(shape))), range(2, len(shape))).astype(np.float32)
    rI = rJ = None
    if rng.random() < 0.6:
        c["tags"].add("explicit_range")
        rI, rJ = (float(rng.choice([-1.5, -1.0, -3.0])), float(rng.choice([1.25, 1.0, 3.5]))), (-1.25, float(rng.choice([1.75, 4.0])))
        if rng.random() < 0.5:   # values exactly on the edges of the bins of I: lo + k (hi - lo) / (B - 3), and on lo and hi
            edges = (rI[0] + np.arange(B - 2) * ((rI[1] - rI[0]) / (B - 3))).astype(np.float32)
            at = rng.random(shape) < 0.2
            I = np.where(at, edges[rng.integers(0, B - 2, shape)], I).astype(np.float32)
            c["tags"].add("values_on_bin_edges")
        if bool(((I < rI[0]) | (I > rI[1]) | (J < rJ[0]) | (J > rJ[1])).any()):
            c["tags"].add("values_outside_range")
    else:
        c["tags"].add("auto_range")
    c["inputs"].update(I=I.astype(dtype), J=J.astype(dtype), G=rng.standard_normal(lead + (B, B)))
    c["params"].update(bins=B, range_I=rI, range_J=rJ)
    nvox = int(np.prod(sp))
    hist = split_row(nvox, chunks_wanted(B * B * 8, rows, nvox, MI_CHUNK_MIN), MI_CHUNK_MIN)[0]   # mi.hip:157 plan_tables<long long>
    bwd = split_row(nvox, 1 << 30, MI_BWD_CHUNK)[0]                                               # mi.hip:182
    c["tags"] |= {"hist_one_chunk" if hist == 1 else "hist_several_chunks", "bwd_one_chunk" if bwd == 1 else "bwd_several_chunks",
                  # mi.hip:164: replicas of the table as LAGO_MI_MAX_REP and 64 KB of LDS allow
                  "rep_full" if MI_MAX_REP * B * B * 8 <= TABLE_LDS_BYTES else "rep_capped"}
    return c


def _mi_ranges(c):
    import mi_ref

    I, J = c["inputs"]["I"], c["inputs"]["J"]
    rI, rJ = c["params"]["range_I"], c["params"]["range_J"]
    return (mi_ref.auto_range(I) if rI is None else rI), (mi_ref.auto_range(J) if rJ is None else rJ)


def _valid_joint_histogram(c):
    I, J, G, B = c["inputs"]["I"], c["inputs"]["J"], c["inputs"]["G"], c["params"]["bins"]
    bad = []
    if not (4 <= B <= 64 and isinstance(B, int)):                      # lagomorph_ext.mi_bins
        bad.append("bins")
    for r in (c["params"]["range_I"], c["params"]["range_J"]):          # lagomorph_ext.mi_range
        if r is not None and not (np.isfinite(r[0]) and np.isfinite(r[1]) and r[0] < r[1]):
            bad.append("range")
    if not (I.shape == J.shape and I.ndim - 2 in (2, 3) and I.dtype == J.dtype == c["dtype"]):   # _check_mi
        bad.append("shape or dtype")
    if G.dtype != np.float64 or G.shape != I.shape[:2] + (B, B):       # mi_backward
        bad.append("G")
    if not (np.isfinite(I).all() and np.isfinite(J).all() and np.isfinite(G).all()) or np.prod(c["sp"]) > 2 ** 30:
        bad.append("finite or extent")
    return bad


def _ref_joint_histogram(c):
    import mi_ref

    I, J, G, B = c["inputs"]["I"], c["inputs"]["J"], c["inputs"]["G"], c["params"]["bins"]
    rI, rJ = _mi_ranges(c)
    dI, dJ = mi_ref.backward(G, I, J, B, rI, rJ)
    return {"P": mi_ref.joint_histogram(I, J, B, rI, rJ), "dI": dI, "dJ": dJ}


def _native_joint_histogram(c):
    """The integer path of mi_ref by its plain statement (np.add.at on int64), and the gradients rounded to the dtype."""
    import mi_ref

    I, J, B = c["inputs"]["I"], c["inputs"]["J"], c["params"]["bins"]
    if I.size > 40_000:
        return None   # (np.add.at: seconds above this; the bincount route is tied to it by tests/test_mi_host.py)
    rI, rJ = _mi_ranges(c)
    P = mi_ref.P_of(mi_ref.histogram_int_add_at(I, J, B, rI, rJ), int(np.prod(c["sp"]))).reshape(I.shape[:2] + (B, B))
    ref = reference(c)
    return {"P": P, "dI": ref["dI"].astype(c["dtype"]), "dJ": ref["dJ"].astype(c["dtype"])}


def _judge_joint_histogram(c, out, ref, fails, worst):
    """tests/test_gpu_mi.py: P bit for bit (float64), dI and dJ within mi_ref.units <= 1."""
    import mi_ref

    bits(out["P"], ref["P"], "P", fails=fails)
    for k in ("dI", "dJ"):
        if out[k].shape != ref[k].shape:
            fails.append(f"{k}: shape {out[k].shape} vs {ref[k].shape}")
            continue
        u = float(units(out[k], ref[k], c["dtype"]))
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), u)
        if not u <= 1.0:
            fails.append(f"{k}: {u:.3g} x RTOL x max|ref|")


# ------------------------------------------------------------------ warp_labels  (csrc/labels.hip: warp_labels_impl)

SLAB_U = 2   # labels.hip:178


def slab_walk(sp):
    """What launch.hpp:69 slab_grid and common.hpp:191 Slabs make of a 3D volume: None where the plain kernel runs, else
    the set of the slab kernel's gate sides."""
    nx, ny, nz = sp
    nvox = nx * ny * nz
    if not (nz >= 2 and KBLOCK // nz + 1 < ny and nvox >= 4 * SLAB_U * KBLOCK):   # launch.hpp:70
        return None
    per = SLAB_U * KBLOCK
    tags = {"slab"}
    rest = nvox % per
    tags.add("slab_whole" if rest == 0 else "slab_ragged_last")       # common.hpp:203: ok[e] false for some lane
    if 0 < rest <= KBLOCK:
        tags.add("slab_last_wholly_invalid")                           # ... for every lane of the last block's slab 1
    s = np.arange(nvox, dtype=np.int64)
    s = s[(s % per < KBLOCK) & (s + KBLOCK < nvox)]                    # slab 0 of a block whose slab 1 is valid
    r = s % (ny * nz)
    j, k = r // nz, r % nz
    cj = j + KBLOCK // nz + ((k + KBLOCK % nz) >= nz)                  # common.hpp:219-221
    tags.add("carry_j" if bool(((k + KBLOCK % nz) >= nz).any()) else "no_carry_j")
    tags.add("carry_i" if bool((cj >= ny).any()) else "no_carry_i")    # common.hpp:222
    return tags


def _case_warp_labels(rng, c0):
    cap = CAPS["warp_labels"]
    pick = rng.random()
    if pick < 0.3:     # slabs whose 256-voxel step carries nowhere or only in j: nz divides 256, whole planes of 512 or not
        nz = int(rng.choice([2, 8, 16, 32, 64]))
        ny = int(rng.choice([e for e in EXTENTS if e > KBLOCK // nz + 1 and e * nz <= cap // 2]))
        nx = int(rng.choice([e for e in EXTENTS if 4 * SLAB_U * KBLOCK <= e * ny * nz <= cap] or [max(-(-4 * SLAB_U * KBLOCK // (ny * nz)), 1)]))
        sp = (nx, ny, nz)
    elif pick < 0.6:
        sp = _shape(rng, cap, d=3, least=4 * SLAB_U * KBLOCK)
    else:
        sp = _shape(rng, cap)
    N, dtype = int(rng.integers(1, 4)), _dtype(rng)
    c = _new(*c0, sp, dtype, N)
    bc = bool(rng.random() < 0.3)
    K = int(rng.choice([2, 5, 300]))
    NL = 1 if bc else N
    if rng.random() < 0.5:   # connected structures
        L = np.stack([_smooth3(rng.standard_normal((min(K, 6),) + sp), range(1, 1 + len(sp))).argmax(0) for _ in range(NL)])[:, None]
    else:
        L = rng.integers(0, K, (NL, 1) + sp)
    c["inputs"]["L"] = np.ascontiguousarray(L.astype(np.int32))
    c["inputs"]["u"] = _displacement(rng, N, sp, dtype, amps=(0.3, 1.5, 6.0, 40.0, 1e4))
    c["params"].update(dt=float(rng.choice([1.0, -1.0, 0.7, -0.37])), mode=str(rng.choice(["vote", "nearest"])), num_labels=K)
    walk = slab_walk(sp) if len(sp) == 3 else None
    c["tags"] |= {"broadcast" if bc else "per_item", c["params"]["mode"]} | (walk or {"2d" if len(sp) == 2 else "plain_3d"})
    return c


def _valid_warp_labels(c):
    L, u, sp, N = c["inputs"]["L"], c["inputs"]["u"], c["sp"], c["N"]
    # lagomorph_ext.warp_labels; labels.hip:170 check_volume with kPlane29
    return [m for ok, m in ((len(sp) in (2, 3), "dim"), (L.dtype == np.int32 and L.shape[1:] == (1,) + sp and L.shape[0] in (1, N), "L"),
                            (u.shape == (N, len(sp)) + sp and u.dtype == c["dtype"], "u"), (c["params"]["mode"] in ("vote", "nearest"), "mode"),
                            (bool(np.isfinite(u).all()), "finite"), (bool((L >= 0).all() and (L < c["params"]["num_labels"]).all()), "labels in [0, K)"),
                            (np.prod(sp) < 2 ** 29, "extent")) if not ok]


def _ref_warp_labels(c):
    import labels_ref

    return {"out": labels_ref.warp(c["inputs"]["L"], c["inputs"]["u"], c["params"]["dt"], c["params"]["mode"])}


def _judge_warp_labels(c, out, ref, fails, worst):
    """tests/test_gpu_labels.py: label for label."""
    bits(out["out"], ref["out"], "out", fails=fails)


# ------------------------------------------------------------------ label_overlap  (csrc/labels.hip: label_overlap_impl)

LAB_CHUNK, LABELS_MAX = 16384, 4096   # labels.hip:29, include/lagomorph_hip.h LAGO_LABELS_MAX
LABEL_DTYPES = ("uint8", "int16", "int32", "int64")   # lagomorph_ext._LABEL_DTYPES


def _case_label_overlap(rng, c0):
    big = rng.random() < 0.4
    sp = _shape(rng, CAPS["label_overlap"], least=LAB_CHUNK + 1 if big else 0)
    N = int(rng.integers(1, 4))
    c = _new(*c0, sp, np.float32, N)
    K = int(rng.choice([1, 2, 5, 21, 22, 200, 1365, 1366, 2730, 2731, 4096, int(rng.integers(1, LABELS_MAX + 1))]))
    dt = str(rng.choice([t for t in LABEL_DTYPES if K - 1 <= np.iinfo(t).max]))
    hi = K if rng.random() < 0.5 else min(K, 6)   # few labels: every wave's ballot finds many equal pairs
    A = rng.integers(0, hi, (N, 1) + sp)
    B = np.where(rng.random(A.shape) < float(rng.choice([0.0, 0.1, 1.0])), rng.integers(0, hi, A.shape), A)
    c["inputs"].update(A=A.astype(dt), B=B.astype(dt))
    c["params"]["num_labels"] = K
    nvox, K3 = int(np.prod(sp)), 3 * K
    chunks, per = split_row(nvox, chunks_wanted(K3 * 4, N, nvox, LAB_CHUNK), LAB_CHUNK)   # labels.hip:267 plan_tables<uint32_t>
    rep = 4 if 4 * K3 * 4 <= TABLE_LDS_BYTES else (2 if 2 * K3 * 4 <= TABLE_LDS_BYTES else 1)   # labels.hip:269-270
    c["tags"] |= {"one_chunk" if chunks == 1 else "several_chunks", f"rep{rep}",
                  "one_reducer_group" if K3 <= 64 else "several_reducer_groups",          # chunk_table.hpp:150 groups of 64 entries
                  "whole_vectors" if nvox % 4 == 0 else "vector_tail"}                     # chunk_table.hpp:49 walk_split<4>
    return c


def _valid_label_overlap(c):
    A, B, K = c["inputs"]["A"], c["inputs"]["B"], c["params"]["num_labels"]
    # lagomorph_ext.label_count / _check_labels / label_overlap; labels.hip:258-260
    return [m for ok, m in ((1 <= K <= LABELS_MAX, "K"), (A.dtype == B.dtype and A.dtype.name in LABEL_DTYPES, "dtype"),
                            (A.shape == B.shape == (c["N"], 1) + c["sp"] and len(c["sp"]) in (2, 3), "shape"),
                            (bool((A >= 0).all() and (A < K).all() and (B >= 0).all() and (B < K).all()), "labels in [0, K)"),
                            (np.prod(c["sp"]) <= 2 ** 30, "extent")) if not ok]


def _ref_label_overlap(c):
    import labels_ref

    return {"counts": labels_ref.overlap(c["inputs"]["A"], c["inputs"]["B"], c["params"]["num_labels"])}


def _native_label_overlap(c):
    """The definition, label by label (labels_ref.overlap is the bincount route), for tables of up to 200 labels."""
    A, B, K = c["inputs"]["A"].astype(np.int64), c["inputs"]["B"].astype(np.int64), c["params"]["num_labels"]
    if K > 200:
        return None
    out = np.zeros((c["N"], K, 3), dtype=np.int64)
    for k in range(K):
        a, b = (A == k).reshape(c["N"], -1), (B == k).reshape(c["N"], -1)
        out[:, k] = np.stack([a.sum(1), b.sum(1), (a & b).sum(1)], axis=1)
    return {"counts": out}


def _judge_label_overlap(c, out, ref, fails, worst):
    """tests/test_gpu_labels.py: count for count."""
    bits(out["counts"], ref["counts"], "counts", fails=fails)


# ------------------------------------------------------------------ distance_transform  (csrc/edt.hip)

EDT_MAX_EXTENT = 1024
EDT_REL = 8 * 2.0 ** -24   # tests/test_gpu_edt.py REL


def edt_tile(n):
    """edt.hip:102."""
    return 64 if n <= 256 else (32 if n <= 512 else 16)


def _case_distance_transform(rng, c0):
    import edt_ref   # (numpy only: the input kinds)

    cap = CAPS["distance_transform"]
    if rng.random() < 0.45:   # one long line (the 32- and 16-line tiles) on a random axis, the other extents small
        d, n = int(rng.choice([2, 3, 3])), int(rng.choice([257, 300, 512, 513, 1024]))
        rest = _shape(rng, cap // n, d=d - 1)
        at = int(rng.integers(0, d))
        sp = rest[:at] + (n,) + rest[at:]
    else:
        sp = _shape(rng, cap)
    N = int(rng.integers(1, 4))
    c = _new(*c0, sp, np.float32, N)
    kind = str(rng.choice(edt_ref.KINDS))
    c["inputs"]["L"] = np.ascontiguousarray(edt_ref.labels(kind, N, sp, seed=int(rng.integers(0, 2 ** 31))))
    d = len(sp)
    spacing = 1.0
    if rng.random() < 0.6:
        spacing = tuple(float(x) for x in rng.choice([0.5, 0.7, 1.0, 1.5, 2.0, 3.25], size=d))
        if all(s == 1.0 for s in spacing):
            spacing = (0.7,) * d
    c["params"].update(where=str(rng.choice(edt_ref.WHERES)), label=1, spacing=spacing, kind=kind)
    side = lambda n: "le256" if n <= 256 else ("le512" if n <= 512 else "gt512")   # edt.hip:102 edt_tile of each pass
    c["tags"] |= {f"{len(sp)}d", "unit_spacing" if spacing == 1.0 else "anisotropic", "z_" + side(sp[-1]), "y_" + side(sp[-2])}
    if d == 3:
        c["tags"].add("x_" + side(sp[0]))
    return c


def _valid_distance_transform(c):
    import edt_ref

    L, p, d = c["inputs"]["L"], c["params"], len(c["sp"])
    s = (p["spacing"],) * d if np.ndim(p["spacing"]) == 0 else tuple(p["spacing"])
    # lagomorph_ext.distance_transform / edt_spacing / edt_where; edt.hip:128-140
    return [m for ok, m in ((p["where"] in edt_ref.WHERES, "where"), (L.dtype == np.int32 and L.shape == (c["N"], 1) + c["sp"] and d in (2, 3), "L"),
                            (max(c["sp"]) <= EDT_MAX_EXTENT, "extent"), (len(s) == d and all(1e-38 < x < 3e38 for x in s), "spacing"),
                            (-2 ** 31 <= p["label"] < 2 ** 31, "label")) if not ok]


def _ref_distance_transform(c):
    import edt_ref

    p = c["params"]
    sq = edt_ref.as_float(edt_ref.edt_sq(edt_ref.features(c["inputs"]["L"], p["where"], p["label"]), p["spacing"]))
    return {"squared": sq.astype(np.float32), "root": np.sqrt(sq.astype(np.float32)), "_sq64": sq}


def _native_distance_transform(c):
    """The recurrence in float32, every term rounded as the kernels round it: (float32 spacing x delta) squared, added."""
    import edt_ref

    p, d = c["params"], len(c["sp"])
    s = (p["spacing"],) * d if np.ndim(p["spacing"]) == 0 else tuple(p["spacing"])
    f = edt_ref.features(c["inputs"]["L"], p["where"], p["label"])
    g = np.where(f, np.float32(0), np.float32(np.inf)).astype(np.float32)
    for a in range(d - 1, -1, -1):
        i = np.arange(f.shape[2 + a])
        t = np.float32(s[a]) * (i[:, None] - i[None, :]).astype(np.float32)
        cost = (t * t).astype(np.float32)
        gm = np.moveaxis(g, 2 + a, -1)
        out = np.full_like(gm, np.inf)
        for j in range(gm.shape[-1]):
            out = np.minimum(out, gm[..., j:j + 1] + cost[:, j])
        g = np.moveaxis(out, -1, 2 + a)
    return {"squared": g, "root": np.sqrt(g)}


def _judge_distance_transform(c, out, ref, fails, worst):
    """tests/test_gpu_edt.py: unit spacing bit for bit (squared and root); otherwise the squared distance has the
    reference's infinities, no NaN, exact zeros and a relative error of at most REL = 8 x 2^-24, and the root is the
    float32 square root of the squared output bit for bit."""
    got, root = np.asarray(out["squared"]), np.asarray(out["root"])
    if got.dtype != np.float32 or root.dtype != np.float32 or got.shape != ref["squared"].shape or root.shape != got.shape:
        fails.append(f"squared / root: {got.shape} {got.dtype}, {root.shape} {root.dtype} vs float32 {ref['squared'].shape}")
        return
    if "unit_spacing" in c["tags"]:
        bits(got, ref["squared"], "squared", fails=fails)
        bits(root.view(np.int32), ref["root"].view(np.int32), "root", fails=fails)
        return
    want = ref["_sq64"]
    g64 = got.astype(np.float64)
    if not np.array_equal(np.isinf(g64), np.isinf(want)) or np.isnan(g64).any():
        fails.append("squared: infinities differ from the reference's, or a NaN")
        return
    fin = np.isfinite(want) & (want > 0)
    if not np.all(g64[want == 0] == 0):
        fails.append("squared: not exactly 0 on a feature voxel")
    err = np.abs(g64[fin] - want[fin]) / want[fin]
    w = float(err.max()) / EDT_REL if err.size else 0.0
    if worst is not None:
        worst["squared"] = max(worst.get("squared", 0.0), w)
    if not w <= 1.0:
        fails.append(f"squared: relative error {w * 8:.3g} x 2^-24 over the bound of 8")
    if not np.array_equal(root.view(np.uint32), np.sqrt(got).view(np.uint32)):
        fails.append("root: not the float32 square root of the squared output")


# ------------------------------------------------------------------ interp_points  (csrc/points.hip)

def _case_interp_points(rng, c0):
    sp = _shape(rng, CAPS["interp_points"])
    N, C, dtype = int(rng.integers(1, 4)), int(rng.integers(1, 4)), _dtype(rng)
    c = _new(*c0, sp, dtype, N)
    bc = bool(rng.random() < 0.3)
    # (a choice of this generator, not a limit of the entry point: at least four points.  The rule's scale is
    # max|reference| over the values of ONE call; a call with a single point whose value nearly cancels -- 6.5e-5 from
    # corners of order 1 -- leaves float32 arithmetic no way to meet it.  The family's own test has P = 1 at fixed seeds)
    P = int(rng.choice([4, 63, 64, 65, 128, 255, 256, 257, 640, 1000, 4096 + 17, 64 * int(rng.integers(1, 40)), int(rng.integers(4, 3000))]))
    d = len(sp)
    kind = str(rng.choice(["scattered", "scattered", "crowd", "grid"]))
    x = np.empty((N, d, P))
    for a, n in enumerate(sp):
        if kind == "crowd":      # every point inside one cell (points_ref.crowd)
            x[:, a] = max((n - 2) // 2, 0) + rng.uniform(0.0, 1.0, (N, P))
        else:                    # half inside, half up to 2.5 voxels outside (points_ref.scattered)
            x[:, a, :P // 2] = rng.uniform(0.0, n - 1.0, (N, P // 2))
            x[:, a, P // 2:] = rng.uniform(-2.5, n + 1.5, (N, P - P // 2))
    if kind == "grid":           # on grid points: t = 0 on every axis
        x = np.round(x)
    if rng.random() < 0.15:      # far outside: the clamped border
        x[:, int(rng.integers(0, d)), ::3] = float(rng.choice([-1e6 - 0.25, 1e6 + 0.25]))
    c["inputs"].update(F=rng.standard_normal(((1 if bc else N), C) + sp).astype(dtype), x=np.ascontiguousarray(x.astype(dtype)),
                       go=rng.standard_normal((N, C, P)).astype(dtype))
    c["params"]["kind"] = kind
    c["tags"] |= {f"{d}d", "broadcast" if bc else "per_item",
                  "one_workgroup" if P <= KBLOCK else "several_workgroups",      # points.hip:152 grid of ceil(P / kBlock)
                  "whole_waves" if P % 64 == 0 else "ragged_wave"}
    if kind == "crowd":
        c["tags"].add("crowd")
    if kind == "grid":
        c["tags"].add("on_grid_points")
    if sp[-1] == 1:
        c["tags"].add("thin_z")
    return c


def _valid_interp_points(c):
    F, x, go, sp = c["inputs"]["F"], c["inputs"]["x"], c["inputs"]["go"], c["sp"]
    # lagomorph_ext._check_points; points.hip:130 points_geom
    return [m for ok, m in ((len(sp) in (2, 3) and F.shape[2:] == sp and F.shape[0] in (1, c["N"]), "F"),
                            (x.shape[:2] == (c["N"], len(sp)) and x.ndim == 3, "x"), (go.shape == (c["N"], F.shape[1], x.shape[2]), "go"),
                            (F.dtype == x.dtype == go.dtype == c["dtype"], "dtype"), (bool(np.isfinite(x).all() and (np.abs(x) < 2 ** 30).all()), "domain"),
                            (c["N"] <= 65535 and x.shape[2] < 2 ** 31, "grid")) if not ok]


def _ref_interp_points(c):
    import points_ref

    F, x, go = c["inputs"]["F"], c["inputs"]["x"], c["inputs"]["go"]
    val, grad = points_ref.sample(F, x)
    return {"out": val, "d_x": (go[:, :, None, :].astype(np.float64) * grad).sum(1), "_wide": points_ref.scatter_wide(go, x, c["sp"], F.shape[0])}


def _native_interp_points(c):
    """The values and d_x rounded to the case's dtype; d_F as the sequential sum in the case's dtype (np.add.at), corner
    by corner -- one of the orders the atomics may take."""
    import itertools

    import points_ref

    ref = reference(c)
    F, x, go = c["inputs"]["F"], c["inputs"]["x"], c["inputs"]["go"]
    R = c["dtype"].type
    sp, N, C, P = c["sp"], c["N"], F.shape[1], x.shape[2]
    tp = points_ref._taps(x, sp)
    dF = np.zeros((F.shape[0], C, int(np.prod(sp))), dtype=R)
    item = np.broadcast_to((np.arange(N) if F.shape[0] == N else np.zeros(N, dtype=np.int64)).reshape(N, 1, 1), (N, C, P))
    chan = np.broadcast_to(np.arange(C).reshape(1, C, 1), (N, C, P))
    for bits in itertools.product((0, 1), repeat=len(sp)):
        fac = [tp[a][2] if b else R(1) - tp[a][2] for a, b in enumerate(bits)]
        w = (fac[0] * fac[1]) * fac[2] if len(sp) == 3 else fac[0] * fac[1]
        lin = np.zeros((N, P), dtype=np.int64)
        for a, b in enumerate(bits):
            lin = lin * sp[a] + (tp[a][1] if b else tp[a][0])
        np.add.at(dF, (item, chan, np.broadcast_to(lin[:, None, :], (N, C, P))), (w[:, None, :] * go).astype(R))
    return {"out": ref["out"].astype(R), "d_x": ref["d_x"].astype(R), "d_F": dF.reshape(F.shape)}


def _judge_interp_points(c, out, ref, fails, worst):
    """tests/test_gpu_points.py: values and d_x within RTOL x max|reference|; d_F cell by cell within
    scatter_bound.cell_bound of points_ref.scatter_wide, cells that receive nothing exactly 0."""
    import scatter_bound

    close(out["out"], ref["out"], c["dtype"], "out", fails=fails, worst=worst)
    close(out["d_x"], ref["d_x"], c["dtype"], "d_x", fails=fails, worst=worst)
    got = np.asarray(out["d_F"])
    if got.shape != ref["_wide"][0].shape:
        fails.append(f"d_F: shape {got.shape} vs {ref['_wide'][0].shape}")
        return
    bad = scatter_bound.violations(got, ref["_wide"], c["dtype"])
    if worst is not None:
        worst["d_F"] = max(worst.get("d_F", 0.0), scatter_bound.worst_ratio(got, ref["_wide"], c["dtype"]))
    if bad.any():
        fails.append(f"d_F: {int(bad.sum())} of {bad.size} cells over their bound, first at {tuple(int(i) for i in np.argwhere(bad)[0])}")


# ------------------------------------------------------------------ gaussian_smooth  (csrc/gauss.hip, gauss.hpp)

GAUSS_MAX_RADIUS, GAUSS_SEGMENT = 32, 1024   # include/lagomorph_hip.h LAGO_GAUSS_MAX_RADIUS; gauss.hpp:72 ZS
GAUSS_WORK = 8e7                             # voxels x taps of a case's reference: about 0.2 s (profiles/fuzz_ops.md)


def gauss_tile_max(dtype):
    """gauss.hpp:86 tmax: positions of a strided axis one workgroup stages."""
    return 64 if np.dtype(dtype) == np.float32 else 32


def _case_gaussian_smooth(rng, c0):
    import gauss_ref   # (numpy only)

    dtype = _dtype(rng)
    pick = rng.random()
    N, C = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    if pick < 0.08:      # three passes, none of which stages whole lines: nz > 1024 and nx, ny > 32 in float64 (gauss.hip:170-176)
        dtype, sp, N, C = np.dtype(np.float64), (33, 33, int(rng.choice([1025, 1028, 1030]))), 1, 1
    elif pick < 0.16:    # rows of several segments
        sp = tuple(int(x) for x in rng.choice([1, 2, 3, 5], size=int(rng.choice([1, 2])))) + (int(rng.choice([1030, 2051, 1100])),)
    else:
        sp = _shape(rng, 120_000)
    d = len(sp)
    c = _new(*c0, sp, dtype, N)
    truncate = float(rng.choice([4.0, 4.0, 3.0, 2.0]))
    kind = rng.random()
    if pick < 0.08:
        sigma = [float(s) for s in rng.choice([0.4, 0.5, 0.7], size=3)]
    elif kind < 0.35:
        sigma = [float(rng.choice([0.4, 0.5, 1.0, 2.5, 5.0, 8.0]))] * d
    else:                # per axis, zeros among them
        sigma = [float(s) for s in rng.choice([0.0, 0.0, 0.1, 0.5, 1.3, 2.5, 8.0], size=d)]
    radii = [min(gauss_ref.radius(s, truncate), GAUSS_MAX_RADIUS) for s in sigma]
    while N * C * int(np.prod(sp)) * sum(2 * r + 1 for r in radii if r) > GAUSS_WORK and (N > 1 or C > 1):
        N, C = max(N - 1, 1), max(C - 1, 1)
    while N * C * int(np.prod(sp)) * sum(2 * r + 1 for r in radii if r) > GAUSS_WORK:
        sigma = [s / 2 for s in sigma]
        radii = [gauss_ref.radius(s, truncate) for s in sigma]
    while any(gauss_ref.radius(s, truncate) > GAUSS_MAX_RADIUS for s in sigma):   # (8.0 x 4 + 0.5 is 32: the cap itself)
        sigma = [s * 0.97 for s in sigma]
    radii = [gauss_ref.radius(s, truncate) for s in sigma]
    c["N"] = N
    x = rng.standard_normal((N, C) + sp).astype(dtype)
    mode = str(rng.choice(["wrap", "zero"]))
    form = str(rng.choice(["new", "out", "accumulate"]))
    c["inputs"]["x"] = x
    if form != "new":
        c["inputs"]["out0"] = rng.standard_normal(x.shape).astype(dtype)
    c["params"].update(sigma=sigma, truncate=truncate, radii=radii, mode=mode, form=form,
                       alpha=float(rng.choice([1.0, 1.0, -0.5, 2.25])))
    filtered = [a for a in range(d) if radii[a] > 0]
    ax3 = [a + 3 - d for a in filtered]          # as the kernels number the axes: z is 2, y is 1, x is 0
    tmax = gauss_tile_max(dtype)
    c["tags"] |= {f"axes_{len(filtered)}", mode, form, "row_gt128" if sp[-1] > 128 else "row_le128"}
    if len(filtered) == 3:   # gauss.hip:128 gauss_whole_lines: nseg == 1 (gauss.hpp:72-73) or nat == 1 (gauss.hpp:86-89)
        whole = sp[2] <= GAUSS_SEGMENT or sp[0] <= tmax or sp[1] <= tmax
        c["tags"].add("three_whole_line" if whole else "three_no_whole_line")
    if 2 in ax3 and sp[-1] > GAUSS_SEGMENT:
        c["tags"].add("z_segments")
    strided = [sp[a] for a in filtered if a != d - 1]
    if strided:
        c["tags"].add("strided_several_tiles" if max(strided) > tmax else "strided_one_tile")
    if mode == "wrap" and any(radii[a] > sp[a] for a in filtered):
        c["tags"].add("radius_above_extent")
    return c


def _valid_gaussian_smooth(c):
    import gauss_ref

    x, p, d = c["inputs"]["x"], c["params"], len(c["sp"])
    # smooth._plan, lagomorph_ext.gaussian_smooth_forward / _gauss_half_taps
    return [m for ok, m in ((d in (2, 3) and x.ndim == d + 2 and x.dtype == c["dtype"], "x"), (p["mode"] in ("wrap", "zero"), "mode"),
                            (len(p["radii"]) == d and all(0 <= r <= GAUSS_MAX_RADIUS for r in p["radii"]), "radius"),
                            (p["radii"] == [gauss_ref.radius(s, p["truncate"]) for s in p["sigma"]], "radii of sigma"),
                            (p["form"] == "new" or c["inputs"]["out0"].shape == x.shape and c["inputs"]["out0"].dtype == x.dtype, "out"),
                            (np.prod(c["sp"]) < 2 ** 29, "extent")) if not ok]


def _gauss_total(c, taps):
    import gauss_ref

    p = c["params"]
    y = p["alpha"] * gauss_ref.smooth_taps(c["inputs"]["x"], taps, p["mode"])
    return {"out": y + c["inputs"]["out0"].astype(np.float64) if p["form"] == "accumulate" else y}


def _ref_gaussian_smooth(c):
    import gauss_ref

    return _gauss_total(c, [gauss_ref.taps(s, c["params"]["truncate"]) for s in c["params"]["sigma"]])


def _native_gaussian_smooth(c):
    """The same sums with the taps as the device holds them (gauss_ref.rounded_taps), the result rounded to the dtype."""
    import gauss_ref

    out = _gauss_total(c, [gauss_ref.rounded_taps(s, c["params"]["truncate"], c["dtype"]) for s in c["params"]["sigma"]])
    return {"out": out["out"].astype(c["dtype"])}


def _judge_gaussian_smooth(c, out, ref, fails, worst):
    """tests/test_gpu_gauss.py: gauss_ref.units <= 1 (units_of there), for alpha G x and for out + alpha G x alike."""
    import gauss_ref

    if out["out"].shape != ref["out"].shape or out["out"].dtype != c["dtype"]:
        fails.append(f"out: {out['out'].shape} {out['out'].dtype} vs {ref['out'].shape} {c['dtype']}")
        return
    u = float(units(out["out"], ref["out"], c["dtype"]))
    if worst is not None:
        worst["out"] = max(worst.get("out", 0.0), u)
    if not u <= 1.0:
        fails.append(f"out: {u:.3g} x RTOL x max|ref|")


# ------------------------------------------------------------------ invert_displacement  (csrc/invert.hip)

def _case_invert_displacement(rng, c0):
    import invert_ref   # (its `field` is numpy only; importing the module loads the CPU oracle)

    sp = _shape(rng, CAPS["invert_displacement"], low=2)   # (the Lipschitz field needs a difference along every axis)
    N, dtype = int(rng.integers(1, 4)), _dtype(rng)
    c = _new(*c0, sp, dtype, N)
    d = len(sp)
    c["inputs"]["u"] = invert_ref.field(sp, N, dtype)                                  # contraction bound 0.5
    c["inputs"]["go"] = rng.standard_normal((N, d) + sp).astype(dtype)
    c["inputs"]["rough"] = _displacement(rng, N, sp, dtype, amps=(0.3, 3.0))          # far outside the contraction regime
    c["params"].update(iters=int(rng.choice([1, 60])), rough_iters=int(rng.choice([0, 1, 2, 5, 9])))
    nvox = int(np.prod(sp))
    c["tags"] |= {f"{d}d", "one_step" if c["params"]["iters"] == 1 else "fixed_point", "no_step" if c["params"]["rough_iters"] == 0 else "steps",
                  "one_block" if nvox <= KBLOCK else "several_blocks"}             # common.hpp:116 make_geom
    return c


def _valid_invert_displacement(c):
    import invert_ref

    u, d = c["inputs"]["u"], len(c["sp"])
    # lagomorph_ext._check_invert / invert_displacement_forward / invert_displacement_adjoint
    return [m for ok, m in ((d in (2, 3) and all(v.shape == (c["N"], d) + c["sp"] and v.dtype == c["dtype"] for v in c["inputs"].values()), "fields"),
                            (c["params"]["iters"] >= 0 and c["params"]["rough_iters"] >= 0, "iters"),
                            (invert_ref.lipschitz_bound(u) <= 0.5 + 1e-9, "Lipschitz bound"), (np.prod(c["sp"]) < 2 ** 29, "extent")) if not ok]


def _ref_invert_displacement(c):
    import invert_ref

    u, go = c["inputs"]["u"], c["inputs"]["go"]
    v60 = invert_ref.forward(u, 60)
    v = v60 if c["params"]["iters"] == 60 else invert_ref.forward(u, c["params"]["iters"])
    # "_v60" is the adjoint's third argument on the GPU too, as in tests/test_gpu_invert.py test_adjoint
    rough = invert_ref.forward(c["inputs"]["rough"], c["params"]["rough_iters"])
    return {"v": v, "lam": invert_ref.lam(go, u, v60), "rough": rough, "rough_loop": rough, "_v60": v60}


def _native_invert_displacement(c):
    """invert_ref.np_forward, the pure-numpy iteration in the case's dtype (one step; sixty of them on small volumes)."""
    import invert_ref

    if c["params"]["iters"] > 1 and int(np.prod(c["sp"])) * c["N"] > 20_000:
        return None
    ref = reference(c)
    v = invert_ref.np_forward(c["inputs"]["u"], c["params"]["iters"])
    rough = invert_ref.np_forward(c["inputs"]["rough"], c["params"]["rough_iters"])
    return {"v": v, "lam": ref["lam"].astype(c["dtype"]), "rough": rough, "rough_loop": rough}


def _judge_invert_displacement(c, out, ref, fails, worst):
    """tests/test_gpu_invert.py: one step within RTOL x max|reference|, sixty within 2 RTOL x max|reference| (the
    contraction bound 0.5); lam within RTOL x max|reference|; the fused steps on a rough field have the bits of the
    unfused loop over interp_forward (both come from the device: "rough" and "rough_loop")."""
    allowed = 1.0 if c["params"]["iters"] <= 1 else 2.0
    w = {}
    close(out["v"], ref["v"], c["dtype"], "v", fails=[], worst=w)
    if "v" not in w or not w["v"] <= allowed:
        fails.append(f"v: {w.get('v')} x RTOL x max|ref| (allowed {allowed:g})")
    if worst is not None and "v" in w:
        worst["v"] = max(worst.get("v", 0.0), w["v"] / allowed)
    close(out["lam"], ref["lam"], c["dtype"], "lam", fails=fails, worst=worst)
    bits(out["rough"], out["rough_loop"], "rough", fails=fails)


# ------------------------------------------------------------------ ffd_expand and its adjoint  (csrc/ffd.hip)

FFD_MAX_SPACING = 32   # lagomorph_ext.FFD_MAX_SPACING


def ffd_tiles(d):
    """ffd.hip:46-48: voxels of a tile per spatial axis, 8 x 8 x 64 in 3D and 64 x 64 in 2D."""
    return (8, 8, 64) if d == 3 else (64, 64)


def _case_ffd_expand(rng, c0):
    N, C, dtype = int(rng.integers(1, 4)), int(rng.integers(1, 4)), _dtype(rng)
    # (float64 results are held against sums in long double, for which numpy has no fast product: a quarter of the cap)
    sp = _shape(rng, CAPS["ffd_expand"] // (4 if dtype == np.float64 else 1))
    c = _new(*c0, sp, dtype, N)
    d = len(sp)
    kind = rng.random()
    if kind < 0.25:
        spacing = tuple([int(rng.integers(1, FFD_MAX_SPACING + 1))] * d)
    else:
        spacing = tuple(int(s) for s in rng.choice([1, 1, 2, 3, 4, 5, 7, 8, 16, 31, 32], size=d))
    m = tuple((n - 1) // s + 4 for n, s in zip(sp, spacing))
    c["inputs"].update(ctrl=rng.standard_normal((N, C) + m).astype(dtype), g=rng.standard_normal((N, C) + sp).astype(dtype))
    c["params"]["spacing"] = spacing
    for name, n, t, s in zip("xyz"[3 - d:], sp, ffd_tiles(d), spacing):
        c["tags"] |= {f"{name}_one_tile" if n <= t else f"{name}_several_tiles", f"{name}_whole_tiles" if n % t == 0 else f"{name}_ragged_tile"}
        if s == 1:
            c["tags"].add("spacing_1")
        if s >= n:
            c["tags"].add("one_cell")
        if (n - 1) % s == 0:
            c["tags"].add("last_plane_unused")
    c["tags"].add(f"{d}d")
    return c


def _valid_ffd_expand(c):
    ctrl, g, s, sp = c["inputs"]["ctrl"], c["inputs"]["g"], c["params"]["spacing"], c["sp"]
    # lagomorph_ext.ffd_spacing / ffd_grid_shape / _check_ffd
    return [m for ok, m in ((len(sp) in (2, 3) and min(sp) >= 1, "shape"), (len(s) == len(sp) and all(isinstance(v, int) and 1 <= v <= FFD_MAX_SPACING for v in s), "spacing"),
                            (ctrl.shape[2:] == tuple((n - 1) // v + 4 for n, v in zip(sp, s)) and ctrl.shape[:2] == g.shape[:2], "control grid"),
                            (g.shape[2:] == sp and ctrl.dtype == g.dtype == c["dtype"], "g")) if not ok]


def _ref_ffd_expand(c):
    import ffd_ref

    ctrl, g, s, sp, dtype = c["inputs"]["ctrl"], c["inputs"]["g"], c["params"]["spacing"], c["sp"], c["dtype"]
    work = np.longdouble if dtype == np.float64 else np.float64   # (tests/test_gpu_ffd.py _forward_case)
    return {"forward": ffd_ref.expand(ctrl, sp, s, work=work), "adjoint": ffd_ref.adjoint(g, s),
            "_vbound": ffd_ref.voxel_bound(ctrl, sp, s, dtype), "_ebound": ffd_ref.entry_bound(g, s, dtype)}


def _native_ffd_expand(c):
    import ffd_ref

    return {"forward": ffd_ref.expand_native(c["inputs"]["ctrl"], c["sp"], c["params"]["spacing"]),
            "adjoint": ffd_ref.adjoint_native(c["inputs"]["g"], c["params"]["spacing"])}


def _judge_ffd_expand(c, out, ref, fails, worst):
    """tests/test_gpu_ffd.py.  Forward: every voxel within ffd_ref.voxel_bound AND max error within RTOL x max|ref|.
    Adjoint: float64 within 1e-12 max|ref|, float32 every control point within ffd_ref.entry_bound; control planes that
    no voxel reaches exactly 0."""
    import ffd_ref

    for k in ("forward", "adjoint"):
        if out[k].shape != ref[k].shape or out[k].dtype != c["dtype"]:
            fails.append(f"{k}: {out[k].shape} {out[k].dtype} vs {ref[k].shape} {c['dtype']}")
            return
    want = ref["forward"]
    err = np.abs(out["forward"].astype(want.dtype) - want).astype(np.float64)
    ratio = ffd_ref.worst_ratio(err, ref["_vbound"])
    rel = float(err.max()) / (RTOL[c["dtype"]] * float(np.abs(want).max())) if err.size else 0.0
    h = out["adjoint"].astype(np.float64)
    erra = np.abs(h - ref["adjoint"])
    if c["dtype"] == np.float64:
        ra, what = float(erra.max()) / (1e-12 * float(np.abs(ref["adjoint"]).max())), "1e-12 x max|ref|"
    else:
        ra, what = ffd_ref.worst_ratio(erra, ref["_ebound"]), "the entry bound"
    if worst is not None:
        for k, v in (("forward voxel bound", ratio), ("forward", rel), ("adjoint", ra)):
            worst[k] = max(worst.get(k, 0.0), v)
    if not ratio <= 1.0:
        fails.append(f"forward: {ratio:.3g} of the voxel bound")
    if not rel <= 1.0:
        fails.append(f"forward: {rel:.3g} x RTOL x max|ref|")
    if not ra <= 1.0:
        fails.append(f"adjoint: {ra:.3g} of {what}")
    for a, (n, s) in enumerate(zip(c["sp"], c["params"]["spacing"])):
        if (n - 1) % s == 0 and not (np.take(h, h.shape[2 + a] - 1, axis=2 + a) == 0).all():
            fails.append(f"adjoint: the unused last control plane of axis {a} is not exactly 0")


# ------------------------------------------------------------------ field_energy / energy_operator  (csrc/energy.hip)

UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def _case_energy(rng, c0):
    sp = _shape(rng, CAPS["energy"])
    N, C, dtype = int(rng.integers(1, 4)), int(rng.integers(1, 4)), _dtype(rng)
    c = _new(*c0, sp, dtype, N)
    d = len(sp)
    u = rng.standard_normal((N, C) + sp)
    if rng.random() < 0.25:   # affine in the voxel index plus small noise: A u is small against u (energy_ref.field)
        x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sp], indexing="ij")
        coef = rng.uniform(-1.0, 1.0, (N, C, d + 1))
        u = 1e-3 * u + coef[..., -1].reshape((N, C) + (1,) * d) + sum(coef[..., a].reshape((N, C) + (1,) * d) * x[a] for a in range(d))
        c["tags"].add("affine")
    c["inputs"]["u"] = np.ascontiguousarray(u.astype(dtype))
    unit = bool(rng.random() < 0.4)
    spacing = (1.0,) * d if unit else tuple(float(h) for h in rng.choice([0.5, 0.7, 1.0, 1.5, 2.0], size=d))
    scaled = bool(rng.random() < 0.5) and "affine" not in c["tags"]   # (the family's test has no scaled affine case: no rule for one)
    if scaled:
        c["inputs"]["scale"] = rng.choice([-1.75, 0.3, 1.0, 2.5, 0.0], size=N).astype(dtype)
    c["params"].update(kind=str(rng.choice(["diffusion", "bending"])), spacing=spacing)
    for name, n, t in zip("xyz"[3 - d:], sp, ffd_tiles(d)):   # energy.hip EnergyTile: 8 x 8 x 64, 2D 64 x 64 (energy_ref.TILE3 / TILE2)
        c["tags"] |= {f"{name}_one_tile" if n <= t else f"{name}_several_tiles", f"{name}_whole_tiles" if n % t == 0 else f"{name}_ragged_tile"}
    c["tags"] |= {f"{d}d", c["params"]["kind"], "unit_spacing" if all(h == 1.0 for h in spacing) else "anisotropic", "scale" if scaled else "no_scale"}
    if min(sp) <= 2:
        c["tags"].add("thin_axis")
    return c


def _valid_energy(c):
    u, p = c["inputs"]["u"], c["params"]
    s = c["inputs"].get("scale")
    return [m for ok, m in ((len(c["sp"]) in (2, 3) and u.shape[2:] == c["sp"] and u.dtype == c["dtype"], "u"), (p["kind"] in ("diffusion", "bending"), "kind"),
                            (len(p["spacing"]) == len(c["sp"]) and all(h > 0 and np.isfinite(h) for h in p["spacing"]), "spacing"),
                            (s is None or s.shape == (c["N"],) and s.dtype == c["dtype"], "scale")) if not ok]


def _ref_energy(c):
    import energy_ref

    u, p, s = c["inputs"]["u"], c["params"], c["inputs"].get("scale")
    A = energy_ref.operator(u, p["kind"], p["spacing"])
    out = {"E": energy_ref.energy(u, p["kind"], p["spacing"]), "_A": A, "_bound": energy_ref.operator_bound(u, p["kind"], p["spacing"], s)}
    out["A"] = A if s is None else A * s.astype(np.float64).reshape((-1,) + (1,) * (A.ndim - 1))
    return out


def _native_energy(c):
    """energy_ref.operator_native times the scale in the case's dtype, and density_native summed in float64."""
    import energy_ref

    u, p, s = c["inputs"]["u"], c["params"], c["inputs"].get("scale")
    A = energy_ref.operator_native(u, p["kind"], p["spacing"])
    if s is not None:
        A = (A * s.reshape((-1,) + (1,) * (A.ndim - 1))).astype(c["dtype"])
    dens = energy_ref.density_native(u, p["kind"], p["spacing"]).astype(np.float64)
    return {"E": (dens.sum(tuple(range(1, dens.ndim))) / float(np.prod(c["sp"]))).astype(c["dtype"]), "A": A}


def _judge_energy(c, out, ref, fails, worst):
    """tests/test_gpu_energy.py test_energy_and_operator.  float64: E within 1e-12 max|E_ref|, A u within 1e-12
    max|A_ref| (x max|scale|).  float32: every voxel of (scale x) A u within K 2^-24 |scale_n| abs_operator(u)
    (energy_ref.operator_bound), without a scale also max error <= 1e-5 max|A_ref|; E within 1e-5 E_ref per item.
    The affine-plus-noise fields are held to the per-voxel bound K u abs_operator(u) alone, in both precisions, as there:
    their A u and their bending energy are what is left of a cancellation, which no fraction of max|ref| describes."""
    import energy_ref

    if out["A"].shape != ref["A"].shape or out["E"].shape != ref["E"].shape or out["A"].dtype != c["dtype"] or out["E"].dtype != c["dtype"]:
        fails.append(f"E / A: {out['E'].shape} {out['E'].dtype}, {out['A'].shape} {out['A'].dtype}")
        return
    s = c["inputs"].get("scale")
    err_E = np.abs(out["E"].astype(np.float64) - ref["E"])
    err_A = np.abs(out["A"].astype(np.float64) - ref["A"])
    f = {}
    if "affine" in c["tags"]:   # "affine plus small noise: the per-voxel bound alone", K u abs_operator(u) in either precision
        f["A voxel bound (affine)"] = float(energy_ref.worst_ratio(err_A, ref["_bound"] * (UNIT[c["dtype"]] / energy_ref.U32)))
    elif c["dtype"] == np.float64:
        top = float(np.abs(ref["_A"]).max()) * (float(np.abs(s).max()) if s is not None else 1.0)
        f["E"] = float(err_E.max()) / (1e-12 * float(np.abs(ref["E"]).max())) if err_E.max() > 0 else 0.0
        f["A"] = float(err_A.max()) / (1e-12 * top) if err_A.max() > 0 else 0.0
    else:
        f["A voxel bound"] = float(energy_ref.worst_ratio(err_A, ref["_bound"]))
        if s is None:
            f["A"] = float(err_A.max()) / (1e-5 * float(np.abs(ref["A"]).max())) if err_A.max() > 0 else 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            f["E"] = float(np.where(err_E == 0, 0.0, err_E / (1e-5 * ref["E"])).max())
    for k, v in f.items():
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), v)
        if not v <= 1.0:
            fails.append(f"{k}: {v:.3g} of its bound")


# ------------------------------------------------------------------ surface_distance  (lagomorph_amd/distance.py over csrc/edt.hip)

def _case_surface_distance(rng, c0):
    cap = CAPS["surface_distance"]
    if rng.random() < 0.3:   # one line above the 64-line tile of edt.hip:102
        d, n = int(rng.choice([2, 3])), int(rng.choice([257, 300, 513]))
        rest = _shape(rng, cap // n, d=d - 1, low=2)
        at = int(rng.integers(0, d))
        sp = rest[:at] + (n,) + rest[at:]
    else:
        sp = _shape(rng, cap, low=2)
    N = int(rng.integers(1, 4))
    c = _new(*c0, sp, np.float32, N)
    d = len(sp)
    blob = lambda: np.stack([_smooth3(_smooth3(rng.standard_normal((4,) + sp), range(1, 1 + d)), range(1, 1 + d)).argmax(0)
                             for _ in range(N)])[:, None].astype(np.int32)
    A, B = blob(), blob()
    labels = [int(k) for k in rng.permutation([1, 2, 3])[:int(rng.integers(1, 4))]]
    if rng.random() < 0.4:   # a label absent from B: nan
        B = np.where(B == labels[0], 0, B).astype(np.int32)
    if len(labels) > 1 and rng.random() < 0.4:   # the same structure in both: 0
        k = labels[-1]
        B = np.where(A == k, k, np.where(B == k, 0, B)).astype(np.int32)
    unit = bool(rng.random() < 0.4)
    spacing = 1.0 if unit else tuple(float(x) for x in rng.choice([0.5, 0.7, 1.5, 2.0], size=d))
    c["inputs"].update(A=A, B=B)
    c["params"].update(labels=labels, spacing=spacing)
    c["tags"] |= {f"{d}d", "unit_spacing" if unit else "anisotropic", "line_gt256" if max(sp) > 256 else "lines_le256",
                  "one_label" if len(labels) == 1 else "several_labels"}
    for n in range(N):
        for k in labels:
            a, b = A[n] == k, B[n] == k
            if not a.any() or not b.any():
                c["tags"].add("empty_surface")
            elif np.array_equal(a, b):
                c["tags"].add("same_structure")
    return c


def _valid_surface_distance(c):
    A, B, p = c["inputs"]["A"], c["inputs"]["B"], c["params"]
    s = p["spacing"]
    return [m for ok, m in ((A.shape == B.shape == (c["N"], 1) + c["sp"] and A.dtype == B.dtype == np.int32, "label maps"),
                            (max(c["sp"]) <= EDT_MAX_EXTENT and len(c["sp"]) in (2, 3), "extent"),
                            (np.ndim(s) == 0 and s > 0 or len(s) == len(c["sp"]) and all(1e-38 < x < 3e38 for x in s), "spacing"),
                            (len(p["labels"]) >= 1 and all(-2 ** 31 <= k < 2 ** 31 for k in p["labels"]), "labels")) if not ok]


def _ref_surface_distance(c):
    import edt_ref

    return edt_ref.surface_distance(c["inputs"]["A"], c["inputs"]["B"], c["params"]["labels"], c["params"]["spacing"])


def _native_surface_distance(c):
    """The same statistics from plain float64 roots (the reference's default forms the float32 roots the library forms)."""
    import edt_ref

    return edt_ref.surface_distance(c["inputs"]["A"], c["inputs"]["B"], c["params"]["labels"], c["params"]["spacing"], float32_distances=False)


def _judge_surface_distance(c, out, ref, fails, worst):
    """tests/test_gpu_edt.py _check_surface: float64 (N, K), nan exactly where the reference has it, else within 1e-6 |ref|."""
    for k, w in ref.items():
        g = np.asarray(out[k])
        if g.dtype != np.float64 or g.shape != w.shape:
            fails.append(f"{k}: {g.shape} {g.dtype} vs float64 {w.shape}")
            continue
        if not np.array_equal(np.isnan(g), np.isnan(w)):
            fails.append(f"{k}: nan where the reference has none, or the reverse")
            continue
        ok = ~np.isnan(w)
        err = np.abs(g[ok] - w[ok])
        with np.errstate(divide="ignore", invalid="ignore"):
            u = float(np.where(err == 0, 0.0, err / (1e-6 * np.abs(w[ok]))).max()) if err.size else 0.0
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), u)
        if not u <= 1.0:
            fails.append(f"{k}: {u:.3g} x 1e-6 |ref|")


# ------------------------------------------------------------------ lncc  (csrc/lncc.hip)

def _case_lncc(rng, c0):
    import lncc_ref   # (numpy only)

    # the family's own condition on its inputs (tests/test_lncc_host.py): the emulation of the case's precision stays within
    # half the tolerance.  A draw with a near-degenerate window (sI sJ close to sX^2: the smallest grids with the "affine"
    # offset have one in most draws) is replaced by the next draw of the same stream, shape and parameters included
    for draw in range(64):
        sp = _shape(rng, CAPS["lncc"], low=2)
        N, C, dtype = int(rng.integers(1, 4)), int(rng.integers(1, 4)), _dtype(rng)
        d = len(sp)
        kind = str(rng.choice(lncc_ref.KINDS))
        # lncc_ref.sigmas_of: 0.5 goes with the zero-mean kinds only; the per-axis sets hold a zero in 3D
        sig = [1.0, 2.5, 8.0] + ([0.5] if kind != "affine" else []) + [lncc_ref.per_axis_set(d), tuple(reversed(lncc_ref.per_axis_set(d)))]
        sigma = sig[int(rng.integers(0, len(sig)))]
        mode = str(rng.choice(lncc_ref.MODES))
        I, Nz, g = (rng.standard_normal((N, C) + sp).astype(np.float32) for _ in range(3))
        if kind == "corr":
            J = np.float32(0.8) * I + np.float32(0.6) * Nz
        elif kind == "affine":
            J = np.float32(-2.5) * I + np.float32(3.0) + np.float32(0.3) * Nz
        else:
            J = Nz
        J = J.astype(np.float32)
        ref = lncc_ref.lncc_with_grads(I, J, g, sigma, mode=mode)
        emu = lncc_ref.emulate(dtype.type)(I, J, g, sigma, mode=mode)
        if max(units(a, b, dtype) for a, b in zip(emu, ref)) <= 0.5:
            break
    else:
        raise RuntimeError("lncc: 64 draws without a well-conditioned case")
    c = _new(*c0, sp, dtype, N)
    c["inputs"].update(I=I.astype(dtype), J=J.astype(dtype), g=g.astype(dtype))
    c["params"].update(sigma=sigma, mode=mode, kind=kind, draw=draw)
    c["_ref"] = dict(zip(("cc", "dI", "dJ"), ref))
    c["_emu"] = dict(zip(("cc", "dI", "dJ"), emu))
    tmax = gauss_tile_max(dtype)
    per = isinstance(sigma, tuple)
    filtered = [a for a in range(d) if (sigma[a] if per else sigma) > 0]
    strided = [sp[a] for a in filtered if a != d - 1]
    c["tags"] |= {f"{d}d", kind, mode, "per_axis_sigma" if per else "scalar_sigma", "row_gt128" if sp[-1] > 128 else "row_le128"}
    if strided:
        c["tags"].add("strided_several_tiles" if max(strided) > tmax else "strided_one_tile")   # gauss.hpp:86-89
    if len(filtered) < d:
        c["tags"].add("unfiltered_axis")
    return c


def _valid_lncc(c):
    import gauss_ref

    I, J, g, p = c["inputs"]["I"], c["inputs"]["J"], c["inputs"]["g"], c["params"]
    sig = gauss_ref.per_axis(p["sigma"], len(c["sp"]))
    # similarity._check / lagomorph_ext._check_lncc_pair
    return [m for ok, m in ((I.shape == J.shape == g.shape and I.ndim - 2 == len(c["sp"]) in (2, 3), "shapes"),
                            (I.dtype == J.dtype == g.dtype == c["dtype"], "dtype"), (p["mode"] in ("wrap", "zero"), "mode"),
                            (all(gauss_ref.radius(s) <= GAUSS_MAX_RADIUS for s in sig), "radius")) if not ok]


def _ref_lncc(c):
    import lncc_ref

    p = c["params"]
    return dict(zip(("cc", "dI", "dJ"), lncc_ref.lncc_with_grads(c["inputs"]["I"], c["inputs"]["J"], c["inputs"]["g"], p["sigma"], mode=p["mode"])))


def _native_lncc(c):
    """lncc_ref.emulate of the case's precision."""
    return {k: v.astype(c["dtype"]) for k, v in c["_emu"].items()} if "_emu" in c else None


def _judge_lncc(c, out, ref, fails, worst):
    """tests/test_gpu_lncc.py: cc, dI and dJ within lncc_ref.units <= 1."""
    import lncc_ref

    for k in ("cc", "dI", "dJ"):
        if out[k].shape != ref[k].shape or out[k].dtype != c["dtype"]:
            fails.append(f"{k}: {out[k].shape} {out[k].dtype}")
            continue
        u = float(units(out[k], ref[k], c["dtype"]))
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), u)
        if not u <= 1.0:
            fails.append(f"{k}: {u:.3g} x RTOL x max|ref|")


# ------------------------------------------------------------------ bspline_prefilter / interp_bspline  (csrc/bspline.hip)

BS_STAGED_MAX = 256   # bspline.hip:39 kBsStagedMax


def _case_bspline(rng, c0):
    cap = CAPS["bspline"]
    if rng.random() < 0.35:   # a line above kBsStagedMax on a random axis
        d, n = int(rng.choice([2, 3])), int(rng.choice([257, 300, 513]))
        rest = _shape(rng, cap // n, d=d - 1)
        at = int(rng.integers(0, d))
        sp = rest[:at] + (n,) + rest[at:]
    else:
        sp = _shape(rng, cap)
    N, K, dtype = int(rng.integers(1, 4)), int(rng.integers(1, 4)), _dtype(rng)
    c = _new(*c0, sp, dtype, N)
    d = len(sp)
    bc = bool(rng.random() < 0.3)
    rows = [(1, 1), (1, 3), (2, 2), (7, 10)][int(rng.integers(0, 4))]   # prefilter rows 1 .. 70
    if rows[0] * rows[1] * int(np.prod(sp)) > 60_000:
        rows = (1, 3)
    c["inputs"].update(I=rng.standard_normal(rows + sp).astype(dtype), C=rng.standard_normal(((1 if bc else N), K) + sp).astype(dtype),
                       u=_displacement(rng, N, sp, dtype, amps=(0.3, 1.5, 6.0)), go=rng.standard_normal((N, K) + sp).astype(dtype))
    c["params"].update(adjoint=bool(rng.random() < 0.5), dt=float(rng.choice([1.0, 1.0, -0.7, 0.5])), need=str(rng.choice(["both", "separate"])))
    for name, n in zip("xyz"[3 - d:], sp):
        c["tags"].add(f"{name}_staged" if n <= BS_STAGED_MAX else f"{name}_long")   # bspline.hip:182, :192
    c["tags"] |= {f"{d}d", "adjoint" if c["params"]["adjoint"] else "forward", "broadcast" if bc else "per_item",
                  "need_" + c["params"]["need"], "rows_70" if rows == (7, 10) else "rows_few"}
    return c


def _valid_bspline(c):
    x, sp, N = c["inputs"], c["sp"], c["N"]
    # lagomorph_ext.bspline_prefilter / _check_bspline
    return [m for ok, m in ((len(sp) in (2, 3) and x["I"].shape[2:] == sp and x["C"].shape[2:] == sp, "shape"),
                            (x["C"].shape[0] in (1, N) and x["u"].shape == (N, len(sp)) + sp and x["go"].shape == (N, x["C"].shape[1]) + sp, "batch"),
                            (all(v.dtype == c["dtype"] for v in x.values()), "dtype"), (bool(np.isfinite(x["u"]).all()), "finite")) if not ok]


def _ref_bspline(c):
    import bspline_ref

    x, p, dtype = c["inputs"], c["params"], c["dtype"]
    kw = dict(wfun=bspline_ref.weights_wide, add_dtype=np.longdouble) if dtype == np.float64 else {}   # (tests/test_gpu_bspline.py)
    C64 = x["C"].astype(np.float64)
    return {"prefilter": bspline_ref.prefilter(x["I"], p["adjoint"]), "values": bspline_ref.interp(C64, x["u"], p["dt"]),
            "d_u": bspline_ref.grad_u(x["go"], C64, x["u"], p["dt"]), "_wide": bspline_ref.grad_C_wide(x["go"], x["C"].shape, x["u"], p["dt"], **kw)}


def _native_bspline(c):
    """d_C by the walk in the kernel's own precision (bspline_ref.weights_f32 and adds in the dtype); the rest rounded."""
    import bspline_ref

    x, p = c["inputs"], c["params"]
    ref = reference(c)
    s = bspline_ref.grad_C_wide(x["go"], x["C"].shape, x["u"], p["dt"], wfun=bspline_ref.weights_f32, add_dtype=c["dtype"].type)[0]
    return {"prefilter": ref["prefilter"].astype(c["dtype"]), "values": ref["values"].astype(c["dtype"]), "d_u": ref["d_u"].astype(c["dtype"]),
            "d_C": s.astype(c["dtype"])}


def _judge_bspline(c, out, ref, fails, worst):
    """tests/test_gpu_bspline.py: prefilter, values and d_u within RTOL x max|reference|, d_u exactly 0 along a clamped
    axis; d_C cell by cell within bspline_ref.cell_bound of the wide sums, empty cells exactly 0."""
    import bspline_ref

    for k in ("prefilter", "values", "d_u"):
        close(out[k], ref[k], c["dtype"], k, fails=fails, worst=worst)
    tp = bspline_ref.taps(c["inputs"]["u"], c["params"]["dt"])
    if out["d_u"].shape == ref["d_u"].shape:
        for a in range(len(c["sp"])):
            if not (np.asarray(out["d_u"])[:, a][tp[a][3]] == 0).all():
                fails.append(f"d_u: not exactly 0 along clamped axis {a}")
    if out["d_C"].shape != ref["_wide"][0].shape:
        fails.append(f"d_C: shape {out['d_C'].shape}")
        return
    ratio, empty_ok = bspline_ref.cell_ratio(out["d_C"], ref["_wide"], c["dtype"], len(c["sp"]))
    if worst is not None:
        worst["d_C"] = max(worst.get("d_C", 0.0), ratio)
    if not empty_ok:
        fails.append("d_C: a cell that receives nothing is not exactly 0")
    if not ratio <= 1.0:
        fails.append(f"d_C: worst cell at {ratio:.3g} of its bound")


# ------------------------------------------------------------------ the module's surface

def case(family, seed, index):
    if family not in FAMILIES:
        raise KeyError(f"no generator for {family!r} (families: {FAMILIES}; not built yet: {PENDING})")
    c = globals()["_case_" + family](_rng(family, seed, index), (family, seed, index))
    unknown = c["tags"] - set(TAGS[family])
    assert not unknown, f"{family}: tags {unknown} are not in TAGS"
    return c


def cases(family, seed, count):
    return [case(family, seed, i) for i in range(count)]


def valid(c):
    """The entry point's argument checks, restated: the list of those the case fails (empty: it is accepted)."""
    return globals()["_valid_" + c["family"]](c)


def reference(c):
    """name -> array of the family's reference (names that start with '_' are the judge's own: bounds, wide sums)."""
    if "_ref" not in c:
        c["_ref"] = globals()["_ref_" + c["family"]](c)
    return c["_ref"]


def rounded(c):
    """The reference's outputs rounded to the dtypes the library returns."""
    ref = reference(c)
    out = {k: (v.astype(c["dtype"]) if RULES[c["family"]][k] in ("rel", "voxel", "entry", "energy", "operator") else v) for k, v in ref.items() if not k.startswith("_")}
    if c["family"] == "interp_points":
        out["d_F"] = ref["_wide"][0].astype(c["dtype"])
    if c["family"] == "bspline":
        out["d_C"] = ref["_wide"][0].astype(c["dtype"])
    return out


def native(c):
    """The family's native-precision restatement of the outputs, or None where there is none for this case."""
    f = globals().get("_native_" + c["family"])
    return f(c) if f is not None else None


def judge(family, c, outputs, worst=None):
    """The failures of `outputs` (name -> numpy array) by the family's own rule, as strings; [] when it passes.  `worst`,
    a dict, collects the largest fraction of each bound."""
    fails = []
    names = [k for k in rounded(c)]
    missing = [k for k in names if k not in outputs]
    if missing:
        return [f"{family}: outputs {missing} are missing"]
    globals()["_judge_" + family](c, outputs, reference(c), fails, worst)
    return fails


# which outputs the families' own tests call bit-reproducible from call to call ...
REPRODUCIBLE = {"surface_distance": ("hausdorff", "hd95", "assd"), "lncc": ("cc", "dI", "dJ"),
                "bspline": ("prefilter", "values", "d_u"), "energy": ("E", "A"), "ffd_expand": ("forward", "adjoint"), "invert_displacement": ("v", "lam", "rough"), "gaussian_smooth": ("out",), "jacobian_determinant": ("forward", "backward"), "joint_histogram": ("P", "dI", "dJ"), "warp_labels": ("out",),
                "label_overlap": ("counts",), "distance_transform": ("squared", "root"), "interp_points": ("out", "d_x")}
# ... and for which they assert or imply that an item alone has the bits of its slice of the batch: the outputs judged
# bit for bit against a reference that is computed item by item, and the histogram's rows (test_gpu_mi.py: a channel
# slice run alone equals the slice of the whole, all three outputs)
ITEM_BITS = {"surface_distance": (), "lncc": (), "bspline": (), "energy": (), "ffd_expand": (), "invert_displacement": (), "gaussian_smooth": (), "jacobian_determinant": ("forward",), "joint_histogram": ("P", "dI", "dJ"), "warp_labels": ("out",),
             "label_overlap": ("counts",), "distance_transform": (), "interp_points": ()}
# the rule of each output: "bits", "rel" (RTOL x max|reference|), "cells" (scatter_bound), "edt" (bits at unit spacing, else REL),
# "surface" (1e-6 |reference| per entry), "bcells" (bspline_ref.cell_bound),
# "energy" / "operator" (tests/test_gpu_energy.py: 1e-12 in float64; 1e-5 E per item and energy_ref.operator_bound in float32),
# "voxel" (ffd_ref.voxel_bound and RTOL x max|reference|), "entry" (ffd_ref.entry_bound in float32, 1e-12 max|reference| in float64)
RULES = {"surface_distance": {"hausdorff": "surface", "hd95": "surface", "assd": "surface"}, "lncc": {"cc": "rel", "dI": "rel", "dJ": "rel"},
         "bspline": {"prefilter": "rel", "values": "rel", "d_u": "rel", "d_C": "bcells"}, "energy": {"E": "energy", "A": "operator"}, "ffd_expand": {"forward": "voxel", "adjoint": "entry"}, "invert_displacement": {"v": "rel", "lam": "rel", "rough": "bits", "rough_loop": "bits"}, "gaussian_smooth": {"out": "rel"},
         "jacobian_determinant": {"forward": "bits", "backward": "rel"}, "joint_histogram": {"P": "bits", "dI": "rel", "dJ": "rel"},
         "warp_labels": {"out": "bits"}, "label_overlap": {"counts": "bits"}, "distance_transform": {"squared": "edt", "root": "edt"},
         "interp_points": {"out": "rel", "d_x": "rel", "d_F": "cells"}}
# inputs that are NOT sliced with the batch item (a leading 1: broadcast) are found by their leading extent


def judged(c):
    """The names of the outputs that the family's rule judges on this case."""
    return tuple(k for k in RULES[c["family"]] if not (c["family"] == "energy" and k == "E" and "affine" in c["tags"]))


def item_case(c, n):
    """The case of batch item n alone: inputs with the batch's leading extent are cut to [n:n+1], broadcast ones stay."""
    sub = dict(c, N=1, inputs={k: (np.ascontiguousarray(v[n:n + 1]) if v.shape[0] == c["N"] and not _is_broadcast(c, k) else v)
                               for k, v in c["inputs"].items()})
    sub.pop("_ref", None)
    if c["family"] == "joint_histogram":   # an automatic range is taken from the whole tensor: the item keeps the batch's
        rI, rJ = _mi_ranges(c)
        sub["params"] = dict(c["params"], range_I=rI, range_J=rJ)
    if "_ref" in c:   # every reference here is computed item by item: the item's reference is its slice ...
        cut = lambda v: tuple(cut(w) for w in v) if isinstance(v, tuple) else (v[n:n + 1] if v.shape[0] == c["N"] else v)
        sub["_ref"] = {k: cut(v) for k, v in c["_ref"].items()}
        if c["family"] == "interp_points" and "broadcast" in c["tags"]:   # ... but for the sum over the items into one d_F
            import points_ref

            sub["_ref"]["_wide"] = points_ref.scatter_wide(sub["inputs"]["go"], sub["inputs"]["x"], c["sp"], 1)
        if c["family"] == "bspline" and "broadcast" in c["tags"]:
            import bspline_ref

            kw = dict(wfun=bspline_ref.weights_wide, add_dtype=np.longdouble) if c["dtype"] == np.float64 else {}
            x = sub["inputs"]
            sub["_ref"]["_wide"] = bspline_ref.grad_C_wide(x["go"], x["C"].shape, x["u"], c["params"]["dt"], **kw)
    return sub


def _is_broadcast(c, name):
    return "broadcast" in c["tags"] and name in ("L", "F", "C")


def item_slice(c, outputs, n):
    """Item n of the outputs of the batch (an output summed over the items of a broadcast input has none: left out)."""
    return {k: v[n:n + 1] for k, v in outputs.items() if not (k in ("d_F", "d_C") and "broadcast" in c["tags"])}
