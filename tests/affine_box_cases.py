"""Matrices, translations and grids for the tests of the affine box splat (affine_splat_box_kernel and the functions of
lagomorph_amd/csrc/affine_box.hpp it calls).  Shared by tests/test_affine_box_cover.py (host walk of the real
candidate / ownership code), tests/test_affine_ref.py (reference pins, sensitivity of the GPU cases) and
tests/test_gpu_affine_partition.py.  Everything here is float32-exact by construction: a value is rounded to float32
before anything is derived from it.

The adversarial family.  A regular matrix (common.hpp: affine_item_regular) may have entries just below 1e3 as long as
its inverse's rows sum to at most 4.  Such a matrix is a large rank-one part plus a small well-conditioned one,

    A = a u v^T + g C,     a u_i v_j in 500 .. 999.99,  C a rotation,  g solved so that max row sum |A^-1| = target,

so that A f is small -- lands inside the grid -- exactly where v . f is nearly 0 while every product of the fma chain
of the position (cuda/affine.cu:42-61) is of the order 1e3 n / 2: an in-grid position is the small difference of terms
whose float32 ulp is 2^-6 for n >= 263.  The inverse then carries that error back into source space times up to 4.
`a` is not float32-representable times anything convenient (999.3, 873.7, ...): products of representable entries with
half-integers are exact and would hide the effect.
"""
import numpy as np

BOX = (8, 8, 48)   # affine_splat_boxes (affine.hip): BX, BY, BZ


def f32(x):
    return np.asarray(x, dtype=np.float32)


def inv_rowsum(A):
    """max row sum of |A^-1| in double, of the float32-rounded matrix: the quantity affine_item_regular limits to 4."""
    Ai = np.linalg.inv(f32(A).astype(np.float64))
    return float(np.abs(Ai).sum(axis=1).max())


def rotation(ax, ang):
    c, s = np.cos(ang), np.sin(ang)
    R = np.eye(3)
    i, j = [(1, 2), (0, 2), (0, 1)][ax]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


# ---------------------------------------------------------------- mild family (sanity anchor)

def mild_matrices():
    """identity and the six kinds of tests/test_gpu_parity.py::test_affine_backward_tiled_splat (both items of each)."""
    rng = np.random.default_rng(77)
    c, s = np.cos(0.6), np.sin(0.6)
    out = {
        "identity": np.eye(3),
        "near_identity0": np.eye(3) + 0.02 * rng.standard_normal((3, 3)),
        "near_identity1": np.eye(3) + 0.02 * rng.standard_normal((3, 3)),
        "rotation0": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]),
        "rotation1": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]),
        "zoom0": 2.5 * np.eye(3),
        "zoom1": 0.4 * np.eye(3),
        "flip0": np.diag([1.0, 1.0, -1.0]),
        "flip1": np.diag([-1.0, 1.0, 1.0]),
        "singular0": np.array([[1.0, 0.5, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),       # not regular
        "singular1": np.eye(3) + 0.05 * rng.standard_normal((3, 3)),
        "shear_far0": np.diag([0.05, 0.04, 1.0]),                                          # not regular
        "shear_far1": np.array([[1.0, 0.9, 0.0], [0.0, 1.0, 0.8], [0.3, 0.0, 1.0]]),
        "small_det": np.diag([0.26, 0.26, 0.26]),   # |det| = 0.0176, inverse rows 3.85: about the smallest a regular matrix has
    }
    return {k: f32(v) for k, v in out.items()}


MILD_REGULAR = {"singular0": False, "shear_far0": False}   # every other mild matrix is regular


# ---------------------------------------------------------------- adversarial family

def adversarial_matrix(a, target, two_entry, seed, neg_row=None):
    """float32 (3, 3) as in the module docstring.  two_entry: only x and z mix (y is an identity row and column), rows
    with two large entries; else rows with three."""
    rng = np.random.default_rng(seed)
    u = 0.80 + 0.19 * rng.random(3)
    v = 0.80 + 0.19 * rng.random(3)
    u[0] = v[0] = 0.995   # the largest entry is 0.99 a
    C = rotation(1, 0.7 + rng.random()) if two_entry else rotation(0, 0.4 + rng.random()) @ rotation(1, 0.9 + rng.random()) @ rotation(2, 0.3 + rng.random())
    if two_entry:
        u[1] = v[1] = 0.0

    def make(g):
        A = a * np.outer(u, v) + g * C
        if two_entry:
            A[1, :] = A[:, 1] = 0.0
            A[1, 1] = 1.0
        if neg_row is not None:
            A[neg_row] = -A[neg_row]
        return f32(A)

    lo, hi = 1e-3, 64.0   # the row sum falls as g grows
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if inv_rowsum(make(mid)) > target:
            lo = mid
        else:
            hi = mid
    A = make(hi)
    big = np.abs(A[A != 0]) if not two_entry else np.abs(A[np.ix_([0, 2], [0, 2])])
    assert big.min() >= 500.0 and np.abs(A).max() <= 999.99, A
    assert target - 0.02 <= inv_rowsum(A) <= min(target, 4.0), (inv_rowsum(A), target)
    return A


# name -> (a, target row sum, two_entry, seed, negated row)
ADVERSARIAL = {
    "two_a": (999.3, 3.98, True, 1, None),
    "two_b": (873.7, 3.5, True, 2, None),
    "two_c": (999.3, 3.8, True, 3, 2),
    "three_a": (999.3, 3.98, False, 4, None),
    "three_b": (761.9, 3.6, False, 5, None),
    "three_c": (999.3, 3.9, False, 6, 0),
}
EXTENTS = (128, 256, 320, 512)   # of the mixed axes x and z; y (its row mixes too for three_*) stays at 16
OFFSETS = (0.0, 1e-3, 4e-3, 1.5e-2)


def adversarial_matrices():
    return {k: adversarial_matrix(*p) for k, p in ADVERSARIAL.items()}


def _sources(A, shape):
    """Two in-grid sources whose products in the position's fma chain are large: one far out on the plane v . f = 0
    where A f itself cancels, one next to a grid corner where A f is of the order 1e3 n and the translation cancels it."""
    n = np.array(shape)
    o = 0.5 * (n - 1)
    A = A.astype(np.float64)
    v = A[0]
    fi = round(0.35 * n[0])
    j = min(3, n[1] - 1)
    fk = -(v[0] * fi + v[1] * (j - o[1])) / v[2]
    k = int(np.clip(round(fk + o[2]), 0, n[2] - 1))
    return [(int(round(o[0] + fi - 0.5)), j, k), (n[0] - 2, n[1] - 2, n[2] - 3)]


def directed_translations(A, shape, offsets=OFFSETS):
    """[(tag, T float32 (3,), source, corner q, offset (3,))]: for each of the eight corner types q of a box that is interior on x and
    z, and each d, translations that send an in-grid source to that corner moved by d along the diagonal into the box and
    out of it (the other six sign patterns at this corner are the inward / outward pair of another corner type of a
    neighbouring box, which the eight q cover).  T is rounded to float32, so the hit is exact to an ulp of |T|."""
    n = np.array(shape)
    o = 0.5 * (n - 1)
    nb = [-(-int(n[d]) // BOX[d]) for d in range(3)]
    # the corner planes per axis: two neighbouring box faces in the middle of the grid, never a face of the grid itself (y
    # with 16 cells has two boxes and one plane inside, at 8: both corner types use it)
    plane = []
    for d in range(3):
        inside = [m * BOX[d] for m in range(1, nb[d]) if m * BOX[d] < n[d] - 1] or [0]
        mid = (len(inside) - 1) // 2
        plane.append((inside[mid], inside[min(mid + 1, len(inside) - 1)]))
    A64 = f32(A).astype(np.float64)
    out = []
    srcs = _sources(A, shape)
    for q in range(8):
        bits = np.array([(q >> 2) & 1, (q >> 1) & 1, q & 1])
        P = np.array([float(plane[d][bits[d]]) for d in range(3)])
        inward = np.where(bits == 1, -1.0, 1.0)
        for d in offsets:
            for sgn in ((1.0,) if d == 0 else (1.0, -1.0)):
                for si, s in enumerate(srcs):
                    off = sgn * d * inward
                    T = (P + off) - o - A64 @ (np.array(s) - o)
                    out.append((f"q{q}_d{d:g}_{'in' if sgn > 0 else 'out'}_s{si}", f32(T), s, q, off))
    return out


# ---------------------------------------------------------------- thresholds of affine_item_regular

def threshold_matrices():
    """name -> (float32 matrix, regular?) on both sides of every threshold, adjacent float32 values.  The expected
    answers follow from exact arithmetic on the float32 values: max |a| < 1e3; inverse row sum <= 4 (1 / 0.25 = 4 exactly
    in double); |det| > 1e-3.  A matrix with |det| near 1e-3 cannot have inverse rows that sum to 4 or less (that needs
    every singular value above 1 / (4 sqrt 3), i.e. |det| > 3e-3), so both sides of the determinant threshold are
    irregular -- the threshold only guards the division."""
    one = np.float32(1.0)
    below_1000 = np.nextafter(np.float32(1000.0), np.float32(0.0))
    q_lo = np.nextafter(np.float32(0.25), np.float32(0.0))
    # diag(0.1, 0.1, x): det = 0.1f * 0.1f * x in double crosses 1e-3 between two adjacent float32 x
    t = np.float64(np.float32(0.1))
    x = np.float32(1e-3 / (t * t))
    while np.float64(x) * t * t > 1e-3:
        x = np.nextafter(x, np.float32(0.0))
    x_below, x_above = x, np.nextafter(x, np.float32(1.0))
    assert np.float64(x_below) * t * t <= 1e-3 < np.float64(x_above) * t * t
    out = {
        "max_1000": (np.diag([np.float32(1000.0), one, one]), False),
        "max_below_1000": (np.diag([below_1000, one, one]), True),
        "max_neg_1000": (np.array([[1, 0, 0], [0, 1, 0], [-1000.0, 0, 1]]), False),
        "rowsum_4": (np.diag([one, one, np.float32(0.25)]), True),
        "rowsum_above_4": (np.diag([one, one, q_lo]), False),
        "det_above_1e-3": (np.diag([np.float32(0.1), np.float32(0.1), x_above]), False),
        "det_below_1e-3": (np.diag([np.float32(0.1), np.float32(0.1), x_below]), False),
        "det_neg_below_1e-3": (np.diag([np.float32(0.1), np.float32(-0.1), x_below]), False),
    }
    # a sheared pair around the row-sum limit: the inverse of [[1,0,0],[0,1,0],[s,0,c]] has the last row (-s/c, 0, 1/c);
    # s = 0.5, c = 0.375: 1.5 * RN(8/3) rounds to 4 or to the double below it, never above
    out["rowsum_4_sheared"] = (np.array([[1, 0, 0], [0, 1, 0], [0.5, 0, 0.375]]), True)
    out["rowsum_above_4_sheared"] = (np.array([[1, 0, 0], [0, 1, 0], [np.nextafter(np.float32(0.5), one), 0, 0.375]]), False)
    return {k: (f32(A), r) for k, (A, r) in out.items()}


def nonfinite_matrices():
    """Host only: the decision must be 'not regular'.  Never sent to a GPU."""
    nan = np.eye(3)
    nan[1, 2] = np.nan
    inf = np.eye(3)
    inf[0, 0] = np.inf
    ninf = np.eye(3)
    ninf[2, 1] = -np.inf
    return {"nan_entry": f32(nan), "inf_entry": f32(inf), "neg_inf_entry": f32(ninf), "zero": f32(np.zeros((3, 3)))}


# ---------------------------------------------------------------- the GPU cases (tests/test_gpu_affine_partition.py)

# (matrix name, grid, translation tags of the two batch items, offsets the tags were made with): the matrices and directed
# translations the host walk (tests/test_affine_box_cover.py) ranked highest by needed slack, at the extents that made
# them so; profiles/affine_box_margin.md has the whole table.  Needed slack in voxels, shipped slack 0.021 .. 0.025.
GPU_ADVERSARIAL = [
    ("three_c", (512, 16, 512), ("q0_d0_in_s1", "q5_d0.001_out_s1"), OFFSETS),        # 0.0356, 0.0356
    ("two_c", (512, 16, 512), ("q7_d0_in_s1", "q7_d0.004_out_s1"), OFFSETS),          # 0.0236, 0.0236
    ("two_c", (263, 40, 263), ("q0_d0_in_s1", "q7_d0.004_in_s1"), (0.0, 4e-3)),       # 0.0199, 0.0199
    ("two_b", (512, 16, 512), ("q6_d0.004_in_s0", "q1_d0.004_out_s0"), OFFSETS),      # 0.0140, 0.0140
    ("two_a", (321, 17, 300), ("q0_d0.004_out_s1", "q3_d0_in_s0"), (0.0, 4e-3)),      # 0.0124, 0.0000
    ("three_c", (320, 16, 320), ("q0_d0.001_in_s0", "q5_d0.001_out_s0"), OFFSETS),    # 0.0039, 0.0029
    ("three_a", (128, 16, 128), ("q1_d0.001_out_s0", "q4_d0.001_in_s0"), OFFSETS),    # 0.0034, 0.0004
]


def gpu_adversarial_cases():
    """[(name, shape, A (2, 3, 3), T (2, 3), [directed source of item 0, of item 1])]"""
    mats = adversarial_matrices()
    out = []
    for name, shape, tags, offsets in GPU_ADVERSARIAL:
        tr = {t[0]: t for t in directed_translations(mats[name], shape, offsets)}
        A = np.stack([mats[name], mats[name]])
        T = np.stack([tr[t][1] for t in tags])
        out.append((f"{name}_{'x'.join(map(str, shape))}", shape, A, T, [tuple(int(v) for v in tr[t][2]) for t in tags]))
    return out


def gpu_go(rng, shape, dtype):
    """grad_out bounded away from zero, so that no term is accidentally tiny: sign * (0.5 + |N(0, 1)|)."""
    g = rng.standard_normal(shape)
    return (np.where(g < 0, -1.0, 1.0) * (0.5 + np.abs(g))).astype(dtype)


def gpu_adversarial_inputs(idx, dtype=np.float32):
    """(name, shape, A, T, directed sources, grad_out) of committed case idx: batch 2, one channel."""
    name, shape, A, T, srcs = gpu_adversarial_cases()[idx]
    go = gpu_go(np.random.default_rng(1000 + idx), (2, 1) + shape, np.float32)
    return name, shape, A.astype(dtype), T.astype(dtype), srcs, go.astype(dtype)
