"""Inputs shared by tests/test_oracle_wide.py (CPU) and tests/test_gpu_scatter_cells.py (GPU): the scatter-add cases of
the max-norm tests.  The affine, regrid and hessian builders reproduce those tests' inputs value for value; interp_inputs
has the same construction (the `_disp` field, normal grad_out) and its own seeds, so its values are not the parity
suite's."""
import numpy as np

LDS2D_SHAPES = [(128, 128), (64, 128), (130, 200), (50, 333), (256, 72)]   # test_interp_backward_2d_lds_splat
AFFINE_KINDS = ["near_identity", "rotation", "zoom", "flip", "singular", "shear_far"]
REGRID_CASES = [((20, 12, 40), (40, 24, 80), 1.0), ((40, 24, 80), (20, 12, 40), 1.0), ((33, 17, 65), (33, 17, 65), 1.0),
                ((16, 16, 16), (24, 20, 90), -0.8), ((12, 10, 14), (30, 22, 66), 7.0), ((12, 10, 14), (30, 22, 66), 0.05),
                ((1, 2, 3), (5, 4, 7), 1.0), ((48, 40), (96, 100), 1.0), ((64, 50), (20, 30), 2.5),
                ((64, 64, 64), (128, 128, 128), 1.0)]                      # test_regrid_backward_every_form
REGRID_SEP_ENTRY = [([1.0e9, 3.0, 4.0], [1.0, 0.5, 0.5]), ([3.0, 3.0, 4.0], [2.0e6, 0.5, 0.5]),
                    ([3.0, 3.0, 4.0], [1e-9, 0.5, 0.5]), ([3.0, 3.0, 4.0], [1e-3, 0.5, 0.5]),
                    ([3.0, 3.0, 4.0], [0.5, -0.5, 0.5])]                   # test_regrid_backward_separable_entry_...


def normal(rng, shape, npdt, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(npdt)


def disp(rng, nn, sp, npdt):
    """test_gpu_parity._disp: clamp (far out of range), the negative floor rule, exact-integer positions."""
    u = normal(rng, (nn, len(sp)) + tuple(sp), npdt, 1.7)
    flat = u.reshape(-1)
    flat[::11] *= 9.0
    flat[::7] = np.round(flat[::7])
    flat[::13] = -np.abs(flat[::13]) - 0.25
    return u


def smooth_disp(rng, nn, sp, npdt, amp=3.0, sigma=6.0):
    """A smooth displacement of at most `amp` voxels (the 2D LDS test's 'smooth' kind, any dimension)."""
    from scipy.ndimage import gaussian_filter

    sig = min(sigma, max(min(sp) / 4.0, 0.5))
    u = gaussian_filter(rng.standard_normal((nn, len(sp)) + tuple(sp)), sigma=(0, 0) + (sig,) * len(sp), mode="wrap")
    return (u * (amp / np.abs(u).max())).astype(npdt)


def interp_inputs(sp, nn, nc, npdt, kind="wild", seed=1):
    """(go, u) of an interp_backward case."""
    rng = np.random.default_rng(hash((tuple(sp), nn, nc, seed)) % 2**31)
    u = disp(rng, nn, sp, npdt) if kind == "wild" else smooth_disp(rng, nn, sp, npdt)
    go = normal(rng, (nn, nc) + tuple(sp), npdt)
    return go, u


def affine_kind_inputs(kind, bc, npdt):
    """(go, I, A, T) of test_gpu_parity.test_affine_backward_tiled_splat."""
    rng = np.random.default_rng(77)
    sp, nn, nc = (36, 20, 70), 2, 2
    I = normal(rng, ((1 if bc else nn), nc) + sp, npdt)
    A = np.eye(3)[None].repeat(nn, 0)
    if kind == "near_identity":
        A = A + 0.02 * rng.standard_normal((nn, 3, 3))
    elif kind == "rotation":
        c, s = np.cos(0.6), np.sin(0.6)
        A[0] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        A[1] = [[1, 0, 0], [0, c, -s], [0, s, c]]
    elif kind == "zoom":
        A = A * np.array([2.5, 0.4])[:, None, None]
    elif kind == "singular":
        A[0] = [[1.0, 0.5, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
        A[1] = A[1] + 0.05 * rng.standard_normal((3, 3))
    elif kind == "shear_far":
        A[0] = [[0.05, 0.0, 0.0], [0.0, 0.04, 0.0], [0.0, 0.0, 1.0]]
        A[1] = [[1.0, 0.9, 0.0], [0.0, 1.0, 0.8], [0.3, 0.0, 1.0]]
    else:
        assert kind == "flip", kind
        A[0, 2, 2] = -1.0
        A[1, 0, 0] = -1.0
    A = A.astype(npdt)
    T = (2.0 * rng.standard_normal((nn, 3))).astype(npdt)
    go = normal(rng, (nn, nc) + sp, npdt)
    return go, I, A, T


def regrid_inputs(sp, out, scale, npdt):
    """(go, origin, spacing) of test_gpu_parity.test_regrid_backward_every_form."""
    rng = np.random.default_rng(78)
    origin = [(s - 1) * 0.5 - 0.2 for s in sp]
    spacing = [scale * (a - 1) / (b - 1) for a, b in zip(sp, out)]
    go = normal(rng, (2, 3) + tuple(out), npdt)
    return go, origin, spacing


def regrid_sep_entry_inputs(npdt):
    """(go, sp, out) of test_regrid_backward_separable_entry_accepts_what_the_reference_accepts."""
    rng = np.random.default_rng(31)
    sp, out = (6, 8, 20), (9, 10, 33)
    return normal(rng, (2, 2) + out, npdt), sp, out


def hessian_inputs(npdt, sp=(9, 8), nn=2, nc=3):
    """(I, u) of test_gpu_parity.test_interp_hessian_diagonal (default arguments), or the same at another shape."""
    rng = np.random.default_rng(11)
    I = normal(rng, (nn, nc) + tuple(sp), npdt)
    u = disp(rng, nn, sp, npdt)
    return I, u
