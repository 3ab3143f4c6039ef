/*
 * lagomorph_hip.h -- C ABI of liblagomorph_hip.so, the MI355X (gfx950) HIP
 * implementation of lagomorph's deform / interp / metric / adjrep hot path.
 *
 * This is the drop-in boundary: each entry point replaces one function of the
 * reference's `lagomorph_ext` pybind11 module
 * (/root/reference/lagomorph/extension/extension.cpp:175-189).  Signatures are
 * plain C: raw device pointers, 64-bit extents, scalar parameters, flags, and
 * the hipStream_t to launch on (as void*; NULL = the null stream).  No torch
 * types, no allocation, no host synchronisation (except in debug mode).
 *
 * Conventions
 *  - Every tensor is dense, contiguous, batch-major N C (D) H W with the LAST
 *    spatial axis fastest, exactly as the reference indexes it
 *    (include/extrap.h:15-21: index = (x*sizeY + y)*sizeZ + z).
 *  - `dim` is 2 or 3.  For dim == 2 pass nz = 1 (ignored).
 *  - Each function exists for float (`_f32`) and double (`_f64`); the
 *    reference dispatches both via AT_DISPATCH_FLOATING_TYPES.
 *  - Outputs are written in full by the call (splat targets are zeroed on the
 *    stream before the kernel), so callers may pass uninitialised buffers.
 *  - Return value: LAGO_OK (0), LAGO_ERR_INVALID (-1: bad argument; nothing
 *    was launched) or LAGO_ERR_HIP (-2: a HIP runtime call failed).
 *    lago_last_error() returns a thread-local description.
 *  - Extent limits: nx*ny*nz < 2^29 per batch item (one channel plane is addressed
 *    with 32-bit byte offsets); whole tensors are addressed with 64-bit offsets.
 */
#ifndef LAGOMORPH_HIP_H
#define LAGOMORPH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LAGO_OK 0
#define LAGO_ERR_INVALID (-1)
#define LAGO_ERR_HIP (-2)

/* (version 5 as before: no signature changed when extents whose product nx*ny*nz does not fit int64_t became
 * LAGO_ERR_INVALID in every entry point -- they used to wrap, and some wrapped values were accepted.  No tensor has
 * such a shape.) */
#define LAGO_ABI_VERSION 5

/* lago_gauss_smooth: the largest radius (taps on each side of the centre) a pass takes, and the border modes */
#define LAGO_GAUSS_MAX_RADIUS 32
#define LAGO_GAUSS_WRAP 0
#define LAGO_GAUSS_ZERO 1

/* lago_mi_histogram / lago_mi_backward: the bin counts B a table side takes, and the fraction bits of the fixed-point
 * histogram (one voxel's whole weight is 2^LAGO_MI_FRAC_BITS) */
#define LAGO_MI_MIN_BINS 4
#define LAGO_MI_MAX_BINS 64
#define LAGO_MI_FRAC_BITS 32

/* lago_warp_labels: how the label of a sample is chosen; lago_label_overlap: the most labels a count table takes */
#define LAGO_LABELS_NEAREST 0
#define LAGO_LABELS_VOTE 1
#define LAGO_LABELS_MAX 4096

/* lago_distance_transform: which voxels of the label map are features, and the largest extent an axis may have */
#define LAGO_EDT_NONZERO 0
#define LAGO_EDT_EQUAL 1
#define LAGO_EDT_NOT_EQUAL 2
#define LAGO_EDT_SURFACE 3
#define LAGO_EDT_MAX_EXTENT 1024

/* lago_field_energy, lago_field_energy_operator: which quadratic form of the field */
#define LAGO_ENERGY_DIFFUSION 0
#define LAGO_ENERGY_BENDING 1

/* lago_pyramid_down, lago_pyramid_up: which per-axis matrix (down applies R or E^T, up applies E or R^T) */
#define LAGO_PYRAMID_REDUCE 0
#define LAGO_PYRAMID_EXPAND 1

/* ---- housekeeping --------------------------------------------------------- */

/* replaces set_debug_mode (extension.cpp:105-107): when non-zero every entry
 * point synchronises its stream after the launch and reports kernel faults
 * through its return value (the reference only printed them, defs.h:17-23). */
void lago_set_debug(int on);
int lago_get_debug(void);
int lago_abi_version(void);
const char *lago_version(void);
const char *lago_last_error(void);

/* Tuning settings: ONE struct, read and written as a whole (the ABI does not grow per experiment).  The settings are
 * PROCESS-WIDE (two users of the library in one process share them), stored atomically field by field (they may be
 * changed while other host threads, e.g. autograd's backward threads, are inside entry points) and affect speed only,
 * never which results are produced beyond the rounding differences noted per field.  The defaults are what the product
 * runs with; the parity tests sweep them.  `struct_size` is sizeof(lago_tuning) as the CALLER was compiled: the
 * library reads / writes only that many bytes, so a caller built against an older header keeps working when fields
 * are appended. */
typedef struct lago_tuning {
    uint32_t struct_size;
    /* interp_backward: 0 global float atomics only (the reference's form), 1 LDS-privatised splat with atomic flush
     * (default for 3D float32) */
    int32_t splat_mode;
    /* general tiled LDS splat: source tile TX TY TZ (TZ = 0: whole z rows, split evenly above 128 voxels; TX = 0: about
     * 4096 voxels per tile), window margins MX MY MZ, threads per workgroup (256 / 512 / 1024).  Default 0 8 0 1 1 4 512 */
    int32_t splat_tile[7];
    /* sheared-window float32 3D displacement splat (csrc/splat.hip: splat_shear_kernel, the form interp_backward takes
     * for float32 3D fields): on (0 leaves every call to the general tiled kernel), source tile TX TY TZ (TX an upper
     * bound shrunk until the window fits 80 KB; TZ = 0: whole z rows, split evenly above 128 voxels), window margins
     * MX MY MZ around the probed origin, threads per workgroup.  Default 1, 8 6 0, 1 1 4, 1024.  d_u is bit-identical
     * under every setting; d_I differs by the order of its sums */
    int32_t splat_shear[8];
    /* several channels with d_u wanted, sheared-window kernel: 2 (default) each voxel's geometry -- window addresses,
     * gather offset, fractions -- and its d_u sums stay in registers over the channel loop (tiles of at most 2048
     * voxels), 1 only the d_u sums do (geometry recomputed per channel), 0 d_u is read-modify-written per channel.
     * Same d_u bits under every setting */
    int32_t splat_shear_mc;
    /* the same for the general tiled kernel: 1 (default) / 0 */
    int32_t splat_mc;
    /* 1 (default): the slab-unrolled 3D gather kernels (two voxels per lane) when the shape allows; 0: one-voxel-per-lane
     * kernels only */
    int32_t vector_kernels;
    /* 1 (default): every launch of the large kernels walks its workgroups in the opposite direction of the launch before
     * it, so that a consumer starts on what its producer wrote last -- still in the 256 MB Infinity Cache; 0: always
     * ascending.  Same results (scatter-add outputs differ in their last bits, as between any two runs).  The direction
     * is taken from ONE process-wide launch counter (every entry point that builds a launch geometry advances it, small
     * launches and calls that fail a later argument check included), so "opposite to its producer" holds for the chains
     * of large kernels the library itself issues back to back, and the last bits of scatter-add outputs (d_I) depend on
     * how many launches came before -- as they depend on the hardware's atomic ordering anyway; every other output is
     * bit-identical in both directions */
    int32_t launch_order;
    /* 1 (default): the 3D Jacobian / stencil terms of Ad_star and jacobian_times_vectorfield_backward are taken from an
     * LDS-staged tile of z-rows with a one-voxel halo (csrc/stencil_tile.hpp) where the shape allows -- 128^3 and 160^3
     * volumes through instantiations with their geometry compiled in; 3: row tiles without those instantiations; 0:
     * every neighbour is loaded from global memory.  Same bits */
    int32_t stencil_tile;
    /* 1 (default): float32 3D trilinear gathers of smooth fields (compose, interp_forward of several channels) stage the
     * source block of a tile of voxels in LDS with LDS-direct loads and take the corners from there
     * (csrc/gather_window.hpp) where the shape allows; 0: pair gathers through the vector L1 only.  Same bits */
    int32_t gather_window;
    /* lago_fluid_metric implementation.  3 (default): the tuned LDS-tiled FFT passes where they apply (float32 3D with nx
     * in {64,96,128,160,192,256} and (ny, nz) any pair of {64,96,128,160,192} or one of the power-of-two planes
     * 32x{64,128,256}, 64x256, 128x256, 256x{64,128}: lengths 2^a, 3*2^a, 5*2^a; since round 6 also nx in {176,208} and
     * the planes 208x176, 176x176, 176x208 -- 11*16 and 13*16: the 176 x 208 x 176 brain grid -- and nx in {112,144,224,240}
     * with the planes 112x96, 96x112, 112x112, 128x112, 112x128, 224x160, 160x224, 224x128, 144x144, 176x144, 144x176,
     * 240x160, 160x240 (odd factors 7, 9, 15), and nx in {80,88,104,120} with the planes 80x80, 104x88, 88x88, 88x104, 120x120
     * (a plane with ny % 16 = 8 needs nx % 16 = 8 as well); planes above the LDS or not in these lists, ny in {128,144,...,256}
     * (multiples of 16 with an odd factor up to 15) and nz from the same set -- since the lists hold every multiple of 16
     * from 64 to 256, ANY volume with such extents -- as rows + columns (five launches:
     * 256^3, 160 x 192 x 224, 192 x 224 x 192 ...); float32 2D planes up to 128 x 128 in
     * one fused kernel) and the generic hand-written passes of csrc/fftg.hip for every other shape and for float64
     * (any extent up to 4096 (float32) / 2048 (float64) points per axis, lines with a prime factor >= 29 through
     * Bluestein's convolution; a longer axis is the one case left to the spot-checked rocFFT path): no rocFFT call
     * otherwise.  2: the tuned passes, rocFFT for the rest (1: rocFFT 2D
     * (y, z) plan + fused x-axis pass, nx in {64,128,256}; 0: rocFFT 3D plan + operator kernel; a mode falls back to
     * the next lower one for shapes it does not support); the rocFFT plans are spot-checked against a direct DFT
     * (csrc/fft.hip).  Results agree to rounding.  4: as 3, with the generic passes' x transforms and operator as three
     * launches instead of the fused one (csrc/fftg.hip: fft_xop_kernel) -- the same bits; the comparison switch */
    int32_t fluid_mode;
    /* FFT-pass fluid metric: batch items per x-pass workgroup (0, the default: chosen by the size of the launch) */
    int32_t fluid_xpass_ipw;
    /* persistent prefetching zy kernels for planes above 80 KB of LDS (default 1) */
    int32_t fluid_zy_persist;
    /* 512-thread x-pass workgroups for the 256-point tile (default 1) */
    int32_t fluid_xpass_wide;
    /* x pass as a persistent grid of two workgroups per CU that prefetch their next tile (default 1: taken when the
     * launch has at least four (bin tile, batch item) pairs per workgroup; 2: always; 0: never).  Same bits */
    int32_t fluid_xpass_persist;
    /* affine_interp_backward (3D), the image splat: 1 (default) by target boxes for batch items whose matrix is
     * invertible with a moderate inverse (decided per item on the device), the general tiled LDS splat for the others;
     * 0: the general tiled splat for every item.  d_I differs by the order of its sums */
    int32_t affine_box;
    /* 1 (default): a compose called with the near-identity hint (lago_compose_near_*) and eligible for the LDS window takes
     * the fixed-origin form with two windows in flight (csrc/fused.hip: compose3_near_kernel); 0: the hint is ignored.
     * Same bits */
    int32_t compose_near;
} lago_tuning;
/* the settings in force / the library's defaults: fills t->struct_size bytes (struct_size set by the caller) */
void lago_get_tuning(lago_tuning *t);
void lago_default_tuning(lago_tuning *t);
/* applies the first t->struct_size bytes (fields beyond them keep their values); LAGO_ERR_INVALID for a null pointer or
 * a struct_size that is not a whole number of fields */
int lago_set_tuning(const lago_tuning *t);
/* Which implementation calls were dispatched to: number of launches so far in this process per path (telemetry; the
 * tests use it to make sure a case meant to exercise a fast path really runs it).  -1 for an unknown id. */
#define LAGO_PATH_GATHER_WINDOW 0  /* compose through the LDS window */
#define LAGO_PATH_STENCIL_TILE 1   /* Ad_star row-tile kernel */
#define LAGO_PATH_VECTOR_GATHER 2  /* slab-unrolled 3D gather kernels (interp_forward, compose, Ad_star) */
#define LAGO_PATH_SPLAT_SHEAR 3    /* sheared-window splat */
#define LAGO_PATH_SPLAT_SHEAR_MC 4 /* its geometry-once multi-channel form */
#define LAGO_PATH_SPLAT_TILED 5    /* tiled LDS splat */
#define LAGO_PATH_SPLAT_GLOBAL 6   /* global-atomics splat (the reference's form) */
#define LAGO_PATH_FLUID_LDS 7      /* lago_fluid_metric: three hand-written FFT passes */
#define LAGO_PATH_FLUID_2D 8       /* lago_fluid_metric: one fused 2D kernel */
#define LAGO_PATH_FLUID_XPASS 9    /* lago_fluid_metric: rocFFT (y, z) plan + fused x pass */
#define LAGO_PATH_FLUID_ROCFFT 10  /* lago_fluid_metric: rocFFT plan + operator kernel */
#define LAGO_PATH_SPLAT_2D 11      /* LDS-privatised 2D splat (interp_backward of 2D fields) */
#define LAGO_PATH_SPLAT_AFFINE_BOX 12 /* affine_interp_backward's image splat by target boxes */
#define LAGO_PATH_FLUID_GENERIC 13 /* lago_fluid_metric: generic hand-written FFT passes (any extent, both precisions) */
#define LAGO_PATH_GATHER_WINDOW_NEAR 14 /* compose with the near-identity hint: fixed-origin LDS windows, two in flight */
long long lago_path_launches(int path);
/* Launch direction (lago_tuning.launch_order): launches so far that walked their workgroups in DESCENDING order.  Kernels
 * whose results do not depend on the block order alternate (a consumer starts on what the Infinity Cache still holds of
 * its producer's output); every launch that feeds a scatter-add (interp_backward, interp_hessian_diagonal_image,
 * affine_interp_backward, regrid_backward) walks ascending and leaves the alternation alone, so that the arrival order
 * of its float atomics -- the last bits of d_I, d_A, d_T -- never depends on the calls made before it.  Telemetry for
 * tests/test_gpu_dispatch.py::test_scatter_direction_is_history_free. */
long long lago_reversed_launches(void);


#define LAGO_DECLARE(REAL, SUF)                                                                                      \
    /* interp_forward (extension.cpp:135-143 -> cuda/interp.cu:80-130):                                           \
     * out[n,c,x] = lerp(I[n or 0,c], x + dt*u[n,:,x]), clamp boundary.                                             \
     * I: (broadcast_I ? 1 : nn, nc, sp)  u: (nn, dim, sp)  out: (nn, nc, sp) */                                    \
    int lago_interp_forward##SUF(REAL *out, const REAL *I, const REAL *u, double dt, int dim, int64_t nn,           \
                                 int64_t nc, int64_t nx, int64_t ny, int64_t nz, int broadcast_I, void *stream);    \
    /* interp_backward (extension.cpp:145-156 -> cuda/interp.cu:246-313): d_I like I (splat of grad_out),           \
     * d_u like u.  Both are always produced; a gradient that is not needed is all zeros, as in the reference. */   \
    int lago_interp_backward##SUF(REAL *d_I, REAL *d_u, const REAL *grad_out, const REAL *I, const REAL *u,         \
                                  double dt, int dim, int64_t nn, int64_t nc, int64_t nx, int64_t ny, int64_t nz,   \
                                  int broadcast_I, int need_I, int need_u, void *stream);                           \
    /* interp_hessian_diagonal_image (cuda/interp.cu:351-381), 2D only.  out like I: (nI, nc, nx, ny);              \
     * as in the reference every (n, c) accumulates into plane 0 of out. */                                         \
    int lago_interp_hessian_diagonal_image##SUF(REAL *out, const REAL *u, double dt, int64_t nI, int64_t nn,        \
                                                int64_t nc, int64_t nx, int64_t ny, void *stream);                  \
    /* jacobian_times_vectorfield_forward (cuda/diff.cu:129-185).  v: (nn, nc, sp) is differentiated,               \
     * w: (nn, dim, sp) is contracted; out like v.  displacement/transpose require nc == dim. */                    \
    int lago_jtv_forward##SUF(REAL *out, const REAL *v, const REAL *w, int displacement, int transpose, int dim,    \
                              int64_t nn, int64_t nc, int64_t nx, int64_t ny, int64_t nz, void *stream);            \
    /* jacobian_times_vectorfield_backward (cuda/diff.cu:475-540): d_v like v, d_w like w, both always. */          \
    int lago_jtv_backward##SUF(REAL *d_v, REAL *d_w, const REAL *grad_out, const REAL *v, const REAL *w,            \
                               int displacement, int transpose, int dim, int64_t nn, int64_t nc, int64_t nx,        \
                               int64_t ny, int64_t nz, void *stream);                                               \
    /* jacobian_times_vectorfield_adjoint_forward (cuda/diff.cu:634-672): out[c] = sum_d D_d^T (w_d z_c).           \
     * z: (nn, nc, sp), w: (nn, dim, sp), out like z. */                                                            \
    int lago_jtv_adjoint_forward##SUF(REAL *out, const REAL *z, const REAL *w, int dim, int64_t nn, int64_t nc,     \
                                      int64_t nx, int64_t ny, int64_t nz, void *stream);                            \
    /* jacobian_times_vectorfield_adjoint_backward (cuda/diff.cu:783-835), nc == dim. */                            \
    int lago_jtv_adjoint_backward##SUF(REAL *d_v, REAL *d_w, const REAL *grad_out, const REAL *v, const REAL *w,    \
                                       int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz, void *stream);      \
    /* fluid_operator (extension.cpp:158-173 -> cuda/metric.cu:308-355): in place on the interleaved-complex        \
     * rFFT buffer Fm of shape (nn, dim, nx, ny[, nz], 2) where the last spatial extent is the half-spectrum        \
     * length; cos/sin LUTs have nx, ny, nz entries (cosZ/sinZ unused for dim == 2). */                             \
    int lago_fluid_operator##SUF(REAL *Fm, int inverse, const REAL *cosX, const REAL *sinX, const REAL *cosY,       \
                                 const REAL *sinY, const REAL *cosZ, const REAL *sinZ, double alpha, double beta,   \
                                 double gamma, int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz,             \
                                 void *stream);                                                                     \
    /* affine_interp_forward (extension.cpp:109-118 -> cuda/affine.cu:114-169).                                     \
     * I: (broadcast_I ? 1 : nn, nc, sp)  A: (nn, dim, dim)  T: (nn, dim)  out: (nn, nc, sp) */                     \
    int lago_affine_interp_forward##SUF(REAL *out, const REAL *I, const REAL *A, const REAL *T, int dim,            \
                                        int64_t nn, int64_t nc, int64_t nx, int64_t ny, int64_t nz,                 \
                                        int broadcast_I, void *stream);                                             \
    /* affine_interp_backward (extension.cpp:120-133 -> cuda/affine.cu:538-610).  Outputs that are not needed       \
     * may be NULL (the reference returns size-0 tensors for them). */                                              \
    int lago_affine_interp_backward##SUF(REAL *d_I, REAL *d_A, REAL *d_T, const REAL *grad_out, const REAL *I,      \
                                         const REAL *A, const REAL *T, int dim, int64_t nn, int64_t nc,             \
                                         int64_t nx, int64_t ny, int64_t nz, int broadcast_I, int need_I,           \
                                         int need_A, int need_T, void *stream);                                     \
    /* regrid_forward (cuda/affine.cu:683-734): resample I (nn, nc, nx, ny, nz) onto an (Nx, Ny, Nz) grid with      \
     * the given origin/spacing (length-dim host arrays of doubles). */                                             \
    int lago_regrid_forward##SUF(REAL *out, const REAL *I, int dim, int64_t nn, int64_t nc, int64_t nx,             \
                                 int64_t ny, int64_t nz, int64_t Nx, int64_t Ny, int64_t Nz, const double *origin,  \
                                 const double *spacing, void *stream);                                              \
    /* regrid_backward (cuda/affine.cu:802-855): splat grad_out (nn, nc, Nx, Ny, Nz) back onto (nx, ny, nz). */     \
    int lago_regrid_backward##SUF(REAL *d_I, const REAL *grad_out, int dim, int64_t nn, int64_t nc, int64_t nx,     \
                                  int64_t ny, int64_t nz, int64_t Nx, int64_t Ny, int64_t Nz,                       \
                                  const double *origin, const double *spacing, void *stream);                       \
    /* the same operator applied axis by axis in gather form (positive spacings): no atomics, d_I need not be       \
     * initialised, results independent of the launch; only the association of the weight products differs from     \
     * the reference's (wz (wy (wx m)) against wx wy wz m).  ws: two temporaries of ws_elems / 2 elements each,     \
     * ws_elems >= 2 nn nc max(nx Ny Nz, nx ny Nz) (3D; 2D: >= 2 nn nc nx Ny with (nx, ny) the 2D extents; may be   \
     * null when ws_elems == 0 suffices).  Inputs the passes do not cover (a non-positive spacing, spacings        \
     * >= 1e6 or so small that rounding moves a sample by more than 64 output cells, |origin| >= 1e9, 2^31 elements  \
     * or more in a pass) are served by lago_regrid_backward: every call the reference accepts is accepted.          \
     * Not in the reference's extension surface. */                                                                 \
    int lago_regrid_backward_sep##SUF(REAL *d_I, const REAL *grad_out, REAL *ws, int64_t ws_elems, int dim,         \
                                      int64_t nn, int64_t nc, int64_t nx, int64_t ny, int64_t nz, int64_t Nx,       \
                                      int64_t Ny, int64_t Nz, const double *origin, const double *spacing,          \
                                      void *stream);                                                                \
    /* jacobian_determinant: out = det J, J[c][a] = D_a u_c (+ 1 when displacement and a == c) with the clamped     \
     * central difference of lago_jtv_forward (a one-sided half difference at the borders, zero along an axis of    \
     * extent 1; the 1 is added to the rounded difference).  u: (nn, dim, sp), out: (nn, 1, sp).  Every product and \
     * sum is rounded on its own, in this order:                                                                    \
     *   2D: J00*J11 - J01*J10                                                                                      \
     *   3D: (J00*(J11*J22 - J12*J21) - J01*(J10*J22 - J12*J20)) + J02*(J10*J21 - J11*J20)                          \
     * No counterpart in the reference. */                                                                          \
    int lago_jacdet_forward##SUF(REAL *out, const REAL *u, int displacement, int dim, int64_t nn, int64_t nx,       \
                                 int64_t ny, int64_t nz, void *stream);                                             \
    /* its gradient: d_u[c] = sum_a D_a^T (grad_out * C[c][a]), C[c][a] = d det / d J[c][a] the cofactor matrix     \
     * and D_a^T the adjoint stencil of lago_jtv_adjoint_forward.  grad_out: (nn, 1, sp), d_u like u.  One gather   \
     * pass without atomics: every element of d_u is written once, identically from run to run.  No counterpart in  \
     * the reference. */                                                                                            \
    int lago_jacdet_backward##SUF(REAL *d_u, const REAL *grad_out, const REAL *u, int displacement, int dim,        \
                                  int64_t nn, int64_t nx, int64_t ny, int64_t nz, void *stream);                    \
    /* invert_displacement: `iters` steps of the fixed-point iteration for the inverse of x -> x + u(x),            \
     *   v_0 = -u,  v_{k+1}(x) = -u(x + v_k(x))                                                                     \
     * (multilinear interpolation of u with the clamped border of lago_interp_forward), all steps in one kernel:     \
     * v stays in registers and is written once.  u, out: (nn, dim, sp).  Bit for bit the value of                  \
     *   v = -u; repeat iters times: v = -lago_interp_forward(I = u, u = v, dt = 1)                                 \
     * The only early stop: a wavefront whose step changed no bit of v ends its loop (later steps would reproduce   \
     * the same bits).  The iteration converges where the interpolated u is a contraction (Lipschitz constant < 1). \
     * LAGO_ERR_INVALID for iters < 0, dim not in {2, 3} and out overlapping u; nn == 0 does nothing.  No            \
     * counterpart in the reference. */                                                                             \
    int lago_invert_disp_forward##SUF(REAL *out, const REAL *u, int iters, int dim, int64_t nn, int64_t nx,         \
                                      int64_t ny, int64_t nz, void *stream);                                        \
    /* the adjoint solve of the CONVERGED inverse (not of the truncated iteration): with psi = id + v and            \
     * G[c][a] = (d_a u_c)(psi(x)) (the gradient of the interpolant, as lago_interp_backward's d_u forms it),        \
     * M = I + G (the 1 added to the rounded gradient), lam = -(M^-T) grad_out by the adjugate.  d_u of the inverse  \
     * is the splat of lam at psi: lago_interp_backward(d_I, ., grad_out = lam, I = u, u = v, dt = 1, need_I).       \
     * grad_out, u, v, lam: (nn, dim, sp).  Every product, sum and quotient is rounded on its own, in this order:    \
     *   2D: det = M00*M11 - M01*M10                                                                                \
     *       lam0 = -((M11*g0 - M10*g1) / det)   lam1 = -((M00*g1 - M01*g0) / det)                                  \
     *   3D: det = (M00*(M11*M22 - M12*M21) - M01*(M10*M22 - M12*M20)) + M02*(M10*M21 - M11*M20)                    \
     *       C[c][a] = M[c+1][a+1]*M[c+2][a+2] - M[c+1][a+2]*M[c+2][a+1]   (indices mod 3)                          \
     *       lam_c = -(((C[c][0]*g0 + C[c][1]*g1) + C[c][2]*g2) / det)                                              \
     * det is not guarded: where the deformation folds (det M <= 0 or tiny) the IEEE result stands.  One gather     \
     * pass, no atomics, nothing cleared: identical from call to call.  lam must not overlap an input. */           \
    int lago_invert_disp_adjoint##SUF(REAL *lam, const REAL *grad_out, const REAL *u, const REAL *v, int dim,       \
                                      int64_t nn, int64_t nx, int64_t ny, int64_t nz, void *stream);                \
    /* gaussian_smooth: out = alpha * G_z G_y G_x in (+ out when accumulate), separable Gaussian filtering of       \
     * `rows` = N*C scalar fields of extent (nx, ny[, nz]).  G_a is the 1-D correlation with the 2 r + 1 symmetric  \
     * taps of axis a, r = radii[a] in 0..LAGO_GAUSS_MAX_RADIUS (0: the axis is left alone); taps holds             \
     * LAGO_GAUSS_MAX_RADIUS + 1 doubles per axis, axis a's w_0 .. w_r at taps[a * (LAGO_GAUSS_MAX_RADIUS + 1)],    \
     * rounded once to REAL.  radii and taps are HOST arrays of `dim` entries / blocks, read during the call and    \
     * passed to the kernels by value (nothing of them is read later: the call may be captured in a graph).        \
     * mode LAGO_GAUSS_WRAP: indices modulo the extent, however large r is relative to it; LAGO_GAUSS_ZERO:         \
     * samples outside the grid are 0.  Both are self-adjoint.  One launch per axis with r > 0 (one copy launch     \
     * when every r is 0), outermost axis first (of three, one that may run in place is taken second, with and      \
     * without accumulate); the last one applies alpha and the accumulation.  scratch: one                         \
     * tensor like in, needed when two or more axes have r > 0 (else may be NULL), clobbered.  in is not modified;  \
     * out and scratch may not overlap in or each other.  No atomics: the same bits from call to call.  With       \
     * accumulate and three passes the middle pass runs in place on scratch, which needs one axis that a workgroup  \
     * stages whole (nz <= 1024, or nx or ny <= 64 (float) / 32 (double)): LAGO_ERR_INVALID otherwise.  An inf or    \
     * NaN of `in` reaches outputs up to (r rounded up to 4) + 3 positions away along a filtered axis (zero padding  \
     * taps are multiplied too); the all-zero-radii copy is exact.  No counterpart in the reference. */                                                                             \
    int lago_gauss_smooth##SUF(REAL *out, const REAL *in, REAL *scratch, const int *radii, const double *taps,      \
                               int mode, double alpha, int accumulate, int dim, int64_t rows, int64_t nx,           \
                               int64_t ny, int64_t nz, void *stream);                                               \
    /* lncc (no counterpart in the reference): Gaussian-windowed local normalised cross-correlation of two fields   \
     * I, J of `rows` = N*C scalar fields of extent (nx, ny[, nz]), in four stages that the caller chains.  With G  \
     * the operator of lago_gauss_smooth (same radii, taps and border modes):                                       \
     *       A = G I, B = G J, C = G(I I), D = G(I J), E = G(J J)                                                   \
     *       sI = C - A^2, sJ = E - B^2, sX = D - A B, cc = sX^2 / (sI sJ + eps)             (nothing is clamped)   \
     * lago_lncc_moments: out (5, rows, *sp) = (A, B, C, D, E).  One kernel along the last axis always runs (at     \
     * radius 0 it only forms the products): it reads I and J once, forms the products in double (exact for float)  \
     * and writes the five rows; the other axes with r > 0 then run the pass kernels of lago_gauss_smooth over the  \
     * 5 rows stacked fields, first axis first.  Every stored intermediate is rounded to REAL.  radii / taps: as for\
     * lago_gauss_smooth, HOST arrays read during the call and passed to the kernels by value (the call may be      \
     * captured in a graph).  scratch: one tensor like out, needed when an axis besides the last has r > 0 (else may\
     * be NULL), clobbered.  out and scratch may not overlap I, J or each other; I may equal J.  No atomics: the    \
     * same bits from call to call.  No counterpart in the reference. */                                            \
    int lago_lncc_moments##SUF(REAL *out, const REAL *I, const REAL *J, REAL *scratch, const int *radii,            \
                               const double *taps, int mode, int dim, int64_t rows, int64_t nx, int64_t ny,         \
                               int64_t nz, void *stream);                                                           \
    /* lago_lncc_cc: cc (n) from the moments (5, n), n = rows * voxels; pointwise, arithmetic in double for both    \
     * precisions, rounded once.  eps >= 0.  cc may not overlap the moments.  No counterpart in the reference. */   \
    int lago_lncc_cc##SUF(REAL *cc, const REAL *moments, double eps, int64_t n, void *stream);                      \
    /* lago_lncc_coeffs: the fields under the G's of the backward for an upstream gradient g (n) on cc.  With       \
     * den = sI sJ + eps, cX = 2 sX / den, cI = -sX^2 sJ / den^2, cJ = -sX^2 sI / den^2:                            \
     *       dI = G[g (-2 A cI - B cX)] + 2 I G[g cI] + J G[g cX]                                                   \
     *       dJ = G[g (-2 B cJ - A cX)] + 2 J G[g cJ] + I G[g cX]                                                   \
     * which = 1: coef (3, n) = (g (-2 A cI - B cX), g cI, g cX); which = 2: (g (-2 B cJ - A cX), g cJ, g cX);      \
     * which = 3: (5, n) = the three of dI, then g (-2 B cJ - A cX), g cJ.  The layout is that of `k rows` stacked  \
     * fields: ONE lago_gauss_smooth call with rows = k * rows filters them.  Pointwise, in double, rounded once;   \
     * coef may not overlap an input.  No counterpart in the reference. */                                          \
    int lago_lncc_coeffs##SUF(REAL *coef, const REAL *moments, const REAL *g, double eps, int which, int64_t n,     \
                              void *stream);                                                                        \
    /* lago_lncc_combine: dI and / or dJ (n each; the one `which` does not name may be NULL) from `smoothed`, the   \
     * filtered output of lago_lncc_coeffs with the same `which`, and I, J: S0 + 2 I S1 + J S2 (and the same with   \
     * J's fields and the shared G[g cX]).  Pointwise, in double, rounded once; an output may not overlap an input  \
     * or the other output.  No counterpart in the reference. */                                                    \
    int lago_lncc_combine##SUF(REAL *dI, REAL *dJ, const REAL *smoothed, const REAL *I, const REAL *J, int which,   \
                               int64_t n, void *stream);                                                            \
    /* mutual information (no counterpart in the reference): the Parzen-window joint histogram of two fields I, J   \
     * of `rows` = N*C scalar fields of extent (nx, ny[, nz]), one bins x bins table P per row, bins = B in         \
     * LAGO_MI_MIN_BINS..LAGO_MI_MAX_BINS.  Each image has a range (lo, hi), lo < hi, both finite, passed by value  \
     * (the call may be captured in a graph).  Per voxel, in double for both precisions and in this order (nothing  \
     * is fused):                                                                                                   \
     *       s = (B - 3) / (hi - lo)    vc = fmin(fmax(v, lo), hi)   (a NaN voxel counts as lo)                      \
     *       c = (vc - lo) * s + 1      k = min(floor(c), B - 3) - 1, clamped as an integer to [0, B - 4]            \
     *       t = c - (k + 1), u = 1 - t                                                                             \
     *       w0 = u u u / 6   w1 = ((3 t - 6) t t + 4) / 6   w2 = (((-3 t + 3) t + 3) t + 1) / 6   w3 = t t t / 6      \
     * (cubic B-spline windows on both images: a voxel touches bins kI..kI+3 x kJ..kJ+3), and                       \
     *       H[kI + a][kJ + b] += llrint(wI_a * wJ_b * 2^32)   as a signed 64-bit integer sum                       \
     *       P = H / ((double)nvox * 2^32)                     nvox the voxels of one row, 2^30 at most             \
     * The integer sum is associative: P has the same bits from call to call, on any stream and for any number of   \
     * scratch tables, and equals a sequential evaluation integer for integer.  scratch: `scratch_tables` >= 1      \
     * tables of bins x bins 64-bit integers PER ROW, (rows, scratch_tables, B, B), clobbered (workgroups write      \
     * partial tables there with plain stores and a second kernel sums them: no memset, no global atomic);          \
     * lago_mi_scratch_tables says how many the call can use, fewer only cost speed.  P and scratch may not overlap \
     * an input or each other; I may equal J.  LAGO_ERR_INVALID: bins out of range, lo >= hi or a bound that is not \
     * finite (or a range so wide or narrow that s is not), more than 2^30 voxels in a row, dim not 2 or 3.         \
     * rows == 0 or an extent of 0: nothing is done (LAGO_OK).  No counterpart in the reference. */                 \
    int lago_mi_histogram##SUF(double *P, const REAL *I, const REAL *J, long long *scratch, int64_t scratch_tables, \
                               int bins, double loI, double hiI, double loJ, double hiJ, int dim, int64_t rows,     \
                               int64_t nx, int64_t ny, int64_t nz, void *stream);                                   \
    /* lago_mi_backward: for G = dL/dP (rows, B, B) and the windows' derivatives                                    \
     *       w0' = -(u u) / 2 s   w1' = (3 t - 4) t / 2 s   w2' = ((-3 t + 2) t + 1) / 2 s   w3' = t t / 2 s         \
     * (all four 0 unless lo <= v <= hi: 0 for NaN, +-inf and clamped voxels)                                       \
     *       dI(x) = (sum_a wI_a'(I(x)) (sum_b wJ_b(J(x)) G[kI + a][kJ + b])) / nvox        a, b ascending          \
     *       dJ(x) = (sum_b wJ_b'(J(x)) (sum_a wI_a(I(x)) G[kI + a][kJ + b])) / nvox                                \
     * in double, rounded once to REAL: the gradient of the unquantised histogram.  The two are one function with   \
     * the roles swapped and G transposed, bit for bit.  dI or dJ may be NULL: that gradient is neither computed    \
     * nor written.  A pure gather: the same bits from call to call.  An output may not overlap an input or the     \
     * other output.  Errors and empty extents as for lago_mi_histogram.  No counterpart in the reference. */       \
    int lago_mi_backward##SUF(REAL *dI, REAL *dJ, const double *G, const REAL *I, const REAL *J, int bins,          \
                              double loI, double hiI, double loJ, double hiJ, int dim, int64_t rows, int64_t nx,    \
                              int64_t ny, int64_t nz, void *stream);                                                \
    /* lago_warp_labels: out(x) = the label of L at x + dt u(x).  L: (broadcast ? 1 : nn, 1, sp) int32 label VALUES \
     * (any bit pattern), u: (nn, dim, sp), out: (nn, 1, sp) int32.  Per axis with extent n and voxel index i:      \
     *       p = i + dt u in REAL, the position lago_interp_forward samples at, bit for bit                         \
     *       p = fmin(fmax(p, -1), n)   (out of range, infinite and saturated positions fall on the border voxel,   \
     *                                   a NaN on the first voxel of the axis; no in-range position changes)        \
     *       f = floor(p), t = p - f    (in REAL, then widened to double)                                           \
     *       corners clamp(f, 0, n - 1) and clamp(f + 1, 0, n - 1)                                                  \
     * LAGO_LABELS_NEAREST: per axis the upper corner where t > 0.5, else the lower (a tie goes to the lower).      \
     * LAGO_LABELS_VOTE: the 2^dim corners, first axis slowest, weigh w_q = (a_x a_y) a_z in double (a = 1 - t for  \
     * the lower corner, t for the upper; a_y a_z in 2D); a label's score is the sum of w_q over the corners that   \
     * carry it, q ascending from 0.0 (clamped corners that coincide each add); the largest score wins, among equal \
     * scores the smallest label value.  Nothing is fused; no atomic: the same bits from call to call.              \
     * LAGO_ERR_INVALID: a mode or dim that is none of the above, out overlapping an input.  Empty extents do       \
     * nothing (LAGO_OK).  No counterpart in the reference. */                                                      \
    int lago_warp_labels##SUF(int32_t *out, const int32_t *L, const REAL *u, double dt, int mode, int broadcast,    \
                              int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz, void *stream);            \
    /* lago_interp_points: a field sampled at a list of positions.  out[n,c,p] = lerp(F[n or 0,c], x[n,:,p]).       \
     * F: (broadcast_F ? 1 : nn, nc, sp)  x: (nn, dim, np), channel-first, in voxel-index units along the spatial   \
     * axes in order (a field (nn, dim, sp) viewed as (nn, dim, nvox) is a point set)  out: (nn, nc, np).  The      \
     * arithmetic is lago_interp_forward's at the same position, expression for expression and bit for bit:        \
     * f = floor(x) saturated to +-2^30, t = x - f, corners clamp(f, 0, n - 1) and clamp(f + 1, 0, n - 1), the same \
     * fma nesting.  So a position outside the grid reads the clamped border, the domain is |x| < 2^30, and a       \
     * coordinate that is not finite gives NaN for that point and never an access outside F (every corner index is \
     * clamped before it is used).  One gather pass, no atomics: the same bits from call to call.                  \
     * LAGO_ERR_INVALID before any device call: dim not 2 or 3, a negative extent, a channel plane of 2^32 bytes or \
     * more, np >= 2^31, nn > 65535, out overlapping an input.  nn, nc, np or an extent equal to 0: nothing is done \
     * (LAGO_OK).  No counterpart in the reference. */                                                              \
    int lago_interp_points##SUF(REAL *out, const REAL *F, const REAL *x, int dim, int64_t nn, int64_t nc,           \
                                int64_t np, int64_t nx, int64_t ny, int64_t nz, int broadcast_F, void *stream);     \
    /* its gradients for an upstream grad_out (nn, nc, np).  Either output may be NULL when it is not needed        \
     * (need_F / need_x 0): it is then neither computed nor written.                                                \
     *   d_x (nn, dim, np): d_x[n,a,p] = sum_c grad_out[n,c,p] dF_c/dx_a, the position gradient of the multilinear  \
     *     value on the fetched corners as lago_interp_backward's d_u forms it, c ascending: the c = 0 product, then \
     *     one fma per channel.  The one-sided derivative of the cell floor(x); zero along an axis on which both    \
     *     clamped corners coincide.  Plain stores, no atomic: the same bits from call to call.                     \
     *   d_F like F (summed over the items when broadcast_F): zeroed on the stream, then every point adds w_q g to  \
     *     its 2^dim clamped corners, w_q = (a_x a_y) a_z in REAL (a = 1 - t for the lower corner, t for the upper; \
     *     a_y a_z for dim 2), the product w_q g rounded once.  The adds are hardware float atomics on memory: the  \
     *     LAST BITS of d_F depend on their arrival order and differ from call to call, as lago_interp_backward's   \
     *     d_I.  Cells that receive nothing hold exactly 0.                                                         \
     * Errors and empty problems as for lago_interp_points (with np == 0 a wanted d_F is zeroed); an output may not \
     * overlap an input or the other output.  No counterpart in the reference. */                                   \
    int lago_interp_points_backward##SUF(REAL *d_F, REAL *d_x, const REAL *grad_out, const REAL *F, const REAL *x,  \
                                         int dim, int64_t nn, int64_t nc, int64_t np, int64_t nx, int64_t ny,       \
                                         int64_t nz, int broadcast_F, int need_F, int need_x, void *stream);         \
    /* lago_bspline_prefilter: samples -> cubic B-spline coefficients.  in, out: (rows, sp), rows = batch items      \
     * times channels.  Per spatial axis of extent n > 1, axes in order, c solves B c = f with B the (1, 4, 1) / 6    \
     * tridiagonal under a whole-sample mirror of period 2n - 2 (first row (4, 2) / 6, last row (2, 4) / 6): pole    \
     * z = sqrt(3) - 2, gain 6, c+[0] = sum_k z^k 6 f[mirror k] / (1 - z^(2n-2)) (cut where |z|^k is below half an   \
     * ulp), c+[i] = 6 f[i] + z c+[i-1], c[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]), c[i] = z (c[i+1] - c+[i]).    \
     * adjoint != 0: B^T instead of B (= D B D^-1, D = diag(1/2, 1, ..., 1, 1/2): the end samples of every line      \
     * doubled before its pass and halved after it; the same for n <= 2).  One launch per axis, the first from in    \
     * to out and the others in place on out; lines up to 256 samples are staged in LDS, longer ones run in place    \
     * through global memory.  8 bytes per element and pass (float32), no atomics: the same bits from call to call.  \
     * LAGO_ERR_INVALID before any device call: dim not 2 or 3, a negative extent, a plane of 2^29 elements or more, \
     * out overlapping in, a null pointer.  rows or an extent equal to 0: nothing is done (LAGO_OK).  No counterpart \
     * in the reference. */                                                                                          \
    int lago_bspline_prefilter##SUF(REAL *out, const REAL *in, int adjoint, int dim, int64_t rows, int64_t nx,        \
                                    int64_t ny, int64_t nz, void *stream);                                           \
    /* lago_interp_bspline: the cubic B-spline with coefficients C evaluated at i + dt u(i) for every voxel i.       \
     * C: (broadcast_C ? 1 : nn, nc, sp)  u: (nn, dim, sp)  out: (nn, nc, sp).  Per axis with extent n: the position \
     * (lago_interp_forward's expression) is clamped to [0, n - 1] first, f = min(floor(x), n - 2), t = x - f, the   \
     * taps f - 1 ... f + 2 weigh ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6 and are folded once     \
     * into the grid (k -> |k|, then k -> 2 (n - 1) - k if k > n - 1; n = 1: index 0): csrc/bspline_weights.hpp.     \
     * 4^dim taps per voxel and channel (64 gathered elements for dim 3), 4 (dim + 2 nc) streamed bytes per voxel    \
     * (float32), summed z innermost, then y, then x: the same bits from call to call.  A position outside the grid  \
     * gives the value at the nearest point of the grid's box, a NaN coordinate gives NaN for that voxel, and no     \
     * position addresses outside C.  LAGO_ERR_INVALID before any device call: dim not 2 or 3, a negative extent, a  \
     * plane of 2^29 elements or more, out overlapping an input, a null pointer.  nn, nc or an extent equal to 0:    \
     * nothing is done (LAGO_OK).  No counterpart in the reference. */                                               \
    int lago_interp_bspline##SUF(REAL *out, const REAL *C, const REAL *u, double dt, int dim, int64_t nn, int64_t nc, \
                                 int64_t nx, int64_t ny, int64_t nz, int broadcast_C, void *stream);                 \
    /* its gradients for an upstream grad_out (nn, nc, sp).  Either output may be NULL when it is not needed         \
     * (need_C / need_u 0): it is then neither computed nor written.                                                 \
     *   d_u (nn, dim, sp): d_u[n,a,i] = dt sum_c grad_out[n,c,i] dS_c/dx_a with the derivative weights              \
     *     (-(1-t)^2, 3t^2 - 4t, -3t^2 + 2t + 1, t^2) / 2 along a; exactly 0 along an axis on which the position     \
     *     was clamped (continuous there: the mirror makes the derivative vanish at both borders); NaN in every      \
     *     component for a voxel with a NaN coordinate.  Plain stores: the same bits from call to call.              \
     *   d_C like C (summed over the items when broadcast_C): zeroed on the stream, then every voxel adds w g to     \
     *     its 4^dim folded taps, w = (w_x w_y) w_z in REAL (w_y w_z for dim 2), the product w g rounded once; a     \
     *     voxel with a NaN coordinate adds nothing.  The adds are hardware float atomics on memory: the LAST BITS   \
     *     of d_C depend on their arrival order and differ from call to call, as lago_interp_backward's d_I.  Cells  \
     *     that receive nothing hold exactly 0.                                                                      \
     * An output may not overlap an input or the other output.  No counterpart in the reference. */                  \
    int lago_interp_bspline_backward##SUF(REAL *d_C, REAL *d_u, const REAL *grad_out, const REAL *C, const REAL *u,   \
                                          double dt, int dim, int64_t nn, int64_t nc, int64_t nx, int64_t ny,        \
                                          int64_t nz, int broadcast_C, int need_C, int need_u, void *stream);       \
    /* lago_ffd_expand: a free-form deformation's control lattice expanded to a dense field by its uniform cubic     \
     * B-spline.  ctrl: (rows, mx, my[, mz])  out: (rows, nx, ny[, nz]), rows = batch items times channels, sx, sy   \
     * [, sz] the integer control spacing per axis in voxels, each in 1..32 (dim 2: nz and sz are ignored).  Per     \
     * axis with extent n and spacing s: m = (n - 1) / s + 4 control points, point j at voxel (j - 1) s; voxel x has \
     * the taps i ... i + 3, i = x / s, weighed ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6 at        \
     * t = (REAL)(x % s) / (REAL)s (csrc/ffd_weights.hpp: the expressions of bspline_weights.hpp, no fma); every tap \
     * is inside the lattice, nothing is folded or clamped.  out[r,x,y,z] = sum_c Wz[z,c] (sum_b Wy[y,b] (sum_a      \
     * Wx[x,a] ctrl[r,a,b,c])): the axes contracted one after the other in LDS, x first, each 4-tap sum as the tap-0  \
     * product and one fma per further tap, ascending.  4 bytes stored per element (float32), the lattice read from  \
     * cache; no atomics: the same bits from call to call.  LAGO_ERR_INVALID before any device call: dim not 2 or 3, \
     * a negative extent, a spacing outside 1..32, a plane of 2^29 elements or more, a null pointer, out overlapping \
     * ctrl.  rows or an extent equal to 0: nothing is done (LAGO_OK).  No counterpart in the reference. */          \
    int lago_ffd_expand##SUF(REAL *out, const REAL *ctrl, int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz, \
                             int sx, int sy, int sz, void *stream);                                                  \
    /* its adjoint: d_ctrl[r,a,b,c] = sum_{x,y,z} Wx[x,a] Wy[y,b] Wz[z,c] grad_out[r,x,y,z], the same weights.       \
     * grad_out: (rows, nx, ny[, nz])  d_ctrl: (rows, mx, my[, mz]).  Workgroups own voxel tiles of 8 x 8 x 64       \
     * (dim 2: 64 x 64), read them once and reduce them in LDS, z first, then y, then x: per control point the taps  \
     * q = 0..3 in order, the voxels of a cell ascending, acc = fma(w, v, acc) from 0.  The partial sums of a tile   \
     * go to `scratch` with plain stores (lago_ffd_scratch_elems elements of REAL, need not be initialised,          \
     * clobbered) and a second kernel adds, per control point, the partials of the tiles that reach it, tiles        \
     * ascending.  4 bytes loaded per element (float32) plus the partials; no atomic on memory: the same bits from   \
     * call to call, and a control point that no voxel reaches, or only with weight 0, holds exactly 0.              \
     * LAGO_ERR_INVALID before any device call: as lago_ffd_expand, and scratch_elems too small, d_ctrl overlapping  \
     * grad_out or scratch, scratch overlapping grad_out.  rows or an extent equal to 0: nothing is done (LAGO_OK;   \
     * d_ctrl is not written).  No counterpart in the reference. */                                                  \
    int lago_ffd_expand_adjoint##SUF(REAL *d_ctrl, const REAL *grad_out, REAL *scratch, int64_t scratch_elems,       \
                                     int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz, int sx, int sy,      \
                                     int sz, void *stream);                                                          \
    /* lago_field_energy: the smoothness energy of a field, per batch item.  u: (nn, nc, nx, ny[, nz]), nc free      \
     * (dim channels for a displacement, 1 for a bias field); energy: (nn); spacing: dim doubles h_a > 0, one per    \
     * axis (host memory, read during the call).  V = the voxels of one item (not times nc); per item, summed over   \
     * the channels k:                                                                                               \
     *   LAGO_ENERGY_DIFFUSION  E = (1/V) sum_x sum_k sum_a (d_a u_k(x))^2,  d_a u(x) = (u(x + e_a) - u(x)) / h_a    \
     *     where x_a + 1 < n_a and 0 otherwise (a forward difference with a Neumann border; an axis of extent 1      \
     *     contributes nothing): VoxelMorph's penalty.                                                               \
     *   LAGO_ENERGY_BENDING    E = (1/V) sum_x sum_k [ sum_a (d_aa u_k(x))^2 + 2 sum_{a<b} (d_ab u_k(x))^2 ],        \
     *     d_aa u(x) = (u(x + e_a) - 2 u(x) + u(x - e_a)) / h_a^2 where 1 <= x_a <= n_a - 2 and 0 otherwise,         \
     *     d_ab u(x) = (u(x + e_a + e_b) - u(x + e_a) - u(x + e_b) + u(x)) / (h_a h_b) where x_a + 1 < n_a and       \
     *     x_b + 1 < n_b and 0 otherwise (forward-forward, so that d_ab^T d_ab = d_aa d_bb in the interior and the   \
     *     operator there is exactly (sum_a d_aa)^2; axes of extent 1 or 2 drop their terms): Rueckert's, NiftyReg's \
     *     and elastix's penalty.                                                                                    \
     * Both are quadratic forms E = <u, A u> / V with A = sum_t w_t D_t^T D_t over the difference operators D_t      \
     * above (weights 1 and 2), symmetric positive semidefinite, and dE/du = (2/V) A u exactly, at the borders too:  \
     * lago_field_energy_operator.  Away from the borders A is -Laplacian (7-point) for diffusion and the discrete   \
     * biharmonic operator (25-point in 3D, 13-point in 2D) for bending.                                             \
     * The arithmetic of a voxel, its order (no fma) and its rounding count are csrc/energy_stencil.hpp; a float32   \
     * operator value is within K 2^-24 |scale| sum |A| |u| of the exact one, K = 13 (bending), 8 (diffusion).       \
     * Workgroups own voxel tiles of 8 x 8 x 64 (dim 2: 64 x 64) staged in LDS with their halo; every lane adds its  \
     * voxels' terms, a tile's sum (added in double, fixed order) goes to `scratch` with a plain store               \
     * (lago_field_energy_scratch_elems elements of REAL, need not be initialised, clobbered), and a second kernel   \
     * adds one item's partials in double in a fixed order and writes E[n] in REAL.  4 bytes loaded per element      \
     * (float32); no atomics: the same bits from call to call.  LAGO_ERR_INVALID before any device call: dim not 2   \
     * or 3, an unknown kind, a negative extent, a plane of 2^29 elements or more, a null pointer, a spacing that is \
     * not positive and finite, scratch_elems too small, energy or scratch overlapping u.  nn, nc or an extent equal \
     * to 0: nothing is done (LAGO_OK; energy is not written).  No counterpart in the reference. */                  \
    int lago_field_energy##SUF(REAL *energy, const REAL *u, REAL *scratch, int64_t scratch_elems, int kind, int dim,  \
                               int64_t nn, int64_t nc, int64_t nx, int64_t ny, int64_t nz, const double *spacing,     \
                               void *stream);                                                                        \
    /* out[n] = scale[n] (A u)[n] with the A of lago_field_energy: out, u (nn, nc, sp); scale (nn) in device memory, \
     * NULL for 1 (the backward of the energy passes 2 g_n / V without a host synchronisation or an extra pass).     \
     * One load and one store per element, the halo of a tile (one voxel for diffusion, two for bending) from cache; \
     * plain stores: the same bits from call to call.  LAGO_ERR_INVALID before any device call: as lago_field_energy \
     * (no scratch), and out overlapping u or scale.  Empty problems: nothing is done (LAGO_OK). */                  \
    int lago_field_energy_operator##SUF(REAL *out, const REAL *u, const REAL *scale, int kind, int dim, int64_t nn,   \
                                        int64_t nc, int64_t nx, int64_t ny, int64_t nz, const double *spacing,        \
                                        void *stream);                                                               \
    /* lago_pyramid_down: one level of an image pyramid, from the fine grid to the coarse one.  in: (rows, nx, ny    \
     * [, nz]), the FINE field, rows = batch items times channels; out: (rows, mx, my[, mz]).  Per axis with fine     \
     * extent n the coarse extent is m = (n + 1) / 2 and coarse voxel j sits at fine voxel 2 j; the extents passed   \
     * are always the fine grid's (dim 2: nz is ignored).  out = scale (Mx (x) My (x) Mz) in with, per axis, op =    \
     *   LAGO_PYRAMID_REDUCE  M = R (m x n), (R a)[j] = sum_{k=-2..2} w_k a[clamp(2 j + k, 0, n - 1)],               \
     *                        w = (1, 4, 6, 4, 1) / 16: the anti-aliased reduce, rows sum to 1;                      \
     *   LAGO_PYRAMID_EXPAND  M = E^T, the exact transpose of the expand of lago_pyramid_up (its backward).          \
     * Workgroups own fine tiles of 8 x 8 x 64 (dim 2: 64 x 64) staged in LDS with a halo of two voxels and contract \
     * the axes one after the other in LDS, the contiguous axis first (z, y, x), five taps ascending, each a product \
     * and an addition (csrc/pyramid_weights.hpp: no fma), then the scale: at most 5 dim + 1 roundings per element.  \
     * 4 bytes loaded per fine element and 4 stored per coarse one (float32); every element has one owner, no        \
     * atomics, no scratch: the same bits from call to call, and exact results for integer-valued inputs up to 512   \
     * in magnitude.  Nothing is allocated and nothing synchronises.  LAGO_ERR_INVALID before any device call: dim   \
     * not 2 or 3, a negative extent, a plane of 2^29 elements or more, an unknown op, a null pointer, out           \
     * overlapping in.  rows or an extent equal to 0: nothing is done (LAGO_OK).  No counterpart in the reference. */ \
    int lago_pyramid_down##SUF(REAL *out, const REAL *in, int op, int dim, int64_t rows, int64_t nx, int64_t ny,     \
                               int64_t nz, double scale, void *stream);                                              \
    /* lago_pyramid_up: from the coarse grid to the fine one.  in: (rows, mx, my[, mz]); out: (rows, nx, ny[, nz]),  \
     * the FINE field, whose extents are the ones passed (both n = 2 m and n = 2 m - 1 belong to a coarse extent m). \
     * out = scale (Mx (x) My (x) Mz) in with, per axis, op =                                                        \
     *   LAGO_PYRAMID_EXPAND  M = E (n x m), (E c)[2 j] = c[j], (E c)[2 j + 1] = (c[j] + c[min(j + 1, m - 1)]) / 2:   \
     *                        linear prolongation, rows sum to 1 (scale = 2 carries a displacement in voxel units    \
     *                        to the finer grid);                                                                    \
     *   LAGO_PYRAMID_REDUCE  M = R^T, the exact transpose of the reduce (its backward; 2 R^T is NOT E: it does not  \
     *                        preserve constants at the border).                                                     \
     * Workgroups own fine tiles of 8 x 8 x 64 (dim 2: 64 x 64), stage the 6 x 6 x 34 coarse voxels a tile reaches   \
     * in LDS and contract x, then y, then z, three taps ascending, each a product and an addition, then the scale.  \
     * 4 bytes stored per fine element (float32), an eighth of that loaded; one owner per element, no atomics: the   \
     * same bits from call to call.  Errors and empty problems as lago_pyramid_down. */                              \
    int lago_pyramid_up##SUF(REAL *out, const REAL *in, int op, int dim, int64_t rows, int64_t nx, int64_t ny,       \
                             int64_t nz, double scale, void *stream);

LAGO_DECLARE(float, _f32)
LAGO_DECLARE(double, _f64)

/* Elements of REAL that lago_ffd_expand_adjoint needs as scratch for this problem (the partial sums of every voxel
 * tile: rows x tiles x the control points a tile reaches); 0 for an empty problem, -1 for arguments the entry point
 * rejects.  The caller allocates.  No counterpart in the reference. */
long long lago_ffd_scratch_elems(int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz, int sx, int sy, int sz);

/* Elements of REAL that lago_field_energy needs as scratch for this problem (one partial sum per voxel tile: nn x nc x
 * tiles of a plane); 0 for an empty problem, -1 for arguments the entry point rejects.  The caller allocates.  No
 * counterpart in the reference. */
long long lago_field_energy_scratch_elems(int kind, int dim, int64_t nn, int64_t nc, int64_t nx, int64_t ny, int64_t nz);

/* How many scratch tables per row lago_mi_histogram can use for `rows` rows of `nvox` voxels at `bins` bins (>= 1: a
 * row is cut into chunks of a few thousand voxels, as many as keep the scratch of all rows within 8 MB).  The caller
 * allocates rows x this x bins x bins 64-bit integers.  No counterpart in the reference. */
int lago_mi_scratch_tables(int bins, int64_t rows, int64_t nvox);

/* label_overlap: counts (rows, K, 3) of two label maps A, B (rows, nvox) of int32 label values, K = num_labels in
 * 1..LAGO_LABELS_MAX: per row and label k in [0, K)  [#(A == k), #(B == k), #(A == k and B == k)]  as 64-bit integers.
 * A voxel whose label is outside [0, K) counts in nothing for that image.  Workgroups count chunks of a row into 32-bit
 * tables in LDS (a wave adds once for all its lanes that hold the same pair) and write them to `scratch`, rows x
 * scratch_chunks x K x 3 32-bit integers that need not be initialised; a second kernel sums the chunks.  No global
 * atomic: the same bits from call to call, for any chunking.  lago_label_overlap_scratch_chunks says how many chunks per
 * row the call can use (>= 1: chunks of about 16384 voxels, as many as keep the scratch of all rows within 8 MB, or
 * one table a row), fewer only cost speed.  counts and scratch may not overlap an input or each other; A may equal B.
 * LAGO_ERR_INVALID: num_labels out of range, more than 2^30 voxels in a row.  No counterpart in the reference. */
int lago_label_overlap(long long *counts, const int32_t *A, const int32_t *B, uint32_t *scratch, int64_t scratch_chunks,
                       int num_labels, int64_t rows, int64_t nvox, void *stream);
int lago_label_overlap_scratch_chunks(int num_labels, int64_t rows, int64_t nvox);

/* distance_transform: out[n, x] = the Euclidean distance (squared != 0: its square) from voxel x to the nearest FEATURE
 * voxel of item n, 0 on features, +inf everywhere in an item without one.  L: (nn, 1, sp) int32 label values, out:
 * (nn, 1, sp) float32.  The features (`where`):
 *   LAGO_EDT_NONZERO    L != 0
 *   LAGO_EDT_EQUAL      L == label
 *   LAGO_EDT_NOT_EQUAL  L != label
 *   LAGO_EDT_SURFACE    L == label and one of the 2 dim face neighbours != label, a neighbour outside the volume counting
 *                       as different (the mask minus its erosion by the face-connected cross, border value 0)
 * spacing: `dim` doubles ON THE HOST, one per spatial axis in order, each narrowed to float32 and positive and finite
 * there.  The squared distance is sum_a (s_a delta_a)^2.  One pass per axis, the last (contiguous) axis first, each per
 * line  out[i] = min_j g[j] + t t, t = s float(i - j)  in float32 with nothing fused (csrc/edt_line.hpp); the first pass
 * forms g (0 on a feature, +inf elsewhere) from L as it loads, the later ones run in place on out, the last takes the
 * correctly rounded square root unless `squared`.  With every spacing 1 all values are integers below 2^24, so the
 * squared distance is exact; otherwise it is within 8 * 2^-24 relative of the real value (no term is negative).  No
 * atomic, no scratch buffer: the same bits from call to call.
 * LAGO_ERR_INVALID before any device call: dim not 2 or 3, an unknown `where`, a spacing that is not positive, a negative
 * extent or one above LAGO_EDT_MAX_EXTENT, 2^31 voxels or more in all, a null pointer, out overlapping L.  nn or an
 * extent equal to 0: nothing is done (LAGO_OK).  No counterpart in the reference. */
int lago_distance_transform(float *out, const int32_t *L, int where, int32_t label, const double *spacing, int squared,
                            int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz, void *stream);

/* ---- fused geometry operators (beyond the reference's extension surface) -------------
 * compose: out = ds*u + dt*interp(v, u, ds) in one pass -- deform.compose
 * (/root/reference/lagomorph/deform.py:53-55), which the reference evaluates as one interp
 * kernel plus three elementwise kernels.  u, v, out: (nn, dim, sp).  Bit-identical to the
 * unfused expression (the three roundings are kept). */
int lago_compose_f32(float *out, const float *u, const float *v, double ds, double dt, int dim, int64_t nn,
                     int64_t nx, int64_t ny, int64_t nz, void *stream);
int lago_compose_f64(double *out, const double *u, const double *v, double ds, double dt, int dim, int64_t nn,
                     int64_t nx, int64_t ny, int64_t nz, void *stream);
/* The same with a hint: the caller expects |ds u| below one voxel everywhere, as in the Euler step of a shoot
 * (phi <- phi o (id - dt v)).  The hint changes speed only, never values: float32 3D calls that qualify for the LDS
 * window take a form whose window sits on the tile itself (lago_tuning.compose_near; LAGO_PATH_GATHER_WINDOW_NEAR), and
 * samples or whole tiles that are farther away than promised are served as lago_compose serves them.  Every other call
 * is lago_compose. */
int lago_compose_near_f32(float *out, const float *u, const float *v, double ds, double dt, int dim, int64_t nn,
                          int64_t nx, int64_t ny, int64_t nz, void *stream);
int lago_compose_near_f64(double *out, const double *u, const double *v, double ds, double dt, int dim, int64_t nn,
                          int64_t nx, int64_t ny, int64_t nz, void *stream);

/* lincomb: out[i] = c0 x0[i] + c1 x1[i] + ... (k = 1..4 terms, n elements), evaluated left to right with one fma per
 * term in the tensors' precision -- the elementwise sums of lddmm_step (lddmm.py:300-325: the regulariser's gradient
 * joining the velocity gradient, and `m.add_(-lr, p)` with p the sum of three gradient contributions) as one pass
 * each instead of torch's chain of mul / add kernels.  out may alias any input; unused inputs may be NULL. */
int lago_lincomb_f32(float *out, int k, const float *x0, const float *x1, const float *x2, const float *x3, double c0,
                     double c1, double c2, double c3, int64_t n, void *stream);
int lago_lincomb_f64(double *out, int k, const double *x0, const double *x1, const double *x2, const double *x3,
                     double c0, double c1, double c2, double c3, int64_t n, void *stream);

/* Ad_star (the coadjoint action of a diffeomorphism): out = (D phiinv + I) (m o (id + phiinv)) -- adjrep.Ad_star
 * (/root/reference/lagomorph/adjrep.py:86-97), which the reference evaluates as interp_forward
 * followed by jacobian_times_vectorfield_forward(displacement = true).  phiinv, m, out:
 * (nn, dim, sp); out may not alias an input.  Bit-identical to the two-call sequence (the
 * resampled momentum is rounded where that sequence stores it).  mphi (nullable, like m): when given, the
 * resampled momentum m o (id + phiinv) -- the interp_forward output of the two-call sequence -- is stored
 * there as well, so that a backward pass need not recompute it. */
int lago_Ad_star_f32(float *out, float *mphi, const float *phiinv, const float *m, int dim, int64_t nn, int64_t nx,
                     int64_t ny, int64_t nz, void *stream);
int lago_Ad_star_f64(double *out, double *mphi, const double *phiinv, const double *m, int dim, int64_t nn,
                     int64_t nx, int64_t ny, int64_t nz, void *stream);

/* interp_backward with start values (the fused backward forms of compose, Ad_star and expmap).  i_mode 0: d_I is
 * zeroed and receives the splat, exactly as lago_interp_backward; i_mode 1 (needs need_I): the splat is ADDED onto
 * the contents of d_I (a gradient accumulated over several calls, e.g. d/d m0 over the Euler steps of expmap).  The reference kernel owns d_u[n, d, x] in one thread and sums the channels' terms in
 * ascending order starting from zero (cuda/interp.cu:185-244); here the sum starts from
 *   u_mode 0: zero (identical to lago_interp_backward with need_u),
 *   u_mode 1: the contents of d_u on entry (d_u += ...: the `d_v.add_(d_u)` of a chain rule, without the extra pass),
 *   u_mode 2: addgo * grad_out[n, d, x] (needs nc == dim: the `ds * grad` term of compose's backward).
 * d_u is always produced (need_u is implied). */
int lago_interp_backward_fused_f32(float *d_I, float *d_u, const float *grad_out, const float *I, const float *u,
                                   double dt, int dim, int64_t nn, int64_t nc, int64_t nx, int64_t ny, int64_t nz,
                                   int broadcast_I, int need_I, int i_mode, int u_mode, double addgo, void *stream);
int lago_interp_backward_fused_f64(double *d_I, double *d_u, const double *grad_out, const double *I, const double *u,
                                   double dt, int dim, int64_t nn, int64_t nc, int64_t nx, int64_t ny, int64_t nz,
                                   int broadcast_I, int need_I, int i_mode, int u_mode, double addgo, void *stream);

/* jacobian_times_vectorfield_backward (lago_jtv_backward) whose d_v is added onto the contents of d_v when acc_v is
 * non-zero (d_w is always overwritten): the chain-rule sum of expmap's reverse sweep without a separate add pass. */
int lago_jtv_backward_acc_f32(float *d_v, float *d_w, const float *grad_out, const float *v, const float *w,
                              int displacement, int transpose, int dim, int64_t nn, int64_t nc, int64_t nx, int64_t ny,
                              int64_t nz, int acc_v, void *stream);
int lago_jtv_backward_acc_f64(double *d_v, double *d_w, const double *grad_out, const double *v, const double *w,
                              int displacement, int transpose, int dim, int64_t nn, int64_t nc, int64_t nx, int64_t ny,
                              int64_t nz, int acc_v, void *stream);

/* ad_star (the infinitesimal coadjoint action): out = (Dv)^T m - sum_d D_d^T (v_d m) -- adjrep.ad_star
 * (/root/reference/lagomorph/adjrep.py:69-83), which the reference evaluates as
 * jacobian_times_vectorfield_forward(v, m, transpose = true) minus
 * jacobian_times_vectorfield_adjoint_forward(m, v).  v, m, out: (nn, dim, sp); out may not alias an input.
 * Bit-identical to the three-call sequence. */
int lago_ad_star_f32(float *out, const float *v, const float *m, int dim, int64_t nn, int64_t nx, int64_t ny,
                     int64_t nz, void *stream);
int lago_ad_star_f64(double *out, const double *v, const double *m, int dim, int64_t nn, int64_t nx, int64_t ny,
                     int64_t nz, void *stream);

/* fluid_metric: the whole FluidMetricOperator.forward of the reference
 * (/root/reference/lagomorph/metric.py:11-19) in one call: out = irfft(L^(+-2) rfft(m)).
 * m, out: (nn, dim, nx, ny[, nz]) real; work: caller-provided scratch for the half spectrum,
 * nn*dim*nx*ny*(nz/2+1)*2 reals for dim == 3 (nn*dim*nx*(ny/2+1)*2 for dim == 2), clobbered.
 * m is not modified; out may not alias m.  LUTs as for lago_fluid_operator.
 * lut_generation: the float32 3D fast paths tabulate the per-frequency coefficients once per
 * (lut_generation, shape, alpha/beta/gamma, direction) in a library-owned device buffer (24 bytes per
 * frequency bin; the cache is bounded to 1 GiB and evicts oldest-first).  The table is a function of the
 * LUT *contents*, so the caller names a set of contents by a non-zero generation number and passes a new
 * number whenever it passes different contents (another shape, a refilled buffer); pointers are not part of
 * the key.  0 means "do not cache": the call takes the table-free path (rocFFT 3D plan + operator kernel).
 * hipFFT plans are cached inside the library per shape; their SetStream + Exec pairs are serialised. */
int lago_fluid_metric_f32(float *out, const float *m, float *work, int64_t lut_generation, int inverse,
                          const float *cosX, const float *sinX, const float *cosY, const float *sinY,
                          const float *cosZ, const float *sinZ, double alpha, double beta, double gamma, int dim,
                          int64_t nn, int64_t nx, int64_t ny, int64_t nz, void *stream);
int lago_fluid_metric_f64(double *out, const double *m, double *work, int64_t lut_generation, int inverse,
                          const double *cosX, const double *sinX, const double *cosY, const double *sinY,
                          const double *cosZ, const double *sinZ, double alpha, double beta, double gamma, int dim,
                          int64_t nn, int64_t nx, int64_t ny, int64_t nz, void *stream);
/* out = out_scale * (the field lago_fluid_metric returns): the factor multiplies the finished value in the field's
 * precision, i.e. the bits of a separate `out *= out_scale` pass, without that pass where the last kernel can take the
 * factor (the tuned 3D passes, the fused 2D kernel); one in-place pass inside the call otherwise.  For the Euler step
 * from the identity, phi_1 = -dt * sharp(m0) (lddmm.py:39-44 with a zero displacement; lagomorph_amd/lddmm.py). */
int lago_fluid_metric_scaled_f32(float *out, const float *m, float *work, int64_t lut_generation, int inverse,
                                 const float *cosX, const float *sinX, const float *cosY, const float *sinY,
                                 const float *cosZ, const float *sinZ, double alpha, double beta, double gamma, int dim,
                                 int64_t nn, int64_t nx, int64_t ny, int64_t nz, double out_scale, void *stream);
int lago_fluid_metric_scaled_f64(double *out, const double *m, double *work, int64_t lut_generation, int inverse,
                                 const double *cosX, const double *sinX, const double *cosY, const double *sinY,
                                 const double *cosZ, const double *sinZ, double alpha, double beta, double gamma, int dim,
                                 int64_t nn, int64_t nx, int64_t ny, int64_t nz, double out_scale, void *stream);
/* Drops every cached coefficient table (buffers still read by enqueued kernels are freed after them). */
void lago_fluid_cache_clear(void);
int lago_fluid_cache_entries(void);
/* rocFFT fallback plans (float64, 2D planes beyond the LDS, extents outside 2^a / 3*2^a / 5*2^a): how many are cached
 * and how many of them are currently verified by the spot check against a direct DFT (csrc/fft.hip: creating a plan
 * marks every plan unverified again; a check on an all-zero field or during stream capture proves nothing and leaves
 * the plan unverified).  Telemetry for the tests. */
int lago_fft_plan_state(int *plans, int *verified);

#ifdef __cplusplus
}
#endif
#endif /* LAGOMORPH_HIP_H */
