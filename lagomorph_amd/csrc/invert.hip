// invert_displacement: the fixed-point inverse of a deformation and its adjoint solve -- gfx950 HIP kernels.
//
// For phi = id + u the field v with (id + u) o (id + v) = id obeys v(x) = -u(x + v(x)).  The standard iteration
//     v_0 = -u,   v_{k+1}(x) = -u(x + v_k(x))
// written with the library's operators is one interp_forward and one negation per step: a round trip of v through HBM
// for every one of them (about 60 bytes per voxel and step for a 3-vector float32 field).  v_{k+1}(x) depends on u and
// on v_k at the SAME voxel only, so the whole loop runs here in one kernel: v stays in registers, the fixed u is
// re-gathered through the caches and v is written once.  No counterpart in the reference.
//
// The gathers are Lerp3 / Lerp2 of common.hpp, unchanged: the result is bit for bit the value of
//     v = -u;  for k in range(iters): v = -interp_forward(u, v, 1.0)
// (negation is exact; sample_pos with dt == 1 is one add, the rounding every interp_forward kernel applies).
#include "common.hpp"

namespace lago {

// Outputs are stored non-temporally, as the forward outputs of interp.hip and fused.hip are (profiles/r04_cache_policy.md:
// a kernel's own output must not displace the lines its gathers re-read).
constexpr int kInvertStoreNT = 1;

template <typename R> struct BitsOf;
template <> struct BitsOf<float> { typedef uint32_t type; };
template <> struct BitsOf<double> { typedef uint64_t type; };
template <typename R>
__device__ __forceinline__ bool same_bits(R a, R b) {
    typedef typename BitsOf<R>::type B;
    return __builtin_bit_cast(B, a) == __builtin_bit_cast(B, b);
}

// One voxel per lane.  The only stopping rule besides the count: a wavefront leaves the loop when the step changed no
// bit of any of its lanes' v -- every later step would gather at the same positions and reproduce the same bits.  Lanes
// beyond the volume iterate on voxel 0 of their batch item (in range) and store nothing, so the vote sees a full wave.
template <typename R, int DIM>
__global__ __launch_bounds__(kBlock) void invert_disp_kernel(R *__restrict__ out, const R *__restrict__ u, int iters,
                                                             Geom g) {
    const Vox vx = locate(g);
    const size_t nv = g.nvox;
    const uint32_t s = vx.valid ? vx.s : 0u;
    const R *un = u + (size_t)vx.n * DIM * nv;
    R v[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) v[d] = -un[(size_t)d * nv + s];
    for (int k = 0; k < iters; ++k) {
        R w[DIM];
        if (DIM == 3) {
            Lerp3<R> L;
            L.setup(sample_pos<R>(vx.i, 1.0, v[0]), sample_pos<R>(vx.j, 1.0, v[1]), sample_pos<R>(vx.k, 1.0, v[2]), g.nx,
                    g.ny, g.nz);
#pragma unroll
            for (int c = 0; c < DIM; ++c) w[c] = -L.value(un + (size_t)c * nv);
        } else {
            Lerp2<R> L;
            L.setup(sample_pos<R>(vx.j, 1.0, v[0]), sample_pos<R>(vx.k, 1.0, v[1]), g.ny, g.nz);
#pragma unroll
            for (int c = 0; c < DIM; ++c) w[c] = -L.value(un + (size_t)c * nv);
        }
        bool same = true;
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            same = same && same_bits(w[d], v[d]);
            v[d] = w[d];
        }
        if (__all(same)) break;
    }
    if (!vx.valid) return;
    R *on = out + (size_t)vx.n * DIM * nv + vx.s;
#pragma unroll
    for (int d = 0; d < DIM; ++d) st_pol<kInvertStoreNT>(&on[(size_t)d * nv], v[d]);
}

// The adjoint solve of the converged inverse.  From v = -u o psi, psi = id + v:  (I + G) dv = -du o psi with
// G[c][a] = (d_a u_c) o psi, hence <g, dv> = <lam, du o psi> for lam = -(I + G)^-T g, and d_u is the splat of lam at
// psi (interp_backward).  This kernel writes lam: per voxel the gradients of the three (two) components of u at
// x + v(x) (Lerp*::grad), M = I + G (the 1 added to the rounded gradient) and the solve by the adjugate,
// (M^-T)[c][a] = C[c][a] / det M with C the cofactor matrix.  Every product, sum and quotient is rounded on its own, in
// the order written in include/lagomorph_hip.h.  det M is not guarded: where the deformation folds, the IEEE result
// (inf / nan / huge) stands.  No atomics, nothing to clear: every element is written once by its own lane.
template <typename R, int DIM>
__global__ __launch_bounds__(kBlock) void invert_disp_adjoint_kernel(R *__restrict__ lam, const R *__restrict__ go,
                                                                     const R *__restrict__ u, const R *__restrict__ v,
                                                                     Geom g) {
    const Vox vx = locate(g);
    if (!vx.valid) return;
    const size_t nv = g.nvox;
    const size_t base = (size_t)vx.n * DIM * nv;
    const R *un = u + base;
    const R *vn = v + base + vx.s;
    const R *gn = go + base + vx.s;
    R *ln = lam + base + vx.s;
    R M[DIM][DIM], gg[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) gg[d] = gn[(size_t)d * nv];
    if constexpr (DIM == 3) {
        Lerp3<R> L;
        L.setup(sample_pos<R>(vx.i, 1.0, vn[0]), sample_pos<R>(vx.j, 1.0, vn[nv]), sample_pos<R>(vx.k, 1.0, vn[2 * nv]),
                g.nx, g.ny, g.nz);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            L.grad(un + (size_t)c * nv, M[c][0], M[c][1], M[c][2]);
            M[c][c] = M[c][c] + (R)1.0;
        }
        const R det = (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])) +
                      M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            R C[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
                C[a] = M[c1][a1] * M[c2][a2] - M[c1][a2] * M[c2][a1];
            }
            const R num = (C[0] * gg[0] + C[1] * gg[1]) + C[2] * gg[2];
            st_pol<kInvertStoreNT>(&ln[(size_t)c * nv], (R)(-(num / det)));
        }
    } else {
        Lerp2<R> L;
        L.setup(sample_pos<R>(vx.j, 1.0, vn[0]), sample_pos<R>(vx.k, 1.0, vn[nv]), g.ny, g.nz);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            L.grad(un + (size_t)c * nv, M[c][0], M[c][1]);
            M[c][c] = M[c][c] + (R)1.0;
        }
        const R det = M[0][0] * M[1][1] - M[0][1] * M[1][0];
        const R num0 = M[1][1] * gg[0] - M[1][0] * gg[1];
        const R num1 = M[0][0] * gg[1] - M[0][1] * gg[0];
        st_pol<kInvertStoreNT>(&ln[0], (R)(-(num0 / det)));
        st_pol<kInvertStoreNT>(&ln[nv], (R)(-(num1 / det)));
    }
}

template <typename R>
static int invert_forward_impl(R *out, const R *u, int iters, int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz,
                               void *stream) {
    if (iters < 0) return fail_invalid("invert_displacement_forward: iters must not be negative (got %d)", iters);
    if (dim != 2 && dim != 3) return fail_invalid("Only two- and three-dimensional displacement inversion is supported");
    Geom g;
    if (!make_geom(g, dim, nn, nx, ny, nz)) return fail_invalid("invert_displacement_forward: bad extent");
    if (g.nblocks == 0) return LAGO_OK;
    if (!out || !u) return fail_invalid("invert_displacement_forward: null pointer");
    // every lane re-gathers u at places other lanes write in `out`: in place is not possible
    if (overlaps(out, u, (size_t)nn * dim * g.nvox * sizeof(R)))
        return fail_invalid("invert_displacement_forward: out must not alias u");
    hipStream_t s = (hipStream_t)stream;
    with_dim(dim, [&](auto DIM) {
        hipLaunchKernelGGL((invert_disp_kernel<R, DIM()>), dim3(g.nblocks), dim3(kBlock), 0, s, out, u, iters, g);
    });
    return finish_launch(s, "invert_displacement_forward");
}

template <typename R>
static int invert_adjoint_impl(R *lam, const R *go, const R *u, const R *v, int dim, int64_t nn, int64_t nx, int64_t ny,
                               int64_t nz, void *stream) {
    if (dim != 2 && dim != 3) return fail_invalid("Only two- and three-dimensional displacement inversion is supported");
    Geom g;
    if (!make_geom(g, dim, nn, nx, ny, nz)) return fail_invalid("invert_displacement_adjoint: bad extent");
    if (g.nblocks == 0) return LAGO_OK;
    if (!lam || !go || !u || !v) return fail_invalid("invert_displacement_adjoint: null pointer");
    const size_t bytes = (size_t)nn * dim * g.nvox * sizeof(R);
    if (any_overlap({{lam, bytes}}, {{u, bytes}, {v, bytes}, {go, bytes}}))
        return fail_invalid("invert_displacement_adjoint: lam must not alias an input");
    hipStream_t s = (hipStream_t)stream;
    with_dim(dim, [&](auto DIM) {
        hipLaunchKernelGGL((invert_disp_adjoint_kernel<R, DIM()>), dim3(g.nblocks), dim3(kBlock), 0, s, lam, go, u, v, g);
    });
    return finish_launch(s, "invert_displacement_adjoint");
}

}  // namespace lago

extern "C" {
#define LAGO_DEFINE(REAL, SUF)                                                                                      \
    int lago_invert_disp_forward##SUF(REAL *out, const REAL *u, int iters, int dim, int64_t nn, int64_t nx,        \
                                      int64_t ny, int64_t nz, void *stream) {                                      \
        return lago::invert_forward_impl<REAL>(out, u, iters, dim, nn, nx, ny, nz, stream);                        \
    }                                                                                                               \
    int lago_invert_disp_adjoint##SUF(REAL *lam, const REAL *grad_out, const REAL *u, const REAL *v, int dim,      \
                                      int64_t nn, int64_t nx, int64_t ny, int64_t nz, void *stream) {              \
        return lago::invert_adjoint_impl<REAL>(lam, grad_out, u, v, dim, nn, nx, ny, nz, stream);                  \
    }
LAGO_DEFINE(float, _f32)
LAGO_DEFINE(double, _f64)
#undef LAGO_DEFINE
}
