// Point sets: sampling a field at positions that come from memory, and the adjoint -- gfx950 HIP kernels.  No
// counterpart in the reference.  Every other gather kernel of the library samples at i + dt u(i) for the voxel i its
// lane owns; here the lane owns point p of batch item n and reads its d coordinates from x (N, d, P), channel-first
// as every field, so that a field (N, d, *sp) reshaped to (N, d, -1) already is a point set.
//
//   interp_points_fwd_kernel   one lane per (n, p), grid ceil(P / 256) x N.  The d coordinates are d coalesced loads, the
//                              stencil (Lerp3 / Lerp2 of common.hpp, as they stand: lg_floor, t = x - floor, corners
//                              clamped with clamp1, the fma nesting of interp_forward) is set up once per point, and
//                              the channel loop takes one wave-uniform plane of F at a time: one buffer descriptor in
//                              SGPRs, four 8-byte pair gathers (z, z + 1) per channel in 3D.  Bit for bit the value
//                              interp_forward gives at the same position.
//   interp_points_bwd_kernel   the same mapping.  Per channel: the corners are fetched when d_x is wanted and the d
//                              components of sum_c g_c dF_c/dx accumulate in registers (c ascending from the c = 0
//                              product, lerp3_grad / Lerp2::grad on the fetched corners; written once with plain
//                              stores, no atomic: the same bits from call to call); when d_F is wanted the 2^d clamped
//                              corners each receive w_q g with one hardware float atomic, w_q = (a_x a_y) a_z formed in
//                              F's precision (a = 1 - t for the lower corner, t for the upper; a_y a_z in 2D).  The
//                              entry point zeroes d_F on the stream first.  The atomics round in arrival order: the
//                              last bits of d_F differ from call to call, as interp_backward's d_I.
//
// Every corner index is clamped before it is used (clamp1 is one v_med3_i32 on whatever integer the conversion gave),
// so no position, finite or not, addresses outside F or d_F.  Bytes per point and the resource usage of both kernels
// are in DESIGN.md; no LDS, no scratch.
#include "common.hpp"

#ifndef LAGO_NT_POINTS_ST
#define LAGO_NT_POINTS_ST 1   // the sampled values are written once and not re-read by the kernel: non-temporal, as interp_forward's output
#endif

namespace lago {

struct PtGeom {
    int nx, ny, nz;   // 2D: nx = 1, (ny, nz) = (H, W), as Geom
    uint32_t nvox;    // of one channel plane
    uint32_t np;      // points per batch item
};

// The 2^DIM corners of one point as ELEMENT offsets into a channel plane with their weights, from the stencil the
// gather uses (so the scatter is its exact transpose: the same floor, the same clamps).  3D corner order: the four rows
// (fx,fy) (cx,fy) (cx,cy) (fx,cy) at floor z, then the same rows at ceil z.
template <typename R>
__device__ __forceinline__ void point_corners(const Lerp3<R> &L, uint32_t (&o)[8], R (&w)[8]) {
    const R omt = (R)1.f - L.t, omu = (R)1.f - L.u, omv = (R)1.f - L.v;
    const R wr[4] = {omt * omu, L.t * omu, L.t * L.u, omt * L.u};
    const uint32_t dlo = L.f_hi ? 1u : 0u, dhi = L.c_lo ? 0u : 1u;   // (thin: f_hi false, c_lo true -- both the row's one voxel)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t e = L.rb[q] / (uint32_t)sizeof(R);
        o[q] = e + dlo;
        o[q + 4] = e + dhi;
        w[q] = wr[q] * omv;
        w[q + 4] = wr[q] * L.v;
    }
}
template <typename R>
__device__ __forceinline__ void point_corners(const Lerp2<R> &L, uint32_t (&o)[4], R (&w)[4]) {
    const R omt = (R)1.f - L.t, omu = (R)1.f - L.u;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = L.o[q];
    w[0] = omt * omu;
    w[1] = L.t * omu;
    w[2] = L.t * L.u;
    w[3] = omt * L.u;
}

template <typename R, int DIM, bool BC>
__global__ __launch_bounds__(kBlock) void interp_points_fwd_kernel(R *__restrict__ out, const R *__restrict__ F,
                                                                   const R *__restrict__ x, int nc, PtGeom g) {
    const uint32_t n = blockIdx.y, p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= g.np) return;
    const size_t nv = g.nvox, np = g.np;
    const R *xn = x + (size_t)n * DIM * np + p;
    const R *Fn = BC ? F : F + (size_t)n * nc * nv;
    R *on = out + (size_t)n * nc * np + p;
    if constexpr (DIM == 3) {
        Lerp3<R> L;
        L.setup(xn[0], xn[np], xn[2 * np], g.nx, g.ny, g.nz);
        for (int c = 0; c < nc; ++c) st_pol<LAGO_NT_POINTS_ST>(on + (size_t)c * np, L.value(Fn + (size_t)c * nv));
    } else {
        Lerp2<R> L;
        L.setup(xn[0], xn[np], g.ny, g.nz);
        for (int c = 0; c < nc; ++c) st_pol<LAGO_NT_POINTS_ST>(on + (size_t)c * np, L.value(Fn + (size_t)c * nv));
    }
}

template <typename R, int DIM, bool BC, bool NEED_F, bool NEED_X>
__global__ __launch_bounds__(kBlock) void interp_points_bwd_kernel(R *__restrict__ d_F, R *__restrict__ d_x,
                                                                   const R *__restrict__ go, const R *__restrict__ F,
                                                                   const R *__restrict__ x, int nc, PtGeom g) {
    const uint32_t n = blockIdx.y, p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= g.np) return;
    const size_t nv = g.nvox, np = g.np;
    const R *xn = x + (size_t)n * DIM * np + p;
    const R *Fn = BC ? F : F + (size_t)n * nc * nv;
    R *dFn = BC ? d_F : d_F + (size_t)n * nc * nv;
    const R *gon = go + (size_t)n * nc * np + p;
    constexpr int NQ = 1 << DIM;
    uint32_t o[NQ];
    R w[NQ];
    R acc[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) acc[a] = (R)0;
    std::conditional_t<DIM == 3, Lerp3<R>, Lerp2<R>> L;
    if constexpr (DIM == 3) L.setup(xn[0], xn[np], xn[2 * np], g.nx, g.ny, g.nz);
    else L.setup(xn[0], xn[np], g.ny, g.nz);
    if (NEED_F) point_corners(L, o, w);
    for (int c = 0; c < nc; ++c) {
        const R gc = gon[(size_t)c * np];
        if (NEED_X) {
            R gr[3];
            if constexpr (DIM == 3) L.grad(Fn + (size_t)c * nv, gr[0], gr[1], gr[2]);
            else L.grad(Fn + (size_t)c * nv, gr[0], gr[1]);
#pragma unroll
            for (int a = 0; a < DIM; ++a) acc[a] = c == 0 ? gr[a] * gc : lg_fma(gr[a], gc, acc[a]);
        }
        if (NEED_F) {
            R *dFc = dFn + (size_t)c * nv;
#pragma unroll
            for (int q = 0; q < NQ; ++q) atomic_add(dFc + o[q], w[q] * gc);
        }
    }
    if (NEED_X) {
        R *dxn = d_x + (size_t)n * DIM * np + p;
#pragma unroll
        for (int a = 0; a < DIM; ++a) dxn[(size_t)a * np] = acc[a];
    }
}

// The checks both entry points share, before any device call.  LAGO_OK with `empty` set: nothing to do.
static int points_geom(const char *what, PtGeom &g, bool &empty, int dim, int64_t nn, int64_t nc, int64_t np, int64_t nx,
                       int64_t ny, int64_t nz, size_t elem) {
    Volume v;   // one channel plane is addressed with 32-bit byte offsets
    if (const int rc = check_volume(v, what, dim, nx, ny, nz, plane_bytes32(elem), {nn, nc, np})) return rc;
    if (np >= (1ll << 31)) return fail_invalid("%s: 2^31 points or more per item", what);
    if (nc > INT_MAX) return fail_invalid("%s: 2^31 channels or more", what);
    empty = nn == 0 || nc == 0 || np == 0 || v.nvox == 0;
    if (!empty && nn > 65535) return fail_invalid("%s: more than 65535 batch items", what);   // the grid's second axis
    g = {(int)v.nx, (int)v.ny, (int)v.nz, (uint32_t)v.nvox, (uint32_t)np};
    return LAGO_OK;
}

template <typename R>
static int interp_points_impl(R *out, const R *F, const R *x, int dim, int64_t nn, int64_t nc, int64_t np, int64_t nx,
                              int64_t ny, int64_t nz, int bc, void *stream) {
    PtGeom g;
    bool empty;
    if (const int rc = points_geom("interp_points", g, empty, dim, nn, nc, np, nx, ny, nz, sizeof(R))) return rc;
    if (empty) return LAGO_OK;   // nothing to write
    const GatherBytes b(sizeof(R), sizeof(R), dim, nn, nc, g.np, g.nvox, bc);
    if (const int rc = check_gather("interp_points", out, F, x, b); rc != kLaunchNow) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((g.np + kBlock - 1) / kBlock, (uint32_t)nn);
    hipError_t e = hipSuccess;
    with_dim(dim, [&](auto DIM) {
        with_flags([&](auto BC) {
            e = launch(interp_points_fwd_kernel<R, DIM(), BC()>, grid, dim3(kBlock), 0, s, out, F, x, (int)nc, g);
        }, bc != 0);
    });
    return launched(e, s, "interp_points");
}

template <typename R>
static int interp_points_backward_impl(R *d_F, R *d_x, const R *go, const R *F, const R *x, int dim, int64_t nn, int64_t nc,
                                       int64_t np, int64_t nx, int64_t ny, int64_t nz, int bc, int need_F, int need_x,
                                       void *stream) {
    PtGeom g;
    bool empty;
    if (const int rc = points_geom("interp_points_backward", g, empty, dim, nn, nc, np, nx, ny, nz, sizeof(R))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const GatherBytes b(sizeof(R), sizeof(R), dim, nn, nc, g.np, g.nvox, bc);
    const int rc = check_gather_backward("interp_points_backward", d_F, d_x, go, F, x, b, need_F != 0, need_x != 0, empty, s);
    if (rc != kLaunchNow) return rc;
    const dim3 grid((g.np + kBlock - 1) / kBlock, (uint32_t)nn);
    hipError_t e = hipSuccess;
    with_dim(dim, [&](auto DIM) {
        with_flags([&](auto BC, auto NEED_F, auto NEED_X) {
            if constexpr (NEED_F() || NEED_X())   // (neither: the call was done above)
                e = launch(interp_points_bwd_kernel<R, DIM(), BC(), NEED_F(), NEED_X()>, grid, dim3(kBlock), 0, s, d_F, d_x,
                           go, F, x, (int)nc, g);
        }, bc != 0, need_F != 0, need_x != 0);
    });
    return launched(e, s, "interp_points_backward");
}

}  // namespace lago

extern "C" {
#define LAGO_DEFINE(REAL, SUF)                                                                                          \
    int lago_interp_points##SUF(REAL *out, const REAL *F, const REAL *x, int dim, int64_t nn, int64_t nc, int64_t np,   \
                                int64_t nx, int64_t ny, int64_t nz, int broadcast_F, void *stream) {                     \
        return lago::interp_points_impl<REAL>(out, F, x, dim, nn, nc, np, nx, ny, nz, broadcast_F, stream);              \
    }                                                                                                                   \
    int lago_interp_points_backward##SUF(REAL *d_F, REAL *d_x, const REAL *grad_out, const REAL *F, const REAL *x,      \
                                         int dim, int64_t nn, int64_t nc, int64_t np, int64_t nx, int64_t ny,            \
                                         int64_t nz, int broadcast_F, int need_F, int need_x, void *stream) {            \
        return lago::interp_points_backward_impl<REAL>(d_F, d_x, grad_out, F, x, dim, nn, nc, np, nx, ny, nz,            \
                                                       broadcast_F, need_F, need_x, stream);                             \
    }
LAGO_DEFINE(float, _f32)
LAGO_DEFINE(double, _f64)
#undef LAGO_DEFINE
}
