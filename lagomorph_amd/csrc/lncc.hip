// lncc: Gaussian-windowed local normalised cross-correlation of two (rows, nx, ny, nz) fields and its backward -- gfx950
// HIP kernels on the passes of gauss.hpp / gauss.hip.  No counterpart in the reference.
//
//   A = G I,  B = G J,  C = G(I I),  D = G(I J),  E = G(J J)            (G: the operator of gaussian_smooth)
//   sI = C - A^2,  sJ = E - B^2,  sX = D - A B,  cc = sX^2 / (sI sJ + eps)              (no clamping)
//
// and for an upstream gradient g on cc, with den = sI sJ + eps, cX = 2 sX / den, cI = -sX^2 sJ / den^2,
// cJ = -sX^2 sI / den^2 (G is self-adjoint):
//
//   dI = G[g (-2 A cI - B cX)] + 2 I G[g cI] + J G[g cX]
//   dJ = G[g (-2 B cJ - A cX)] + 2 J G[g cJ] + I G[g cX]
//
//   lncc_moments_kernel   the contiguous axis, always run: gauss_z_pass of gauss.hpp (the pass of gauss_z_kernel) over
//                         two staged fields, I and J, and five sums per position -- I, J and I I, I J, J J formed in
//                         double from each staged pair (exact for float32).  2 volumes read, 5 written into
//                         (5, rows, *sp); the kernel holds only that expansion and the five plane stores.  The
//                         remaining axes are gauss.hip's pass kernels over the stacked 5 rows (gauss_axis_pass).
//   lncc_cc_kernel        pointwise, 5 volumes read, 1 written.
//   lncc_coeff_kernel     pointwise: the 3 (one input) or 5 (both) coefficient fields under the G's of the backward, as
//                         (k, rows, *sp): one stacked call of lago_gauss_smooth filters them.
//   lncc_combine_kernel   pointwise: dI and / or dJ from the filtered coefficients, I and J.
//
// The pointwise arithmetic is in double for both precisions and rounded once on the store.  No atomics: every element
// is written once by its own lane from a sum in a fixed order, the same bits from call to call.
#include <initializer_list>

#include "gauss.hpp"

namespace lago {

template <typename R>
__global__ __launch_bounds__(kBlock) void lncc_moments_kernel(R *out, const R *I, const R *J, GaussTaps taps,
                                                              GaussPass p, uint64_t plane) {
    typedef R vec4 __attribute__((ext_vector_type(4)));
    const R *const fields[2] = {I, J};
    gauss_z_pass<R, 2, 5>(reinterpret_cast<R *>(gauss_smem), fields, taps, p,
                          [](const double (&v)[2], double (&x)[5]) {
        x[0] = v[0];
        x[1] = v[1];
        x[2] = v[0] * v[0];
        x[3] = v[0] * v[1];
        x[4] = v[1] * v[1];
    }, [&](uint64_t row, uint32_t z0, const double (&acc)[5][4]) {
        R *o = out + row * p.n + z0;
        if (p.vec && z0 + 3u < p.n) {
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                const vec4 x = {(R)acc[m][0], (R)acc[m][1], (R)acc[m][2], (R)acc[m][3]};
                *reinterpret_cast<vec4 *>(o + (size_t)m * plane) = x;
            }
            return;
        }
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (z0 + (uint32_t)k < p.n) o[(size_t)m * plane + k] = (R)acc[m][k];
    });
}

// ---- pointwise kernels: a lane owns four consecutive elements of the n = rows x voxels of one field; VEC: every base
// pointer is aligned to four elements and n is a multiple of four, so each field is one 4-vector per lane

template <typename R, bool VEC>
__device__ __forceinline__ void lncc_load4(const R *p, uint64_t e, uint64_t n, double (&v)[4]) {
    typedef R vec4 __attribute__((ext_vector_type(4)));
    if (VEC) {
        const vec4 x = *reinterpret_cast<const vec4 *>(p + e);
        v[0] = (double)x.x; v[1] = (double)x.y; v[2] = (double)x.z; v[3] = (double)x.w;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = e + (uint64_t)k < n ? (double)p[e + k] : 0.0;
}

template <typename R, bool VEC>
__device__ __forceinline__ void lncc_store4(R *p, uint64_t e, uint64_t n, const double (&v)[4]) {
    typedef R vec4 __attribute__((ext_vector_type(4)));
    if (VEC) {
        const vec4 x = {(R)v[0], (R)v[1], (R)v[2], (R)v[3]};
        *reinterpret_cast<vec4 *>(p + e) = x;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (e + (uint64_t)k < n) p[e + k] = (R)v[k];
}

// the local (co)variances of one voxel from its five moments
struct LnccStats {
    double A, B, sI, sJ, sX;
};
__device__ __forceinline__ LnccStats lncc_stats(double A, double B, double C, double D, double E) {
    LnccStats s;
    s.A = A;
    s.B = B;
    s.sI = C - A * A;
    s.sJ = E - B * B;
    s.sX = D - A * B;
    return s;
}

template <typename R, bool VEC>
__global__ __launch_bounds__(kBlock) void lncc_cc_kernel(R *cc, const R *mom, double eps, uint64_t n) {
    const uint64_t e = 4ull * ((uint64_t)blockIdx.x * kBlock + threadIdx.x);
    if (e >= n) return;
    double m[5][4], out[4];
#pragma unroll
    for (int q = 0; q < 5; ++q) lncc_load4<R, VEC>(mom + (size_t)q * n, e, n, m[q]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const LnccStats s = lncc_stats(m[0][k], m[1][k], m[2][k], m[3][k], m[4][k]);
        out[k] = (s.sX * s.sX) / (s.sI * s.sJ + eps);
    }
    lncc_store4<R, VEC>(cc, e, n, out);
}

// WHICH: 1 = the three fields of dI (g (-2 A cI - B cX), g cI, g cX), 2 = those of dJ (g (-2 B cJ - A cX), g cJ, g cX),
// 3 = five: dI's three, then g (-2 B cJ - A cX), g cJ
template <typename R, int WHICH, bool VEC>
__global__ __launch_bounds__(kBlock) void lncc_coeff_kernel(R *coef, const R *mom, const R *g, double eps, uint64_t n) {
    const uint64_t e = 4ull * ((uint64_t)blockIdx.x * kBlock + threadIdx.x);
    if (e >= n) return;
    constexpr int NF = WHICH == 3 ? 5 : 3;
    double m[5][4], gv[4], f[NF][4];
#pragma unroll
    for (int q = 0; q < 5; ++q) lncc_load4<R, VEC>(mom + (size_t)q * n, e, n, m[q]);
    lncc_load4<R, VEC>(g, e, n, gv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const LnccStats s = lncc_stats(m[0][k], m[1][k], m[2][k], m[3][k], m[4][k]);
        const double den = s.sI * s.sJ + eps;
        const double cX = (2.0 * s.sX) / den;
        const double q2 = -(s.sX * s.sX) / (den * den);
        const double cI = q2 * s.sJ, cJ = q2 * s.sI;
        const double pI = gv[k] * (-2.0 * s.A * cI - s.B * cX), pJ = gv[k] * (-2.0 * s.B * cJ - s.A * cX);
        if (WHICH == 2) {
            f[0][k] = pJ;
            f[1][k] = gv[k] * cJ;
        } else {
            f[0][k] = pI;
            f[1][k] = gv[k] * cI;
        }
        f[2][k] = gv[k] * cX;
        if (WHICH == 3) {
            f[NF - 2][k] = pJ;
            f[NF - 1][k] = gv[k] * cJ;
        }
    }
#pragma unroll
    for (int q = 0; q < NF; ++q) lncc_store4<R, VEC>(coef + (size_t)q * n, e, n, f[q]);
}

// `sm`: the filtered fields of lncc_coeff_kernel<WHICH>.  dI = S0 + 2 I S1 + J S2; dJ likewise from its own fields and
// the shared S2
template <typename R, int WHICH, bool VEC>
__global__ __launch_bounds__(kBlock) void lncc_combine_kernel(R *dI, R *dJ, const R *sm, const R *I, const R *J,
                                                              uint64_t n) {
    const uint64_t e = 4ull * ((uint64_t)blockIdx.x * kBlock + threadIdx.x);
    if (e >= n) return;
    constexpr int NF = WHICH == 3 ? 5 : 3;
    double s[NF][4], iv[4], jv[4], out[4];
#pragma unroll
    for (int q = 0; q < NF; ++q) lncc_load4<R, VEC>(sm + (size_t)q * n, e, n, s[q]);
    lncc_load4<R, VEC>(I, e, n, iv);
    lncc_load4<R, VEC>(J, e, n, jv);
    if (WHICH != 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = s[0][k] + 2.0 * iv[k] * s[1][k] + jv[k] * s[2][k];
        lncc_store4<R, VEC>(dI, e, n, out);
    }
    if (WHICH != 1) {
        constexpr int a = WHICH == 3 ? 3 : 0, b = WHICH == 3 ? 4 : 1;
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = s[a][k] + 2.0 * jv[k] * s[b][k] + iv[k] * s[2][k];
        lncc_store4<R, VEC>(dJ, e, n, out);
    }
}

// ---- host side

template <typename R>
static int lncc_moments_impl(R *out, const R *I, const R *J, R *scratch, const int *radii, const double *taps, int mode,
                             int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz, void *stream) {
    int rad[3];
    const double *tp[3];
    const int rc = gauss_parse_axes("lncc_moments", "lncc", "", dim, mode, radii, taps, rad, tp);
    if (rc != LAGO_OK) return rc;
    if (rows < 0 || rows >= (1ll << 28)) return fail_invalid("lncc_moments: bad extent");
    Geom g;
    if (!make_geom(g, dim, 5 * rows, nx, ny, nz)) return fail_invalid("lncc_moments: bad extent");
    if (g.nblocks == 0) return LAGO_OK;
    if (!out || !I || !J) return fail_invalid("lncc_moments: null pointer");
    const size_t bytes = (size_t)rows * g.nvox * sizeof(R);
    if (any_overlap({{out, 5 * bytes}}, {{I, bytes}, {J, bytes}}))
        return fail_invalid("lncc_moments: out must not alias an input");
    const int later = (rad[0] > 0) + (rad[1] > 0);   // passes after the moments pass, x before y
    if (later) {
        if (!scratch) return fail_invalid("lncc_moments: a filtered axis besides the last needs the scratch tensor");
        if (any_overlap({{scratch, 5 * bytes}}, {{I, bytes}, {J, bytes}, {out, 5 * bytes}}))
            return fail_invalid("lncc_moments: scratch must not alias an input or out");
    }
    hipStream_t s = (hipStream_t)stream;
    R *cur = later == 1 ? scratch : out;   // ping-pong so that the last pass writes `out`
    GaussPass p;
    GaussTaps tw;
    if (!gauss_plan<R>(p, 2, rad[2], mode, rows, g, cur)) return fail_invalid("lncc_moments: bad extent");
    gauss_fill_taps<R>(tw, rad[2], tp[2]);
    const uint64_t plane = (uint64_t)rows * g.nvox;
    size_t smem;
    const uint32_t nb = gauss_blocks<R>(p, 2, 2, smem);
    const hipError_t e = launch(lncc_moments_kernel<R>, dim3(nb), dim3(kBlock), smem, s, cur, I, J, tw, p, plane);
    if (e != hipSuccess) return fail_hip(e, "lncc_moments");
    for (int a = 0; a < 2; ++a) {
        if (rad[a] == 0) continue;
        R *dst = cur == out ? scratch : out;
        const int rp = gauss_axis_pass<R>("lncc_moments", dst, cur, a, rad[a], tp[a], mode, 5 * rows, g, s);
        if (rp != LAGO_OK) return rp;
        cur = dst;
    }
    return finish_launch(s, "lncc_moments");
}

static bool lncc_count_ok(int64_t n) { return n >= 0 && n < (1ll << 40); }

// What the pointwise entry points share once their arguments are checked: the grid of one lane per four of the n
// elements, VEC where n is a multiple of four and every pointer of `ptrs` is aligned to four elements, the launch
// f(VEC, grid, stream) -> hipError_t and its report under `name`.
template <typename R, typename F>
static int lncc_pointwise(const char *name, int64_t n, std::initializer_list<const void *> ptrs, void *stream, F f) {
    const dim3 grid((uint32_t)((n + 4 * kBlock - 1) / (4 * kBlock)));
    bool vec = n % 4 == 0;
    for (const void *p : ptrs) vec = vec && (uintptr_t)p % (4 * sizeof(R)) == 0;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    with_flags([&](auto VEC) { e = f(VEC, grid, s); }, vec);
    return launched(e, s, name);
}

template <typename R>
static int lncc_cc_impl(R *cc, const R *mom, double eps, int64_t n, void *stream) {
    if (!lncc_count_ok(n)) return fail_invalid("lncc_cc: bad extent");
    if (!(eps >= 0)) return fail_invalid("lncc_cc: eps must not be negative");
    if (n == 0) return LAGO_OK;
    if (!cc || !mom) return fail_invalid("lncc_cc: null pointer");
    if (overlaps(cc, (size_t)n * sizeof(R), mom, 5 * (size_t)n * sizeof(R)))
        return fail_invalid("lncc_cc: cc must not alias the moments");
    return lncc_pointwise<R>("lncc_cc", n, {cc, mom}, stream, [&](auto VEC, dim3 grid, hipStream_t s) {
        return launch(lncc_cc_kernel<R, VEC()>, grid, dim3(kBlock), 0, s, cc, mom, eps, (uint64_t)n);
    });
}

template <typename R>
static int lncc_coeffs_impl(R *coef, const R *mom, const R *g, double eps, int which, int64_t n, void *stream) {
    if (!lncc_count_ok(n)) return fail_invalid("lncc_coeffs: bad extent");
    if (which < 1 || which > 3) return fail_invalid("lncc_coeffs: which must be 1 (I), 2 (J) or 3 (both), got %d", which);
    if (!(eps >= 0)) return fail_invalid("lncc_coeffs: eps must not be negative");
    if (n == 0) return LAGO_OK;
    if (!coef || !mom || !g) return fail_invalid("lncc_coeffs: null pointer");
    const size_t bytes = (size_t)n * sizeof(R);
    const size_t cbytes = (which == 3 ? 5 : 3) * bytes;
    if (any_overlap({{coef, cbytes}}, {{mom, 5 * bytes}, {g, bytes}}))
        return fail_invalid("lncc_coeffs: coef must not alias an input");
    return lncc_pointwise<R>("lncc_coeffs", n, {coef, mom, g}, stream, [&](auto VEC, dim3 grid, hipStream_t s) {
        hipError_t e = hipSuccess;
        with_int<1, 2, 3>(which, [&](auto WHICH) {
            e = launch(lncc_coeff_kernel<R, WHICH(), VEC()>, grid, dim3(kBlock), 0, s, coef, mom, g, eps, (uint64_t)n);
        });
        return e;
    });
}

template <typename R>
static int lncc_combine_impl(R *dI, R *dJ, const R *sm, const R *I, const R *J, int which, int64_t n, void *stream) {
    if (!lncc_count_ok(n)) return fail_invalid("lncc_combine: bad extent");
    if (which < 1 || which > 3) return fail_invalid("lncc_combine: which must be 1 (I), 2 (J) or 3 (both), got %d", which);
    if (n == 0) return LAGO_OK;
    if (!sm || !I || !J || ((which & 1) && !dI) || ((which & 2) && !dJ)) return fail_invalid("lncc_combine: null pointer");
    const size_t bytes = (size_t)n * sizeof(R);
    R *const outs[2] = {(which & 1) ? dI : nullptr, (which & 2) ? dJ : nullptr};   // (an output not asked for is ignored)
    if (any_overlap({{outs[0], bytes}, {outs[1], bytes}}, {{sm, (which == 3 ? 5 : 3) * bytes}, {I, bytes}, {J, bytes}}))
        return fail_invalid("lncc_combine: an output must not alias an input or the other output");
    return lncc_pointwise<R>("lncc_combine", n, {sm, I, J, outs[0], outs[1]}, stream,
                             [&](auto VEC, dim3 grid, hipStream_t s) {
        hipError_t e = hipSuccess;
        with_int<1, 2, 3>(which, [&](auto WHICH) {
            e = launch(lncc_combine_kernel<R, WHICH(), VEC()>, grid, dim3(kBlock), 0, s, dI, dJ, sm, I, J, (uint64_t)n);
        });
        return e;
    });
}

}  // namespace lago

extern "C" {
#define LAGO_DEFINE(REAL, SUF)                                                                                      \
    int lago_lncc_moments##SUF(REAL *out, const REAL *I, const REAL *J, REAL *scratch, const int *radii,           \
                               const double *taps, int mode, int dim, int64_t rows, int64_t nx, int64_t ny,        \
                               int64_t nz, void *stream) {                                                         \
        return lago::lncc_moments_impl<REAL>(out, I, J, scratch, radii, taps, mode, dim, rows, nx, ny, nz, stream); \
    }                                                                                                               \
    int lago_lncc_cc##SUF(REAL *cc, const REAL *moments, double eps, int64_t n, void *stream) {                    \
        return lago::lncc_cc_impl<REAL>(cc, moments, eps, n, stream);                                               \
    }                                                                                                               \
    int lago_lncc_coeffs##SUF(REAL *coef, const REAL *moments, const REAL *g, double eps, int which, int64_t n,    \
                              void *stream) {                                                                      \
        return lago::lncc_coeffs_impl<REAL>(coef, moments, g, eps, which, n, stream);                               \
    }                                                                                                               \
    int lago_lncc_combine##SUF(REAL *dI, REAL *dJ, const REAL *smoothed, const REAL *I, const REAL *J, int which,  \
                               int64_t n, void *stream) {                                                          \
        return lago::lncc_combine_impl<REAL>(dI, dJ, smoothed, I, J, which, n, stream);                             \
    }
LAGO_DEFINE(float, _f32)
LAGO_DEFINE(double, _f64)
#undef LAGO_DEFINE
}
