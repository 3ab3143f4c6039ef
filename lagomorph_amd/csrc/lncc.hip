// lncc: Gaussian-windowed local normalised cross-correlation of two (rows, nx, ny, nz) fields and its backward -- gfx950
// HIP kernels on the passes of gauss.hip.  No counterpart in the reference.
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
//   lncc_moments_kernel   the contiguous axis, always run.  A workgroup stages the I and J row tiles plus halo in LDS
//                         (gauss_z_kernel's tile, border rule applied while loading); a lane owns four consecutive
//                         outputs, walks its window once, forms I I, I J, J J in double from each staged pair (exact for
//                         float32) and feeds five accumulator sets: 2 volumes read, 5 written into (5, rows, *sp).
//                         The remaining axes are gauss.hip's pass kernels over the stacked 5 rows (gauss_axis_pass).
//   lncc_cc_kernel        pointwise, 5 volumes read, 1 written.
//   lncc_coeff_kernel     pointwise: the 3 (one input) or 5 (both) coefficient fields under the G's of the backward, as
//                         (k, rows, *sp): one stacked call of lago_gauss_smooth filters them.
//   lncc_combine_kernel   pointwise: dI and / or dJ from the filtered coefficients, I and J.
//
// The pointwise arithmetic is in double for both precisions and rounded once on the store.  No atomics: every element
// is written once by its own lane from a sum in a fixed order, the same bits from call to call.
#include "gauss.hpp"

namespace lago {

extern __shared__ __attribute__((aligned(32))) unsigned char lncc_smem[];

// acc[m][o] += t * x_m for the five moments m of one staged pair (a, b) and the four outputs o of the lane
__device__ __forceinline__ void lncc_feed(double (&acc)[5][4], const double (&t)[7], int i, double a, double b) {
    const double x[5] = {a, b, a * a, a * b, b * b};
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[m][o] = lg_fma(t[i - o + 3], x[m], acc[m][o]);
}

template <typename R>
__global__ __launch_bounds__(kBlock) void lncc_moments_kernel(R *out, const R *I, const R *J, GaussTaps taps,
                                                              GaussPass p, uint64_t plane) {
    typedef R vec4 __attribute__((ext_vector_type(4)));
    const uint32_t staged = p.RT * p.pitch;
    R *ldsI = reinterpret_cast<R *>(lncc_smem);
    R *ldsJ = ldsI + staged;   // (staged is a multiple of 4: the 4-vector reads below stay aligned)
    const uint32_t rb = p.dseg.div(blockIdx.x);
    const uint32_t seg = blockIdx.x - rb * p.nseg;
    const uint64_t row0 = (uint64_t)rb * p.RT;
    const int zs0 = (int)(seg * p.ZS);
    const int lo = p.H - p.r, hi = p.H + (int)p.ZS + p.r;   // staged positions outside [lo, hi) carry zero taps only
    for (uint32_t e0 = threadIdx.x; e0 < staged; e0 += kGaussInFlight * kBlock) {   // loads first, then the LDS stores
        R vi[kGaussInFlight], vj[kGaussInFlight];
#pragma unroll
        for (int f = 0; f < kGaussInFlight; ++f) {
            const uint32_t e = e0 + (uint32_t)f * kBlock;
            const uint32_t rl = p.dpitch.div(e);
            const int q = (int)(e - rl * p.pitch);
            const uint64_t row = row0 + rl;
            vi[f] = (R)0;
            vj[f] = (R)0;
            if (e < staged && row < p.outer && q >= lo && q < hi) {
                bool inside;
                const uint32_t u = gauss_resolve<R>(p, zs0 - p.H + q, inside);
                if (inside) {
                    vi[f] = I[row * p.n + u];
                    vj[f] = J[row * p.n + u];
                }
            }
        }
#pragma unroll
        for (int f = 0; f < kGaussInFlight; ++f) {
            const uint32_t e = e0 + (uint32_t)f * kBlock;
            if (e < staged) {
                ldsI[e] = vi[f];
                ldsJ[e] = vj[f];
            }
        }
    }
    __syncthreads();
    const uint32_t item = threadIdx.x;
    if (item >= p.RT * p.nzc) return;
    const uint32_t rl = p.dzc.div(item);
    const uint32_t c = item - rl * p.nzc;
    const uint64_t row = row0 + rl;
    const uint32_t z0 = (uint32_t)zs0 + 4u * c;
    if (row >= p.outer || z0 >= p.n) return;
    const R *wi = ldsI + rl * p.pitch + 4u * c;
    const R *wj = ldsJ + rl * p.pitch + 4u * c;
    R res[5][4];
    if (p.H == 0) {   // radius 0: the values and their products, each rounded once
        const vec4 a = *reinterpret_cast<const vec4 *>(wi), b = *reinterpret_cast<const vec4 *>(wj);
        const R av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const double x = (double)av[o], y = (double)bv[o];
            res[0][o] = av[o];
            res[1][o] = bv[o];
            res[2][o] = (R)(x * x);
            res[3][o] = (R)(x * y);
            res[4][o] = (R)(y * y);
        }
    } else {
        // the sliding sum of gauss.hip (gauss_slide) with five accumulator sets: output o sits at window position
        // H + o, so value j carries tap j - H - o
        double acc[5][4];
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[m][o] = 0.0;
        double t[7];
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j + 4] = 0.0;
        const int steps = (2 * p.H + 4) >> 2;
        for (int s = 0; s < steps; ++s) {
            const int k0 = 4 * s - p.H;
#pragma unroll
            for (int j = 0; j < 3; ++j) t[j] = t[j + 4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + j;
                t[j + 3] = taps.w[k < 0 ? -k : k];
            }
            const vec4 a = *reinterpret_cast<const vec4 *>(wi + 4 * s), b = *reinterpret_cast<const vec4 *>(wj + 4 * s);
            lncc_feed(acc, t, 0, (double)a.x, (double)b.x);
            lncc_feed(acc, t, 1, (double)a.y, (double)b.y);
            lncc_feed(acc, t, 2, (double)a.z, (double)b.z);
            lncc_feed(acc, t, 3, (double)a.w, (double)b.w);
        }
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int o = 0; o < 4; ++o) res[m][o] = (R)acc[m][o];
    }
    R *o0 = out + row * p.n + z0;
    if (p.vec && z0 + 3u < p.n) {
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            const vec4 x = {res[m][0], res[m][1], res[m][2], res[m][3]};
            *reinterpret_cast<vec4 *>(o0 + (size_t)m * plane) = x;
        }
        return;
    }
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (z0 + (uint32_t)k < p.n) o0[(size_t)m * plane + k] = res[m][k];
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

// do [a, a + na) and [b, b + nb) bytes intersect?  (common.hpp's overlaps() is for two buffers of one size)
static bool lncc_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + nb && q < p + na;
}

template <typename R>
static int lncc_moments_impl(R *out, const R *I, const R *J, R *scratch, const int *radii, const double *taps, int mode,
                             int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz, void *stream) {
    if (dim != 2 && dim != 3) return fail_invalid("Only two- and three-dimensional lncc is supported");
    if (mode != LAGO_GAUSS_WRAP && mode != LAGO_GAUSS_ZERO) return fail_invalid("lncc_moments: unknown border mode %d", mode);
    if (!radii) return fail_invalid("lncc_moments: null radii");
    int rad[3] = {0, 0, 0};   // per axis of the (nx, ny, nz) geometry; a 2D field is (1, H, W)
    const double *tp[3] = {nullptr, nullptr, nullptr};
    for (int a = 0; a < dim; ++a) {
        const int r = radii[a];
        if (r < 0 || r > kGaussMaxRadius)
            return fail_invalid("lncc_moments: radius %d is outside 0..%d", r, kGaussMaxRadius);
        if (r > 0 && !taps) return fail_invalid("lncc_moments: null taps");
        rad[a + 3 - dim] = r;
        tp[a + 3 - dim] = taps ? taps + (size_t)a * (kGaussMaxRadius + 1) : nullptr;
    }
    if (rows < 0 || rows >= (1ll << 28)) return fail_invalid("lncc_moments: bad extent");
    Geom g;
    if (!make_geom(g, dim, 5 * rows, nx, ny, nz)) return fail_invalid("lncc_moments: bad extent");
    if (g.nblocks == 0) return LAGO_OK;
    if (!out || !I || !J) return fail_invalid("lncc_moments: null pointer");
    const size_t bytes = (size_t)rows * g.nvox * sizeof(R);
    if (lncc_overlap(out, 5 * bytes, I, bytes) || lncc_overlap(out, 5 * bytes, J, bytes))
        return fail_invalid("lncc_moments: out must not alias an input");
    const int later = (rad[0] > 0) + (rad[1] > 0);   // passes after the moments pass, x before y
    if (later) {
        if (!scratch) return fail_invalid("lncc_moments: a filtered axis besides the last needs the scratch tensor");
        if (lncc_overlap(scratch, 5 * bytes, I, bytes) || lncc_overlap(scratch, 5 * bytes, J, bytes) ||
            overlaps(scratch, out, 5 * bytes))
            return fail_invalid("lncc_moments: scratch must not alias an input or out");
    }
    hipStream_t s = (hipStream_t)stream;
    R *cur = later == 1 ? scratch : out;   // ping-pong so that the last pass writes `out`
    GaussPass p;
    GaussTaps tw;
    if (!gauss_plan<R>(p, 2, rad[2], mode, rows, g, cur)) return fail_invalid("lncc_moments: bad extent");
    gauss_fill_taps<R>(tw, rad[2], tp[2]);
    const uint64_t plane = (uint64_t)rows * g.nvox;
    const uint32_t nb = (uint32_t)((p.outer + p.RT - 1) / p.RT * p.nseg);
    const size_t smem = 2 * (size_t)p.RT * p.pitch * sizeof(R);
    const hipError_t e = launch(lncc_moments_kernel<R>, dim3(nb), dim3(kBlock), smem, s, cur, I, J, tw, p, plane);
    if (e != hipSuccess) return fail_hip(e, "lncc_moments");
    for (int a = 0; a < 2; ++a) {
        if (rad[a] == 0) continue;
        R *dst = cur == out ? scratch : out;
        if (!gauss_axis_pass<R>(dst, cur, a, rad[a], tp[a], mode, 5 * rows, g, s))
            return fail_invalid("lncc_moments: bad extent");
        cur = dst;
    }
    return finish_launch(s, "lncc_moments");
}

static bool lncc_aligned(const void *p, size_t elem) { return (uintptr_t)p % (4 * elem) == 0; }

static bool lncc_grid(int64_t n, uint32_t &nb) {
    if (n < 0 || n >= (1ll << 40)) return false;
    nb = (uint32_t)((n + 4 * kBlock - 1) / (4 * kBlock));
    return true;
}

template <typename R>
static int lncc_cc_impl(R *cc, const R *mom, double eps, int64_t n, void *stream) {
    uint32_t nb;
    if (!lncc_grid(n, nb)) return fail_invalid("lncc_cc: bad extent");
    if (!(eps >= 0)) return fail_invalid("lncc_cc: eps must not be negative");
    if (n == 0) return LAGO_OK;
    if (!cc || !mom) return fail_invalid("lncc_cc: null pointer");
    if (lncc_overlap(cc, (size_t)n * sizeof(R), mom, 5 * (size_t)n * sizeof(R))) return fail_invalid("lncc_cc: cc must not alias the moments");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = n % 4 == 0 && lncc_aligned(cc, sizeof(R)) && lncc_aligned(mom, sizeof(R));
    hipError_t e = hipSuccess;
    with_flags([&](auto VEC) { e = launch(lncc_cc_kernel<R, VEC()>, dim3(nb), dim3(kBlock), 0, s, cc, mom, eps, (uint64_t)n); },
               vec);
    if (e != hipSuccess) return fail_hip(e, "lncc_cc");
    return finish_launch(s, "lncc_cc");
}

template <typename R>
static int lncc_coeffs_impl(R *coef, const R *mom, const R *g, double eps, int which, int64_t n, void *stream) {
    uint32_t nb;
    if (!lncc_grid(n, nb)) return fail_invalid("lncc_coeffs: bad extent");
    if (which < 1 || which > 3) return fail_invalid("lncc_coeffs: which must be 1 (I), 2 (J) or 3 (both), got %d", which);
    if (!(eps >= 0)) return fail_invalid("lncc_coeffs: eps must not be negative");
    if (n == 0) return LAGO_OK;
    if (!coef || !mom || !g) return fail_invalid("lncc_coeffs: null pointer");
    const size_t bytes = (size_t)n * sizeof(R);
    const size_t cbytes = (which == 3 ? 5 : 3) * bytes;
    if (lncc_overlap(coef, cbytes, mom, 5 * bytes) || lncc_overlap(coef, cbytes, g, bytes))
        return fail_invalid("lncc_coeffs: coef must not alias an input");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = n % 4 == 0 && lncc_aligned(coef, sizeof(R)) && lncc_aligned(mom, sizeof(R)) && lncc_aligned(g, sizeof(R));
    hipError_t e = hipSuccess;
    with_int<1, 2, 3>(which, [&](auto WHICH) {
        with_flags([&](auto VEC) {
            e = launch(lncc_coeff_kernel<R, WHICH(), VEC()>, dim3(nb), dim3(kBlock), 0, s, coef, mom, g, eps, (uint64_t)n);
        }, vec);
    });
    if (e != hipSuccess) return fail_hip(e, "lncc_coeffs");
    return finish_launch(s, "lncc_coeffs");
}

template <typename R>
static int lncc_combine_impl(R *dI, R *dJ, const R *sm, const R *I, const R *J, int which, int64_t n, void *stream) {
    uint32_t nb;
    if (!lncc_grid(n, nb)) return fail_invalid("lncc_combine: bad extent");
    if (which < 1 || which > 3) return fail_invalid("lncc_combine: which must be 1 (I), 2 (J) or 3 (both), got %d", which);
    if (n == 0) return LAGO_OK;
    if (!sm || !I || !J || ((which & 1) && !dI) || ((which & 2) && !dJ)) return fail_invalid("lncc_combine: null pointer");
    const size_t bytes = (size_t)n * sizeof(R);
    for (R *d : {(which & 1) ? dI : nullptr, (which & 2) ? dJ : nullptr}) {
        if (!d) continue;
        if (lncc_overlap(d, bytes, sm, (which == 3 ? 5 : 3) * bytes) || overlaps(d, I, bytes) || overlaps(d, J, bytes))
            return fail_invalid("lncc_combine: an output must not alias an input");
    }
    if (which == 3 && overlaps(dI, dJ, bytes)) return fail_invalid("lncc_combine: dI must not alias dJ");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = n % 4 == 0 && lncc_aligned(sm, sizeof(R)) && lncc_aligned(I, sizeof(R)) && lncc_aligned(J, sizeof(R)) &&
                     (!(which & 1) || lncc_aligned(dI, sizeof(R))) && (!(which & 2) || lncc_aligned(dJ, sizeof(R)));
    hipError_t e = hipSuccess;
    with_int<1, 2, 3>(which, [&](auto WHICH) {
        with_flags([&](auto VEC) {
            e = launch(lncc_combine_kernel<R, WHICH(), VEC()>, dim3(nb), dim3(kBlock), 0, s, dI, dJ, sm, I, J, (uint64_t)n);
        }, vec);
    });
    if (e != hipSuccess) return fail_hip(e, "lncc_combine");
    return finish_launch(s, "lncc_combine");
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
