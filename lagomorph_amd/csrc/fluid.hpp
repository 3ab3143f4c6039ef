// The fluid metric family (lago_fluid_operator*, lago_fluid_metric*): what its seven translation units share.
//   * FluidOp<R>: the operator's arguments, built once in each C entry point and passed by value from there on;
//   * Cplx<R>: the complex pair of the half spectrum;
//   * FluidBin3 / FluidBin2: the operator on ONE frequency bin (cuda/metric.cu:20-160, :220-306) -- the symmetric 3 x 3
//     (2 x 2) symbol squared, applied to the real and the imaginary parts of the three (two) components, or its inverse
//     through a Cholesky factor.  The only place where the coefficient expressions are written: metric.hip's operator
//     kernel, the generic x pass (fftg.hip), the coefficient table (fftx.hip) and the fused 2D kernel (fft3.hip) all
//     set up a bin here, hence the same bits on every path;
//   * the functions of the family that are called across translation units, each under the file that defines it.
// The application of a TABULATED bin (the six coefficients read back from fluid_coef_kernel's table) is
// fl::fluid_bin in fft_lds.hpp, beside the tuned x pass that it was written for: that header also compiles for the
// host (tests/native/fft_emul.hip), which this one, with common.hpp's device code, does not.
#pragma once
#include "common.hpp"

namespace lago {

// cos / sin look-up tables per axis (the 2D paths read X and Y only) and the operator's parameters
template <typename R>
struct FluidOp {
    const R *cosX, *sinX, *cosY, *sinY, *cosZ, *sinZ;
    double alpha, beta, gamma;
};

template <typename R>
struct alignas(2 * sizeof(R)) Cplx {
    R re, im;
};

// cuda/metric.cu:14-18
template <typename R>
__device__ __forceinline__ R fb_safe_sqrt(R x) {
    if ((double)x < 1e-8) return (R)1e-4;
    return sizeof(R) == 4 ? (R)sqrtf((float)x) : (R)sqrt((double)x);  // correctly rounded (IEEE) forms
}
template <typename R>
__device__ __forceinline__ R fb_recip_via_double(R x) {  // `1./x` with x a Real: double division, narrowed
    return (R)(1. / (double)x);
}

// setup(): the bin (i, j, k) of the LUTs.  apply(): both parts of each component, then times `scale` (scale == 1 is a
// bitwise no-op).  INV: the six L are by-products, the factor is what apply() reads; !INV: the factor stays zero.
template <typename R, bool INV>
struct FluidBin3 {
    R L00, L10, L11, L20, L21, L22;
    R ooG00, G10, ooG11, G20, G21, ooG22;
    __device__ __forceinline__ void setup(const FluidOp<R> &o, int i, int j, int k) {
        const R wx = o.cosX[i], wy = o.cosY[j], wz = o.cosZ[k];
        const R sx = o.sinX[i], sy = o.sinY[j], sz = o.sinZ[k];
        const double alpha = o.alpha, beta = o.beta, gamma = o.gamma;
        const R lambda = (R)__builtin_fma(alpha, (double)(wx + wy + wz), gamma);
        const R l00 = (R)__builtin_fma(-beta, (double)wx, (double)lambda);
        const R l11 = (R)__builtin_fma(-beta, (double)wy, (double)lambda);
        const R l22 = (R)__builtin_fma(-beta, (double)wz, (double)lambda);
        const R l10 = (R)(beta * (double)sx * (double)sy);
        const R l20 = (R)(beta * (double)sx * (double)sz);
        const R l21 = (R)(beta * (double)sy * (double)sz);
        L00 = lg_fma(l20, l20, lg_fma(l00, l00, l10 * l10));
        L10 = lg_fma(l20, l21, lg_fma(l00, l10, l10 * l11));
        L11 = lg_fma(l21, l21, lg_fma(l10, l10, l11 * l11));
        L20 = lg_fma(l20, l22, lg_fma(l00, l20, l10 * l21));
        L21 = lg_fma(l21, l22, lg_fma(l10, l20, l11 * l21));
        L22 = lg_fma(l22, l22, lg_fma(l20, l20, l21 * l21));
        ooG00 = G10 = ooG11 = G20 = G21 = ooG22 = 0;
        if (INV) {  // cuda/metric.cu:47-78
            ooG00 = fb_recip_via_double(fb_safe_sqrt(L00));
            G10 = L10 * ooG00;
            G20 = L20 * ooG00;
            ooG11 = lg_fma(-G10, G10, L11);
            ooG11 = fb_recip_via_double(fb_safe_sqrt(ooG11));
            G21 = lg_fma(-G20, G10, L21) * ooG11;
            ooG22 = lg_fma(-G21, G21, lg_fma(-G20, G20, L22));
            ooG22 = fb_recip_via_double(fb_safe_sqrt(ooG22));
        }
    }
    __device__ __forceinline__ void apply(Cplx<R> &X, Cplx<R> &Y, Cplx<R> &Z, R scale) const {
        part(X.re, Y.re, Z.re);
        part(X.im, Y.im, Z.im);
        X = Cplx<R>{X.re * scale, X.im * scale};
        Y = Cplx<R>{Y.re * scale, Y.im * scale};
        Z = Cplx<R>{Z.re * scale, Z.im * scale};
    }
    __device__ __forceinline__ void part(R &bX, R &bY, R &bZ) const {
        if (INV) {  // cuda/metric.cu:103-130
            R y0 = bX * ooG00;
            R y1 = lg_fma(-G10, y0, bY) * ooG11;
            R y2 = lg_fma(-G21, y1, lg_fma(-G20, y0, bZ)) * ooG22;
            bZ = y2 * ooG22;
            bY = lg_fma(-G21, bZ, y1) * ooG11;
            bX = lg_fma(-G20, bZ, lg_fma(-G10, bY, y0)) * ooG00;
        } else {  // cuda/metric.cu:145-160
            R x = lg_fma(L20, bZ, lg_fma(L00, bX, L10 * bY));
            R y = lg_fma(L21, bZ, lg_fma(L10, bX, L11 * bY));
            bZ = lg_fma(L22, bZ, lg_fma(L20, bX, L21 * bY));
            bX = x;
            bY = y;
        }
    }
};

// the 2D operator (cuda/metric.cu:20-45, :80-101, :132-143, :162-218): bin (i, j) of the X and Y LUTs
template <typename R, bool INV>
struct FluidBin2 {
    R L00, L10, L11, ooG00, G10, ooG11;
    __device__ __forceinline__ void setup(const FluidOp<R> &o, int i, int j) {
        const R wx = o.cosX[i], wy = o.cosY[j];
        const R sx = o.sinX[i], sy = o.sinY[j];
        const double alpha = o.alpha, beta = o.beta, gamma = o.gamma;
        const R lambda = (R)__builtin_fma(alpha, (double)(wx + wy), gamma);
        const R l00 = (R)__builtin_fma(-beta, (double)wx, (double)lambda);
        const R l11 = (R)__builtin_fma(-beta, (double)wy, (double)lambda);
        const R l10 = (R)(beta * (double)sx * (double)sy);
        L00 = lg_fma(l00, l00, l10 * l10);
        L10 = lg_fma(l00, l10, l10 * l11);
        L11 = lg_fma(l11, l11, l10 * l10);
        ooG00 = G10 = ooG11 = 0;
        if (INV) {  // cuda/metric.cu:20-45
            ooG00 = fb_recip_via_double(fb_safe_sqrt(L00));
            G10 = L10 * ooG00;
            ooG11 = lg_fma(-G10, G10, L11);
            ooG11 = fb_recip_via_double(fb_safe_sqrt(ooG11));
        }
    }
    __device__ __forceinline__ void apply(Cplx<R> &X, Cplx<R> &Y, R scale) const {
        part(X.re, Y.re);
        part(X.im, Y.im);
        X = Cplx<R>{X.re * scale, X.im * scale};
        Y = Cplx<R>{Y.re * scale, Y.im * scale};
    }
    __device__ __forceinline__ void part(R &bX, R &bY) const {
        if (INV) {  // cuda/metric.cu:80-101
            R y0 = bX * ooG00;
            R y1 = lg_fma(-G10, y0, bY) * ooG11;
            bY = y1 * ooG11;
            bX = lg_fma(-G10, bY, y0) * ooG00;
        } else {  // cuda/metric.cu:132-143
            R x = lg_fma(L00, bX, L10 * bY);
            bY = lg_fma(L10, bX, L11 * bY);
            bX = x;
        }
    }
};

// ---- called across translation units (each defining file includes this header) ------------------------------------
// metric.hip: the operator kernel on a half spectrum of extents (nx, ny, nz), in place, times `scale`
template <typename R>
int fluid_operator_impl(R *Fm, int inverse, const FluidOp<R> &op, int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz,
                        hipStream_t s, double scale);

// fftx.hip: the coefficient table and the x pass that reads it between rocFFT's (y, z) plans
int fluid_coef_launch(float *tab, int inverse, const FluidOp<float> &op, int64_t nx, int64_t ny, int64_t nzc, int split,
                      hipStream_t s);
bool fluid_xpass_supported(int64_t nx);
int fluid_xpass_launch(float *F, const float *tab, int inverse, int64_t nn, int64_t nx, int64_t ny, int64_t nzc,
                       double scale, hipStream_t s);

// fft3.hip: the tuned LDS passes (3D, from a split-layout table) and the fused 2D kernel
bool fluid_native_supported(int64_t nx, int64_t ny, int64_t nz);
int fluid_metric_native(float *out, const float *m, float *work, const float *tab, int inverse, int64_t nn,
                        int64_t nx, int64_t ny, int64_t nz, double scale, hipStream_t s, float oscale);
bool fluid2d_supported(int64_t h, int64_t w);
int fluid_metric_2d(float *out, const float *m, int inverse, const FluidOp<float> &op, int64_t nn, int64_t h, int64_t w,
                    hipStream_t s, float oscale);

// fftg.hip: the generic passes
bool fluid_generic_supported(int dim, int64_t nx, int64_t ny, int64_t nz, size_t esize);
template <typename R>
int fluid_metric_generic(R *out, const R *m, R *work, int inverse, const FluidOp<R> &op, int dim, int64_t nn, int64_t nx,
                         int64_t ny, int64_t nz, hipStream_t s);
void tune_generic_fuse(int on);
void bluestein_cache_clear();
int bluestein_cache_entries();

}  // namespace lago
