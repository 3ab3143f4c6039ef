// The per-voxel arithmetic of the Parzen joint histogram (mi.hip): the cubic B-spline window of one intensity, its
// derivative, the integer bin clamp, the fixed-point product of two weights and the gradient sum of the backward.
// Plain C++ that a host compiler builds as well (tests/native/mi_emul.cpp runs it against the numpy reference
// tests/mi_ref.py integer for integer).  Everything is in double, in exactly the order written; the library and the
// emulation are built with -ffp-contract=off, so nothing is fused or reassociated.
//
//   s  = (B - 3) / (hi - lo)                      (host, mi_axis)
//   vc = fmin(fmax(v, lo), hi)                    (a NaN voxel becomes lo)
//   c  = (vc - lo) * s + 1
//   k  = min(floor(c), B - 3) - 1                 (then clamped AS AN INTEGER to [0, B - 4])
//   t  = c - (k + 1)
//   w0 = u u u / 6, u = 1 - t     w1 = ((3 t - 6) t t + 4) / 6     w2 = (((-3 t + 3) t + 3) t + 1) / 6     w3 = t t t / 6
//   w0' = -(u u) / 2 s            w1' = (3 t - 4) t / 2 s          w2' = ((-3 t + 2) t + 1) / 2 s          w3' = t t / 2 s
//                                 (all four 0 unless lo <= v <= hi: 0 for NaN, +-inf and clamped voxels)
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LAGO_MI_HD __host__ __device__ __forceinline__
#else
#define LAGO_MI_HD inline
#endif

namespace lago {

constexpr double kMiOne = 4294967296.0;   // 2^LAGO_MI_FRAC_BITS: one voxel's whole weight in the fixed-point table

struct MiAxis {   // the range of one image and its bin scale
    double lo, hi, s;
};

LAGO_MI_HD MiAxis mi_axis(double lo, double hi, int B) {
    MiAxis ax;
    ax.lo = lo;
    ax.hi = hi;
    ax.s = (double)(B - 3) / (hi - lo);
    return ax;
}

// first bin k of the four a voxel of value v touches, in [0, B - 4] for EVERY v, and its offset t in that bin.  With
// lo, hi and s finite c is finite for every v (fmax / fmin drop a NaN, clamp an inf); fmin(NaN, B - 3) would be B - 3
// too.  The clamp is on the integer, after the conversion: no value can form an index outside the table.
LAGO_MI_HD int mi_locate(double v, const MiAxis &ax, int B, double &t) {
    const double vc = __builtin_fmin(__builtin_fmax(v, ax.lo), ax.hi);
    const double c = (vc - ax.lo) * ax.s + 1.0;
    int k = (int)(__builtin_fmin(__builtin_floor(c), (double)(B - 3)) - 1.0);
    k = k < 0 ? 0 : (k > B - 4 ? B - 4 : k);
    t = c - (double)(k + 1);
    return k;
}

// x / 6, the correctly rounded quotient, in three instructions instead of a division sequence (eight of them a voxel
// were most of the histogram kernel's arithmetic): with y = RN(1 / 6), q = RN(x y) is within an ulp of x / 6, the fma
// gives the remainder r = x - 6 q exactly, and RN(q + r y) is RN(x / 6) (Markstein's correction step; 6 = 1.5 x 4 is
// not the exceptional all-ones significand).  The bits of `x / 6.0` for every x but -0 (which gives +0; no numerator
// below can be -0): 4 x 10^8 random doubles of both signs between 2^-600 and 2^600 and dense in [0, 8], and subnormals,
// were compared on the host, and tests/test_mi_host.py compares every weight with numpy's division.
LAGO_MI_HD double mi_sixth(double x) {
    const double y = 1.0 / 6.0;
    const double q = x * y;
    return __builtin_fma(__builtin_fma(-6.0, q, x), y, q);
}

LAGO_MI_HD void mi_weights(double t, double (&w)[4]) {
    const double u = 1.0 - t;
    w[0] = mi_sixth(u * u * u);
    w[1] = mi_sixth((3.0 * t - 6.0) * t * t + 4.0);
    w[2] = mi_sixth(((-3.0 * t + 3.0) * t + 3.0) * t + 1.0);
    w[3] = mi_sixth(t * t * t);
}

// d w / d v at the voxel's own value v (not the clamped one: the window does not move outside the range)
LAGO_MI_HD void mi_derivs(double v, double t, const MiAxis &ax, double (&d)[4]) {
    const double u = 1.0 - t;
    const bool in = v >= ax.lo && v <= ax.hi;   // false for NaN
    d[0] = in ? -(u * u) / 2.0 * ax.s : 0.0;
    d[1] = in ? (3.0 * t - 4.0) * t / 2.0 * ax.s : 0.0;
    d[2] = in ? ((-3.0 * t + 2.0) * t + 1.0) / 2.0 * ax.s : 0.0;
    d[3] = in ? t * t / 2.0 * ax.s : 0.0;
}

// llrint(wa wb 2^32).  Both weights lie in [0, 2/3] (w0 may be a rounding error below 0 at v = hi, where the product
// rounds to -0), so the rounded value is an integer in [0, 2^31): the conversion goes through uint32, which is one
// instruction on the device, with the same result.
LAGO_MI_HD long long mi_fixed(double wa, double wb) {
    return (long long)(unsigned int)__builtin_rint(wa * wb * kMiOne);
}

// sum_a dw[a] (sum_b w[b] M[a][b]), a and b ascending, M = g (TR false) or its transpose (TR true): dI is
// mi_grad_sum<false>(wI', wJ, g) / nvox and dJ is mi_grad_sum<true>(wJ', wI, g) / nvox -- ONE function with the roles
// swapped and the table transposed, which is what makes (dI, dJ) of (J, I, G^T) the bits of (dJ, dI) of (I, J, G).
template <bool TR>
LAGO_MI_HD double mi_grad_sum(const double (&dw)[4], const double (&w)[4], const double (&g)[4][4]) {
    double out = 0.0;
    for (int a = 0; a < 4; ++a) {
        double in = w[0] * (TR ? g[0][a] : g[a][0]);
        for (int b = 1; b < 4; ++b) in = in + w[b] * (TR ? g[b][a] : g[a][b]);
        out = a == 0 ? dw[0] * in : out + dw[a] * in;
    }
    return out;
}

}  // namespace lago
