// Cubic B-spline sampling along one axis: clamp, cell, weights, derivative weights and folded tap indices, as the
// gather kernels of bspline.hip use them -- and as a plain host compiler builds them (tests/native/bspline_emul.cpp
// runs this header on the CPU against the numpy reference, tests/bspline_ref.py).  Needs nothing but the language.
//
// One axis of extent n, position x in the coefficients' precision R:
//
//   x   <- fmin(fmax(x, 0), n - 1)         a NaN stays a NaN; +-inf clamp like any position outside.  `clamped` is set
//                                           when the position was moved (the value then does not depend on it)
//   f    = min(floor(x), n - 2), >= 0      the cell; x = n - 1 belongs to the LAST cell with t = 1, so that the taps
//   t    = x - f  in [0, 1]                f - 1 ... f + 2 stay in [-1, n] and one fold brings them into the grid
//   k_q  = fold(f - 1 + q), q = 0..3       fold: k -> |k|, then k -> 2 (n - 1) - k if k > n - 1 (the whole-sample
//                                           mirror of the prefilter); n = 1: every tap is index 0
//   s    = 1 - t
//   w    = (s^3, p(s), p(t), t^3) / 6      p(r) = ((3 - 3 r) r + 3) r + 1 -- the B-spline pieces 3t^3 - 6t^2 + 4 and
//                                           -3t^3 + 3t^2 + 3t + 1 written so that every sum adds terms of one sign
//   dw   = (-s^2, q(t), -q(s), t^2) / 2    q(r) = (3 r - 4) r;  dw_2 = -3t^2 + 2t + 1 = -q(s)
//
// Every operation is a single +, - or * in R (the library is built with -ffp-contract=off; no fma here), so a numpy
// float32 restatement gives the same bits.  Rounding: s carries one rounding; w_0 = ((s s) s) sixth has 3 u from s, two
// products and the rounded constant with its product: 7 u.  p(r): 3 r (1), 3 - 3r (absolute error <= 3 u + u b), times r,
// plus 3 (>= 3: relative 2.5 u), times r (3.5 u), plus 1 (4.5 u), times sixth (6.5 u); through s = fl(1 - t) one more u
// times the condition s p'(s) / p(s) < 1.  So every weight is within 7.5 u (1 + O(u)) of the exact cubic at the SAME t:
// tests/test_gpu_bspline.py takes 8 u per axis for its cell bound.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LAGO_BS_HD __host__ __device__ __forceinline__
#else
#define LAGO_BS_HD inline
#endif

namespace lago {

template <typename R>
struct BsAxis {
    int k[4];       // folded tap indices, each in [0, n - 1]
    R w[4];         // weights (sum 1)
    R t;            // position inside the cell, NaN for a NaN position
    int f;          // the cell
    bool clamped;   // the position lay outside [0, n - 1] (never for a NaN)
    bool nan;       // the position was a NaN
};

LAGO_BS_HD int bs_fold(int k, int n) {   // k in [-1, n], n >= 1
    if (n == 1) return 0;
    k = k < 0 ? -k : k;
    return k > n - 1 ? 2 * (n - 1) - k : k;
}

template <typename R>
LAGO_BS_HD R bs_poly(R r) {   // 6 x the B-spline piece next to the cell's own end: ((3 - 3 r) r + 3) r + 1
    const R a = (R)3 * r;
    const R b = (R)3 - a;
    const R c = b * r;
    const R d = c + (R)3;
    const R e = d * r;
    return e + (R)1;
}

template <typename R>
LAGO_BS_HD R bs_dpoly(R r) {   // 2 x: (3 r - 4) r
    const R a = (R)3 * r;
    const R b = a - (R)4;
    return b * r;
}

template <typename R>
LAGO_BS_HD void bs_axis(R x, int n, BsAxis<R> &A) {
    const R hi = (R)(n - 1);
    A.nan = !(x == x);
    A.clamped = x < (R)0 || x > hi;
    x = x < (R)0 ? (R)0 : x;
    x = x > hi ? hi : x;
    int f = A.nan ? 0 : (int)x;          // 0 <= x <= n - 1: truncation is the floor
    const int last = n >= 2 ? n - 2 : 0;
    f = f > last ? last : f;             // (also where (R)(n - 1) rounded up to n)
    A.f = f;
    const R t = x - (R)f;
    A.t = t;
    const R s = (R)1 - t;
    const R sixth = (R)(1.0 / 6.0);
    A.w[0] = ((s * s) * s) * sixth;
    A.w[1] = bs_poly(s) * sixth;
    A.w[2] = bs_poly(t) * sixth;
    A.w[3] = ((t * t) * t) * sixth;
    A.k[0] = bs_fold(f - 1, n);
    A.k[1] = bs_fold(f, n);
    A.k[2] = bs_fold(f + 1, n);
    A.k[3] = bs_fold(f + 2, n);
}

// d w_q / d x at the same t (meaningful where the position was not clamped)
template <typename R>
LAGO_BS_HD void bs_dweights(const BsAxis<R> &A, R (&dw)[4]) {
    const R t = A.t, s = (R)1 - t, half = (R)0.5;
    dw[0] = -((s * s) * half);
    dw[1] = bs_dpoly(t) * half;
    dw[2] = -(bs_dpoly(s) * half);
    dw[3] = (t * t) * half;
}

}  // namespace lago
