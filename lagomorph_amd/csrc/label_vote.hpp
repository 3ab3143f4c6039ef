// The per-voxel arithmetic of warp_labels (labels.hip): the clamped sample position of one axis, its two corners, and
// the label of the 2^d corners -- the nearest one, or the one with the largest sum of multilinear weights.  Plain C++
// that a host compiler builds as well (tests/native/label_emul.cpp runs it against the numpy reference
// tests/labels_ref.py label for label).  The position is formed in the displacement's precision R, the weights and
// scores in double, in exactly the order written; the library and the emulation are built with -ffp-contract=off, so
// nothing is fused or reassociated.
//
//   p  = sample position i + dt u in R (lv_sample_pos: the expressions of common.hpp's sample_pos)
//   p  = fmin(fmax(p, -1), n)                 (no in-range position changes; out of range, +-inf and saturated ones
//                                              fall on the border voxel; a NaN becomes -1, the first voxel)
//   f  = floor(p), t = p - f                  (in R, then widened to double)
//   lo = clamp(f, 0, n - 1), hi = clamp(f + 1, 0, n - 1)
//   nearest: hi where t > 0.5, else lo (a tie at 0.5 goes to lo), per axis
//   vote   : corner q (first axis slowest) weighs w_q = (a_x a_y) a_z, a = 1 - t for lo and t for hi (2D: a_y a_z);
//            a label's score is the sum of w_q over the corners that carry it, q ascending from 0.0 (clamped corners
//            that coincide each add); the largest score wins, the smallest label value among equal scores
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LAGO_LV_HD __host__ __device__ __forceinline__
#define LAGO_LV_UNROLL _Pragma("unroll")   // the corner arrays must stay in registers on the device
#else
#define LAGO_LV_HD inline
#define LAGO_LV_UNROLL
#endif

namespace lago {

// the sample position of interp_forward (common.hpp: sample_pos, expression for expression): in double and narrowed
// to R, where for float and dt == +-1 the one float add is that value bit for bit
template <typename R>
LAGO_LV_HD R lv_sample_pos(int i, double dt, R u) {
    if (sizeof(R) == 4) {
        if (dt == 1.0) return (R)((float)i + (float)u);
        if (dt == -1.0) return (R)((float)i - (float)u);
    }
    return (R)__builtin_fma(dt, (double)u, (double)i);
}

LAGO_LV_HD float lv_minmax(float p, float lo, float hi) { return __builtin_fminf(__builtin_fmaxf(p, lo), hi); }
LAGO_LV_HD double lv_minmax(double p, double lo, double hi) { return __builtin_fmin(__builtin_fmax(p, lo), hi); }
LAGO_LV_HD float lv_floor(float p) { return __builtin_floorf(p); }
LAGO_LV_HD double lv_floor(double p) { return __builtin_floor(p); }

struct LvAxis {   // one axis of a sample: its two corners in [0, n - 1] and the offset t in [0, 1) between them
    int lo, hi;
    double t;
    LAGO_LV_HD int nearest() const { return t > 0.5 ? hi : lo; }
};

// p is in [-1, n] after the clamp (fmax and fmin drop a NaN), so floor(p) converts to an int exactly for every input
// and no corner can lie outside the axis.  n >= 1.
template <typename R>
LAGO_LV_HD LvAxis lv_axis(R p, int n) {
    p = lv_minmax(p, (R)-1, (R)n);
    const R fl = lv_floor(p);
    const int f = (int)fl;
    LvAxis a;
    a.t = (double)(p - fl);
    a.lo = f < 0 ? 0 : (f > n - 1 ? n - 1 : f);
    a.hi = f + 1 < 0 ? 0 : (f + 1 > n - 1 ? n - 1 : f + 1);
    return a;
}

// the weights of the 2^d corners, first axis slowest
LAGO_LV_HD void lv_weights(double tx, double ty, double tz, double (&w)[8]) {
    LAGO_LV_UNROLL
    for (int q = 0; q < 8; ++q) w[q] = (((q & 4) ? tx : 1.0 - tx) * ((q & 2) ? ty : 1.0 - ty)) * ((q & 1) ? tz : 1.0 - tz);
}
LAGO_LV_HD void lv_weights(double ty, double tz, double (&w)[4]) {
    LAGO_LV_UNROLL
    for (int q = 0; q < 4; ++q) w[q] = ((q & 2) ? ty : 1.0 - ty) * ((q & 1) ? tz : 1.0 - tz);
}

// The winner among NC corner labels c with weights w.  A label is scored at the first corner q that carries it: every
// weight is >= +0, so 0.0 + w[q] is w[q], and adding 0.0 for a later corner of another label leaves the sum as it is --
// s is the sum over the label's corners in ascending order from 0.0, in 7 - q additions.  A sample between two
// structures scores two labels; on the device a wave skips the corners at which none of its lanes meets a new label.
template <int NC>
LAGO_LV_HD int32_t lv_vote(const int32_t (&c)[NC], const double (&w)[NC]) {
    int32_t best = c[0];
    double top = -1.0;
    LAGO_LV_UNROLL
    for (int q = 0; q < NC; ++q) {
        bool first = true;
        LAGO_LV_UNROLL
        for (int r = 0; r < q; ++r) first = first && c[r] != c[q];
        if (first) {
            double s = w[q];
            LAGO_LV_UNROLL
            for (int r = q + 1; r < NC; ++r) s = s + (c[r] == c[q] ? w[r] : 0.0);
            if (s > top || (s == top && c[q] < best)) {
                top = s;
                best = c[q];
            }
        }
    }
    return best;
}

}  // namespace lago
