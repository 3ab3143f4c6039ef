// Image pyramid by a factor of two: the per-axis matrices of the reduce R and the expand E, their tap ranges, and the
// one evaluation order -- as the kernels of pyramid.hip use them, and as a plain host compiler builds them
// (tests/native/pyramid_emul.cpp runs this header on the CPU against the numpy restatement, tests/pyramid_ref.py).
// Needs nothing but the language.  The definition is in include/lagomorph_hip.h (lago_pyramid_down).
//
// One axis of fine extent n >= 1; the coarse extent is m = (n + 1) / 2 and coarse voxel j sits at fine voxel 2 j.
//
//   R (m x n)   (R a)[j] = sum_{k = -2..2} w_k a[clamp(2 j + k, 0, n - 1)],  w = (1, 4, 6, 4, 1) / 16
//               R[j][x]  = the sum of the w_k whose clamped index is x: sixteenths, rows sum to 1; non-zero only for
//                          |2 j - x| <= 2 (the clamp moves weight onto the first or last column, never beyond the band)
//   E (n x m)   (E c)[2 j] = c[j],  (E c)[2 j + 1] = (c[j] + c[min(j + 1, m - 1)]) / 2
//               E[x][j]  = 1 (x = 2 j), 1/2 per coincidence (x odd: j = x / 2 and j = min(x / 2 + 1, m - 1), which are
//                          the same j at the last voxel of an even n: 1), rows sum to 1; non-zero only for |x - 2 j| <= 1
//
// Every entry is a dyadic number with at most four fraction bits, exact in float32 and float64.  Both matrices are
// addressed as W::at(j, x, n) with j the coarse and x the fine index (PyrReduce, PyrExpand), whichever way they are
// applied.  The two directions a matrix of either kind is applied in:
//
//   down  (coarse out, fine in: R and E^T)   out[j] = sum_{k = 0..4} W::at(j, 2 j - 2 + k, n) in[2 j - 2 + k]
//   up    (fine out, coarse in: E and R^T)   out[x] = sum_{t = 0..2} W::at(x / 2 - 1 + t, x, n) in[x / 2 - 1 + t]
//
// A tap outside the input's axis weighs exactly 0 (pyr_down_weight, pyr_up_weight) and is multiplied like any other:
// the kernels read a clamped or zeroed cell there, so the term is +-0 for finite data.  The ranges cover both bands.
//
// Evaluation order.  One axis at a time, the result of one contraction rounded to the field's precision R before the
// next: DOWN contracts the contiguous axis first (z, then y, then x: each pass halves what the next one reads), UP the
// contiguous axis last (x, then y, then z: each pass doubles what the next one reads).  2D fields are (y, z).  One
// contraction (pyr_dot) takes its taps ascending: acc = w_0 v_0, then acc = acc + w_t v_t -- a product and an addition,
// each rounded on its own; the library is built with -ffp-contract=off and nothing here is an fma, so a numpy
// restatement gives the same bits.  After the last axis the sum is multiplied by the caller's scale, rounded to R once
// (pyr_scale).
//
// Roundings between the input and one output element, longest path: per axis one product and four additions (down;
// up has one and two), then the scale: K = 5 d + 1 (kPyrRoundings: 16 in 3D, 11 in 2D).  A result is within
// K u sum_taps |W| |in| |scale| of the exact one, u the unit roundoff of R -- tests/test_gpu_pyramid.py.  For
// integer-valued inputs of magnitude <= 512 and a scale of 1 or 2 every product and partial sum is a multiple of 2^-12
// of magnitude <= 2^10 (R, R^T: column sums stay below 1) or a multiple of 2^-3 of magnitude <= 2^13 (E, E^T): it
// fits float32's 24-bit significand, nothing rounds, and the result is exact in any order.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LAGO_PY_HD __host__ __device__ __forceinline__
#else
#define LAGO_PY_HD inline
#endif

namespace lago {

constexpr int kPyramidReduce = 0, kPyramidExpand = 1;   // LAGO_PYRAMID_* of the header: which matrix
constexpr int kPyrDownTaps = 5, kPyrUpTaps = 3;
constexpr int kPyrRoundings(int dim) { return 5 * dim + 1; }
// the order the axes (x, y, z as laid out in memory; dim 2: y, z) are contracted in
constexpr int kPyrDownOrder[3] = {2, 1, 0}, kPyrUpOrder[3] = {0, 1, 2};

LAGO_PY_HD int64_t pyr_coarse_extent(int64_t n) { return (n + 1) / 2; }   // n >= 0

LAGO_PY_HD int pyr_clamp(int v, int n) { return v < 0 ? 0 : v > n - 1 ? n - 1 : v; }   // n >= 1

// the taps of a row of the coarse-by-fine band: the first fine voxel coarse voxel j gathers from (kPyrDownTaps of
// them), and the first coarse voxel fine voxel x gathers from (kPyrUpTaps); x, j >= 0
LAGO_PY_HD int pyr_down_first(int j) { return 2 * j - 2; }
LAGO_PY_HD int pyr_up_first(int x) { return (x >> 1) - 1; }

struct PyrReduce {   // R[j][x] of an axis of n fine voxels; any j, x: 0 outside the matrix
    template <typename R>
    static LAGO_PY_HD R at(int j, int x, int n) {
        if (j < 0 || x < 0 || x >= n || 2 * j > n - 1) return (R)0;
        int sixteenths = 0;
        for (int k = -2; k <= 2; ++k)
            if (pyr_clamp(2 * j + k, n) == x) sixteenths += k == 0 ? 6 : (k == -1 || k == 1) ? 4 : 1;
        return (R)sixteenths * (R)0.0625;
    }
};

struct PyrExpand {   // E[x][j], addressed (j, x, n) like R
    template <typename R>
    static LAGO_PY_HD R at(int j, int x, int n) {
        if (j < 0 || x < 0 || x >= n || 2 * j > n - 1) return (R)0;
        if ((x & 1) == 0) return x == 2 * j ? (R)1 : (R)0;
        const int m = (n + 1) / 2, j0 = x >> 1, j1 = j0 + 1 < m ? j0 + 1 : m - 1;
        return (R)((j == j0) + (j == j1)) * (R)0.5;
    }
};

// tap k (0..4) of coarse voxel j, tap t (0..2) of fine voxel x: the entry, exactly 0 for a tap outside the axis
template <typename R, typename W>
LAGO_PY_HD R pyr_down_weight(int j, int k, int n) { return W::template at<R>(j, pyr_down_first(j) + k, n); }
template <typename R, typename W>
LAGO_PY_HD R pyr_up_weight(int x, int t, int n) { return W::template at<R>(pyr_up_first(x) + t, x, n); }

// one contraction: taps ascending, a product and an addition per tap (no fma)
template <int TAPS, typename R, typename Val>
LAGO_PY_HD R pyr_dot(const R *w, Val val) {
    R acc = w[0] * val(0);
    for (int t = 1; t < TAPS; ++t) {
        const R p = w[t] * val(t);
        acc = acc + p;
    }
    return acc;
}

template <typename R>
LAGO_PY_HD R pyr_scale(R acc, double scale) { return (R)scale * acc; }

}  // namespace lago
