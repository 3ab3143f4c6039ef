// Free-form deformation (FFD): the uniform cubic B-spline of a control lattice at the voxels of a regular grid, one
// axis at a time -- as the kernels of ffd.hip use it, and as a plain host compiler builds it (tests/native/ffd_emul.cpp
// runs this header on the CPU against the numpy restatement, tests/ffd_ref.py).  Needs nothing but the language.
//
// One axis of extent n >= 1 with an integer spacing s >= 1, in voxels:
//
//   m    = (n - 1) / s + 4                 control points; point j sits at voxel (j - 1) s, so one point lies before the
//                                           grid and at least two at or beyond its last voxel
//   i    = x / s,  r = x % s               the cell of voxel x and its place in it
//   t    = (R)r / (R)s  in [0, 1)          ONE rounded division in the field's precision R
//   taps   i ... i + 3                      all inside [0, m - 1] by construction: no fold, no clamp
//   s'   = 1 - t
//   w    = (s'^3, p(s'), p(t), t^3) / 6    bspline_weights.hpp's expressions (bs_poly, the rounded sixth): every operation
//                                           a single +, - or * in R, so a numpy restatement gives the same bits
//
// The weights depend on r alone: a table of 4 s values per axis serves every voxel.  r = 0 gives t = 0 and
// w = (1, 4, 1, 0) / 6 with w_3 EXACTLY 0, so when (n - 1) % s == 0 the last control point weighs 0 at every voxel.
// Rounding: as bspline_weights.hpp derives, every weight is within 7.5 u (1 + O(u)) of the exact cubic at the SAME t.
#pragma once

#include <stdint.h>

#include "bspline_weights.hpp"

namespace lago {

constexpr int kFfdMaxSpacing = 32;

template <typename R>
struct FfdAxis {
    R t;      // r / s, rounded once
    R w[4];   // the weights of taps i ... i + 3 (sum 1)
};

// control points along an axis of n >= 1 voxels at spacing s >= 1
LAGO_BS_HD int64_t ffd_ctrl_extent(int64_t n, int64_t s) { return (n - 1) / s + 4; }

template <typename R>
LAGO_BS_HD FfdAxis<R> ffd_axis(int r, int s) {   // 0 <= r < s
    FfdAxis<R> A;
    const R t = (R)r / (R)s;
    A.t = t;
    const R sp = (R)1 - t;
    const R sixth = (R)(1.0 / 6.0);
    A.w[0] = ((sp * sp) * sp) * sixth;
    A.w[1] = bs_poly(sp) * sixth;
    A.w[2] = bs_poly(t) * sixth;
    A.w[3] = ((t * t) * t) * sixth;
    return A;
}

}  // namespace lago
