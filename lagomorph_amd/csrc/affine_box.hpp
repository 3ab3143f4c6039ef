// The candidate and ownership logic of affine_splat_box_kernel (affine.hip), as __host__ __device__ functions: the
// kernel calls them, and tests/native/affine_box_emul.hip walks whole grids through the same code on the CPU to check
// that every source voxel is inside the candidate range of the box that owns it (tests/test_affine_box_cover.py).
// A source whose owner does not list it is dropped from d_I: no other kernel picks it up.
//
// Everything that decides WHERE a box looks is double; everything that decides WHO owns a source is the reference's
// own position expression (cuda/affine.cu:42-61) in the input type R, so ownership is a partition whatever it rounds to.
#pragma once

#include "common.hpp"

namespace lago {

template <typename R>
__host__ __device__ __forceinline__ R half_extent(int n) {  // `.5*static_cast<Real>(n-1)`, cuda/affine.cu:42-43
    return (R)(.5 * (double)(R)(n - 1));
}

// The box [org, org + len) in position space: [lo, hi) per axis; a border box owns everything clamped onto it, i.e. it
// reaches to the image of the source grid (its eight corners) on that side, and two cells beyond.
template <typename R>
__host__ __device__ __forceinline__ void affine_box_interval(const R *An, const double (&Td)[3], const double (&od)[3],
                                                             const int (&ext)[3], const int (&org)[3], const int (&len)[3],
                                                             double (&lo)[3], double (&hi)[3]) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        lo[d] = (double)org[d];
        hi[d] = (double)(org[d] + len[d]);
    }
    double hmin[3] = {1e300, 1e300, 1e300}, hmax[3] = {-1e300, -1e300, -1e300};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const double f[3] = {((q & 4) ? ext[0] - 1 : 0) - od[0], ((q & 2) ? ext[1] - 1 : 0) - od[1], ((q & 1) ? ext[2] - 1 : 0) - od[2]};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double h = (double)An[3 * d] * f[0] + (double)An[3 * d + 1] * f[1] + (double)An[3 * d + 2] * f[2] + Td[d] + od[d];
            hmin[d] = h < hmin[d] ? h : hmin[d];
            hmax[d] = h > hmax[d] ? h : hmax[d];
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (org[d] == 0) lo[d] = fmin(lo[d], hmin[d] - 2.0);
        if (org[d] + len[d] == ext[d]) hi[d] = fmax(hi[d], hmax[d] + 2.0);
    }
}

// Bounding box [mn, mx] (source coordinates, no slack) of the preimage of [lo, hi) under h = A (x - o) + T + o.
__host__ __device__ __forceinline__ void affine_box_preimage(const double (&Ai)[9], const double (&Td)[3], const double (&od)[3],
                                                             const double (&lo)[3], const double (&hi)[3], double (&mn)[3],
                                                             double (&mx)[3]) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        mn[d] = 1e300;
        mx[d] = -1e300;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const double h[3] = {((q & 4) ? hi[0] : lo[0]) - Td[0] - od[0], ((q & 2) ? hi[1] : lo[1]) - Td[1] - od[1],
                             ((q & 1) ? hi[2] : lo[2]) - Td[2] - od[2]};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double x = Ai[3 * d] * h[0] + Ai[3 * d + 1] * h[1] + Ai[3 * d + 2] * h[2] + od[d];
            mn[d] = x < mn[d] ? x : mn[d];
            mx[d] = x > mx[d] ? x : mx[d];
        }
    }
}

// Slack per side of the candidate range, in source voxels, for what the position h, computed in R, is off from the
// exact affine map once the inverse carries it back into source space (the preimage itself is double).  NOT a whole
// voxel: a box of 8 x 8 x 48 cells then has about 1.45 instead of 2.0 candidates per owned voxel (-9 % on the kernel,
// profiles/r06_ab_box_slack.txt).
// What is known about it (profiles/affine_box_margin.md; tests/test_affine_box_cover.py walks this header on the host):
//  * Sources sit on integers and affine_box_candidates rounds the widened box OUTWARD (floor / ceil), so a source is
//    dropped exactly when it lies 1 + slack or more outside its owner's preimage box -- the slack alone is not the margin.
//  * Measured "needed slack" (distance outside the preimage box, before slack and rounding) over regular float32
//    matrices with entries of 500 .. 999.99 that cancel on in-grid sources, inverse row sums 3.5 .. 3.98, translations
//    aimed at every corner type of a box: at most 0.0356 voxels up to extent 512 (this function: 0.0251 there), 0.028
//    at 2048; mild matrices need none.  So the slack by itself IS exceeded by admissible matrices (the error of h is
//    not "six ulps of the extent", as an earlier comment argued: the products of the fma chain reach 1e3 n / 2 and
//    cancel), by a factor 1.4, and the outward rounding is what covers them, with a factor of about 29 to spare.
//  * No source was found uncovered.  The bound behind it: |h - exact| is a few ulps of (row sum |A| * n / 2 + |T|), times
//    an inverse row sum of at most 4 (affine_item_regular), to be kept below 1 voxel: fine for extents up to about a
//    thousand at entries near 1e3, and for any extent this library addresses at entries of order 1.
__host__ __device__ __forceinline__ double affine_box_slack(int nx, int ny, int nz) {
#ifdef LAGO_TEST_BOX_SLACK   // tests/test_affine_box_cover.py only: a deliberately wrong value, to see the walk notice
    return (double)(LAGO_TEST_BOX_SLACK);
#else
    const int m = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
    return 0.02 + 1e-5 * (double)m;
#endif
}

// Candidate sources s0 .. s1 (inclusive) per axis: the preimage box widened by the slack, inside the grid.
__host__ __device__ __forceinline__ void affine_box_candidates(const double (&mn)[3], const double (&mx)[3], double slack,
                                                               const int (&ext)[3], int (&s0)[3], int (&s1)[3]) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int a = (int)floor(fmax(mn[d] - slack, -1e9)), b = (int)ceil(fmin(mx[d] + slack, 1e9));
        s0[d] = a > 0 ? a : 0;
        s1[d] = b < ext[d] - 1 ? b : ext[d] - 1;
    }
}

// One source's position: cuda/affine.cu:42-61 (as affine_bwd_kernel), f = index - half extent.
template <typename R>
__host__ __device__ __forceinline__ void affine_box_position(const R *An, const R *Tn, R fi, R fj, R fk, R ox, R oy, R oz,
                                                             R &hx, R &hy, R &hz) {
    hx = lg_fma(An[2], fk, lg_fma(An[0], fi, An[1] * fj)) + Tn[0] + ox;
    hy = lg_fma(An[5], fk, lg_fma(An[3], fi, An[4] * fj)) + Tn[1] + oy;
    hz = lg_fma(An[8], fk, lg_fma(An[6], fi, An[7] * fj)) + Tn[2] + oz;
}

// Its floor cell (fx, fy, fz), the clamped cell relative to the box origin (lx, ly, lz; wraps for a cell below it) and
// whether the box [X0, X0 + ex) x ... owns it.
template <typename R>
__host__ __device__ __forceinline__ bool affine_box_owns(R hx, R hy, R hz, int nx, int ny, int nz, int X0, int Y0, int Z0,
                                                         int ex, int ey, int ez, int &fx, int &fy, int &fz, uint32_t &lx,
                                                         uint32_t &ly, uint32_t &lz) {
    fx = lg_floor(hx); fy = lg_floor(hy); fz = lg_floor(hz);
    lx = (uint32_t)(clamp1(fx, nx) - X0); ly = (uint32_t)(clamp1(fy, ny) - Y0); lz = (uint32_t)(clamp1(fz, nz) - Z0);
    return lx < (uint32_t)ex && ly < (uint32_t)ey && lz < (uint32_t)ez;   // else: another box owns it
}

}  // namespace lago
