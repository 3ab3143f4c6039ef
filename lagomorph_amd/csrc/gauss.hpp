// What gauss.hip shares with the kernels built on its passes (lncc.hip): the tap and pass descriptors, the border rule,
// the tile plan, and a host entry that runs ONE axis pass of the existing kernels over a stack of rows.
#pragma once

#include "common.hpp"

namespace lago {

constexpr int kGaussMaxRadius = LAGO_GAUSS_MAX_RADIUS;
constexpr int kGaussTapSlots = kGaussMaxRadius + 4;   // w[0..r], zeros up to H + 3 <= 35
constexpr int kGaussLanes = 64;                       // gauss_s_kernel: lanes along the contiguous direction
constexpr int kGaussInFlight = 6;                     // staging: global loads a lane issues before it waits for the first

// Non-finite input: a staged value is multiplied with every tap of its lane's window, the zero taps beyond r included
// (the window is 2 H + 4 wide), so an inf or NaN reaches outputs up to H + 3 positions away along the filtered axis
// instead of r (0 * inf = NaN).  Finite fields are unaffected; a pass of radius 0 copies its values untouched.
//
// Sums are taken in double for both precisions.  A float32 product of a tap and a value is then exact and a pass returns
// the correctly rounded sum (up to 1e-16), so the error of a float32 result is the rounding of the stored intermediates,
// relative to THEIR size -- which matters where the filter cancels its input (a wide kernel on a short periodic axis
// returns the mean of the line, far smaller than the values).  (Assumed, not measured here: v_fma_f64 issues at the rate
// of the unpacked v_fma_f32 on gfx950.)
struct GaussTaps {
    double w[kGaussTapSlots];   // w[|k|] for |k| <= r (already rounded to the field's precision), 0 beyond
};

struct GaussPass {
    uint32_t n;          // extent of the filtered axis
    uint32_t inner;      // elements between neighbours along it (1 for the z pass)
    uint64_t outer;      // lines-of-lines: the tensor is (outer, n, inner)
    int r, H;            // radius, radius rounded up to a multiple of 4
    int wrap;            // 1: periodic, 0: zero outside
    uint32_t bias;       // a multiple of n, >= H: (index + bias) is never negative
    FastDiv dn;
    int final, accumulate;   // the last pass applies alpha and may add onto out
    // z pass: RT rows x one segment of ZS (a multiple of 4) outputs per workgroup
    uint32_t ZS, nseg, nzc, RT, pitch;
    FastDiv dseg, dzc, dpitch;
    int vec;             // 4-vector stores allowed (nz % 4 == 0, base 16-byte (32 for double) aligned)
    // strided pass: T (a multiple of 4) positions of the axis x 64 lanes per workgroup
    uint32_t T, nat, nit;
    FastDiv dat, dit;
};

template <typename R>
__device__ __forceinline__ uint32_t gauss_resolve(const GaussPass &p, int idx, bool &inside) {
    if (p.wrap) {
        const uint32_t u = (uint32_t)(idx + (int)p.bias);
        inside = true;
        return u - p.dn.div(u) * p.n;
    }
    inside = idx >= 0 && idx < (int)p.n;
    return inside ? (uint32_t)idx : 0u;
}

template <typename R>
static bool gauss_plan(GaussPass &p, int axis, int r, int mode, int64_t rows, const Geom &g, const R *out) {
    const int64_t ext[3] = {g.nx, g.ny, g.nz};
    p = GaussPass();
    p.n = (uint32_t)ext[axis];
    p.inner = axis == 2 ? 1u : axis == 1 ? (uint32_t)g.nz : (uint32_t)(g.ny * g.nz);
    p.outer = (uint64_t)rows * (axis == 2 ? (uint64_t)g.nx * g.ny : axis == 1 ? (uint64_t)g.nx : 1ull);
    p.r = r;
    p.H = (r + 3) & ~3;
    p.wrap = mode == LAGO_GAUSS_WRAP;
    p.bias = p.n * (uint32_t)((p.H + (int)p.n - 1) / (int)p.n);
    p.dn = FastDiv(p.n);
    if (axis == 2) {
        const uint32_t n4 = (p.n + 3u) & ~3u;
        p.ZS = n4 < 1024u ? n4 : 1024u;
        p.nseg = (p.n + p.ZS - 1) / p.ZS;
        p.nzc = p.ZS / 4;
        p.RT = kBlock / p.nzc;
        if (p.RT > 32) p.RT = 32;
        if (p.RT < 1) p.RT = 1;
        p.pitch = p.ZS + 2u * (uint32_t)p.H;
        p.dseg = FastDiv(p.nseg);
        p.dzc = FastDiv(p.nzc);
        p.dpitch = FastDiv(p.pitch);
        p.vec = p.n % 4 == 0 && (uintptr_t)out % (4 * sizeof(R)) == 0;
        const uint64_t nb = (p.outer + p.RT - 1) / p.RT * p.nseg;
        return nb < (1ull << 31);
    }
    const uint32_t tmax = sizeof(R) == 4 ? 64u : 32u;   // (T + 2 H) x 64 elements: at most 32 KiB (float) / 48 KiB (double) of LDS
    p.nat = (p.n + tmax - 1) / tmax;
    p.T = ((p.n + p.nat - 1) / p.nat + 3u) & ~3u;
    p.nat = (p.n + p.T - 1) / p.T;
    p.nit = (p.inner + kGaussLanes - 1) / kGaussLanes;
    p.dat = FastDiv(p.nat);
    p.dit = FastDiv(p.nit);
    const uint64_t nb = p.outer * p.nat * p.nit;
    return nb < (1ull << 31);
}

// the taps of one pass as the kernels take them: w_0 .. w_r of `half` rounded once to R, zeros beyond; the single tap 1
// for r == 0
template <typename R>
static void gauss_fill_taps(GaussTaps &t, int r, const double *half) {
    for (int k = 0; k < kGaussTapSlots; ++k) t.w[k] = 0.0;
    if (r == 0) t.w[0] = 1.0;
    for (int k = 0; k <= r; ++k)
        if (r > 0) t.w[k] = (double)(R)half[k];   // rounded once to the field's precision
}

// One pass of gauss_z_kernel / gauss_s_kernel (gauss.hip) along `axis` (0, 1, 2 of the (nx, ny, nz) geometry) with
// radius r > 0 over `rows` fields: dst = G_axis src, no factor, nothing added.  dst must not overlap src.  false: the
// launch does not fit a grid.  (Defined in gauss.hip for float and double; the launch error is left to the caller's
// finish_launch.)
template <typename R>
bool gauss_axis_pass(R *dst, const R *src, int axis, int r, const double *half, int mode, int64_t rows, const Geom &g,
                     hipStream_t s);

}  // namespace lago
