// The per-line arithmetic of distance_transform (edt.hip): which voxels are features, the candidate a source voxel
// offers a target voxel of its line, and the minimum over the candidates.  Plain C++ that a host compiler builds as
// well (tests/native/edt_emul.cpp runs it against the numpy reference tests/edt_ref.py).  Everything is float32, in
// exactly the order written; the library and the emulation are built with -ffp-contract=off, so nothing is fused.
//
//   feature : LAGO_EDT_NONZERO  L != 0        LAGO_EDT_EQUAL  L == label        LAGO_EDT_NOT_EQUAL  L != label
//             LAGO_EDT_SURFACE  L == label and one of the 2 dim face neighbours != label; a neighbour outside the
//             volume counts as different.  The neighbour's index is clamped into the axis BEFORE it is used, so the
//             load is inside the volume whether or not its value matters.  A 2D map has no first axis: nx = 1 there
//             and dim = 2 says that its two "neighbours" do not exist (a 3D map with nx = 1 has them, both outside).
//   g0      : 0 on a feature, +inf elsewhere (the first pass's input, formed as the line is loaded)
//   cand    : g[j] + t * t, t = s * float(i - j).  Every term is >= 0 or +inf: no cancellation, never inf - inf, no NaN
//   out[i]  : min over j.  At s = 1 every value is an integer below 2^24 (3 * 1023^2 < 2^24) or +inf, so each sum is
//             exact and the minimum does not depend on the order it is taken in.
//
// A lane owns EDT_BLOCK consecutive outputs of one line, so that one read of g[j] serves all of them (EdtBlock);
// edt_line is the same walk over a whole line on the host.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LAGO_EDT_HD __host__ __device__ __forceinline__
#define LAGO_EDT_UNROLL _Pragma("unroll")   // the output block must stay in registers on the device
#else
#define LAGO_EDT_HD inline
#define LAGO_EDT_UNROLL
#endif

#ifndef LAGO_EDT_NONZERO   // include/lagomorph_hip.h has them; repeated so that this file stands alone on the host
#define LAGO_EDT_NONZERO 0
#define LAGO_EDT_EQUAL 1
#define LAGO_EDT_NOT_EQUAL 2
#define LAGO_EDT_SURFACE 3
#endif

namespace lago {

constexpr int EDT_BLOCK = 8;   // outputs of one line a lane holds
constexpr int EDT_MAX_EXTENT = 1024;

// does the neighbour of voxel a at a + d along an axis of extent n (element stride `stride`) differ from `label`?
// `at` points at the voxel itself.
LAGO_EDT_HD bool edt_differs(const int32_t *at, int a, int d, int n, int64_t stride, int32_t label) {
    const int b = a + d;
    const int c = b < 0 ? 0 : (b > n - 1 ? n - 1 : b);   // inside the axis for every a in [0, n)
    const int32_t v = at[(int64_t)(c - a) * stride];
    return c != b || v != label;
}

// Is voxel (x, y, z) of the volume Lv (nx, ny, nz), last axis fastest, a feature?  dim 2: nx = 1, x = 0.
LAGO_EDT_HD bool edt_feature(const int32_t *Lv, int where, int32_t label, int dim, int x, int y, int z, int nx, int ny, int nz) {
    const int32_t *at = Lv + ((int64_t)x * ny + y) * nz + z;
    const int32_t v = *at;
    if (where == LAGO_EDT_NONZERO) return v != 0;
    if (where == LAGO_EDT_EQUAL) return v == label;
    if (where == LAGO_EDT_NOT_EQUAL) return v != label;
    if (v != label) return false;
    bool edge = edt_differs(at, z, -1, nz, 1, label) || edt_differs(at, z, 1, nz, 1, label) ||
                edt_differs(at, y, -1, ny, nz, label) || edt_differs(at, y, 1, ny, nz, label);
    if (dim == 3)
        edge = edge || edt_differs(at, x, -1, nx, (int64_t)ny * nz, label) || edt_differs(at, x, 1, nx, (int64_t)ny * nz, label);
    return edge;
}

LAGO_EDT_HD float edt_g0(bool feature) { return feature ? 0.0f : __builtin_inff(); }

// the cost of an offset of d voxels, d = float(i - j) (exact): t t with t = s d
LAGO_EDT_HD float edt_cost(float s, float d) {
    const float t = s * d;
    return t * t;
}

LAGO_EDT_HD float edt_min(float a, float b) { return __builtin_fminf(a, b); }   // (no operand is ever a NaN)

// The EDT_BLOCK targets i0 ... i0 + EDT_BLOCK - 1 of one line against its sources in ascending order.  cost[r] is the
// cost of target i0 + r against the CURRENT source j; the next source is one voxel further, so its costs are these moved
// up by one target, and only the cost of target i0 is formed anew: 3 operations a source for the costs and 2 a candidate
// (add, min), where forming every candidate's cost from its own offset took 5 a candidate.  The values are the same:
// cost[r] is always edt_cost(s, float(i0 + r - j)), whichever way it got there.  With the walk unrolled EDT_BLOCK times
// the moves are renamings of registers.
struct EdtBlock {
    float acc[EDT_BLOCK], cost[EDT_BLOCK];
    float d;   // float(i0 - j) of the current source
    LAGO_EDT_HD void start(float s, int i0) {   // before source 0
        d = (float)i0;
        LAGO_EDT_UNROLL
        for (int r = 0; r < EDT_BLOCK; ++r) {
            acc[r] = __builtin_inff();
            cost[r] = edt_cost(s, d + (float)r);   // integers below 2^24: the sum is float(i0 + r) exactly
        }
    }
    LAGO_EDT_HD void source(float g, float s) {   // the current source offers g + cost; then on to the next one
        LAGO_EDT_UNROLL
        for (int r = 0; r < EDT_BLOCK; ++r) acc[r] = edt_min(acc[r], g + cost[r]);
        LAGO_EDT_UNROLL
        for (int r = EDT_BLOCK - 1; r > 0; --r) cost[r] = cost[r - 1];
        d -= 1.0f;
        cost[0] = edt_cost(s, d);
    }
};

// a whole line on the host: out[i] = min_j g[j] + (s (i - j))^2.  out may not alias g.
inline void edt_line(float *out, const float *g, int n, float s) {
    for (int i0 = 0; i0 < n; i0 += EDT_BLOCK) {
        EdtBlock b;
        b.start(s, i0);
        for (int j = 0; j < n; ++j) b.source(g[j], s);
        for (int r = 0; r < EDT_BLOCK && i0 + r < n; ++r) out[i0 + r] = b.acc[r];
    }
}

}  // namespace lago
