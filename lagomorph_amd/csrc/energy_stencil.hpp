// Diffusion and bending energy of a field, and the operator A of their quadratic forms E = <u, A u> / V: the arithmetic
// of ONE voxel -- as the kernels of energy.hip use it, and as a plain host compiler builds it
// (tests/native/energy_emul.cpp runs this header on the CPU against the numpy restatement, tests/energy_ref.py).  Needs
// nothing but the language.  The definition is in include/lagomorph_hip.h (lago_field_energy).
//
// A voxel reads its neighbours through `at(dx, dy, dz)`, the value at the voxel's coordinates plus the offsets, EACH
// COORDINATE CLAMPED to its axis [0, n - 1] (the kernels stage their LDS tile that way; offsets are within +-2).  The
// clamp is what makes the borders exact without a predicate on any first difference:
//
//   f_a(x)  = u(x + e_a) - u(x)                        0 at x_a = n_a - 1: the forward difference with its Neumann border
//   L_a(x)  = (u(x) - u(x - e_a)) - (u(x + e_a) - u(x))      = (D_a^T D_a u)(x) h_a^2, the Neumann Laplacian's negative
//   m_ab(x) = (u(x+e_a+e_b) - u(x+e_a)) - (u(x+e_b) - u(x))  0 wherever x_a + 1 = n_a or x_b + 1 = n_b: both brackets
//                                                            are then equal bit for bit (or both 0)
//   M_ab(x) = (L_a(x) - L_a(x - e_b)) + (L_a(x) - L_a(x + e_b))   = (D_ab^T D_ab u)(x) (h_a h_b)^2 = L_b L_a; a bracket
//                                                            whose neighbour is clamped is L_a(x) - L_a(x), exactly 0
//
// Only the second difference along one axis needs predicates, because its rows exist for 1 <= x_a <= n_a - 2 only; they
// are the numbers 0 and 1 in the field's precision (EnergyMask), multiplied in -- an exact product:
//
//   s(y)    = (u(y + e_a) - u(y)) - (u(y) - u(y - e_a))      row y of the second difference
//   B_a(x)  = (m s(x - e_a) - c s(x)) + (p s(x + e_a) - c s(x))   = (D_aa^T D_aa u)(x) h_a^4, with m, c, p = whether
//                                                            rows x_a - 1, x_a, x_a + 1 exist
//
// Weights (EnergyWeights, from the spacings in double, rounded once to the field's precision R):
//   diffusion  wa[a] = 1 / h_a^2                       bending  wa[a] = 1 / h_a^4,  wab[(a, b)] = 2 / (h_a^2 h_b^2)
// Sums (a fixed order; axes ascending x, y, z, then the pairs (x, y), (x, z), (y, z); dim 2 has y, z and (y, z) only):
//   diffusion  density = sum_a wa[a] (f_a f_a)          A u = sum_a wa[a] L_a
//   bending    density = sum_a wa[a] (s_a s_a) + sum_{a<b} wab (m_ab m_ab),   s_a = c s(x)
//              A u     = sum_a wa[a] B_a + sum_{a<b} wab M_ab
// acc = w_0 t_0; acc = acc + w_1 t_1; ...  Every operation is a single +, - or * in R: the library is built with
// -ffp-contract=off and nothing here is fused, so a numpy restatement gives the same bits.
//
// Roundings between u and (A u)(x), bending, dim 3, longest path: first difference, second difference, the bracket of
// B_a, their sum, the weight (itself rounded once), the product, five additions, the caller's scale: 12.  The kernels'
// float32 results are within K u sum |A| |u|, u = 2^-24, K = 13 for bending (12 and one for the second-order terms),
// K = 8 for diffusion (difference, L_a, weight, product, two additions, scale: 7) -- tests/test_gpu_energy.py.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LAGO_EN_HD __host__ __device__ __forceinline__
#else
#define LAGO_EN_HD inline
#endif

namespace lago {

constexpr int kEnergyDiffusion = 0, kEnergyBending = 1;   // LAGO_ENERGY_* of the header

template <typename R>
struct EnergyWeights {
    R wa[3];    // per axis (x, y, z)
    R wab[3];   // per pair (x, y), (x, z), (y, z); bending only
};

// h: the spacing of the axes (x, y, z) as laid out in memory (dim 2: h[0] is not used)
template <typename R>
LAGO_EN_HD EnergyWeights<R> energy_weights(int kind, const double *h) {
    EnergyWeights<R> w;
    double h2[3];
    for (int a = 0; a < 3; ++a) h2[a] = h[a] * h[a];
    for (int a = 0; a < 3; ++a) w.wa[a] = (R)(kind == kEnergyBending ? 1.0 / (h2[a] * h2[a]) : 1.0 / h2[a]);
    w.wab[0] = (R)(2.0 / (h2[0] * h2[1]));
    w.wab[1] = (R)(2.0 / (h2[0] * h2[2]));
    w.wab[2] = (R)(2.0 / (h2[1] * h2[2]));
    return w;
}

// whether the second-difference rows x - 1, x, x + 1 of an axis of extent n exist (rows 1 ... n - 2), as 0 or 1 in R
template <typename R>
struct EnergyMask {
    R m, c, p;
};
template <typename R>
LAGO_EN_HD EnergyMask<R> energy_mask(int x, int n) {
    EnergyMask<R> q;
    q.m = (R)((x >= 2 && x <= n - 1) ? 1 : 0);
    q.c = (R)((x >= 1 && x <= n - 2) ? 1 : 0);
    q.p = (R)((x >= 0 && x <= n - 3) ? 1 : 0);
    return q;
}

// the neighbour at offset i along axis A, at offsets (i, j) along the axes (A, B)
template <int A, typename At>
LAGO_EN_HD auto en_at1(At &at, int i) {
    if constexpr (A == 0) return at(i, 0, 0);
    else if constexpr (A == 1) return at(0, i, 0);
    else return at(0, 0, i);
}
template <int A, int B, typename At>
LAGO_EN_HD auto en_at2(At &at, int i, int j) {
    static_assert(A < B, "pairs are (x, y), (x, z), (y, z)");
    if constexpr (A == 0 && B == 1) return at(i, j, 0);
    else if constexpr (A == 0 && B == 2) return at(i, 0, j);
    else return at(0, i, j);
}

template <typename R, int A, typename At>
LAGO_EN_HD R en_forward(At &at, R u0) { return en_at1<A>(at, 1) - u0; }                       // f_a

template <typename R, int A, typename At>
LAGO_EN_HD R en_laplace(At &at, R u0) { return (u0 - en_at1<A>(at, -1)) - (en_at1<A>(at, 1) - u0); }   // L_a

template <typename R, int A, typename At>
LAGO_EN_HD R en_second(const EnergyMask<R> &q, At &at, R u0) {                                 // s_a = c s(x)
    return q.c * ((en_at1<A>(at, 1) - u0) - (u0 - en_at1<A>(at, -1)));
}

template <typename R, int A, int B, typename At>
LAGO_EN_HD R en_mixed(At &at, R u0) {                                                          // m_ab
    return (en_at2<A, B>(at, 1, 1) - en_at2<A, B>(at, 1, 0)) - (en_at2<A, B>(at, 0, 1) - u0);
}

// B_a; La receives L_a, which shares its first differences
template <typename R, int A, typename At>
LAGO_EN_HD R en_bend_axis(const EnergyMask<R> &q, At &at, R u0, R &La) {
    const R um2 = en_at1<A>(at, -2), um1 = en_at1<A>(at, -1), up1 = en_at1<A>(at, 1), up2 = en_at1<A>(at, 2);
    const R fm2 = um1 - um2, fm1 = u0 - um1, f0 = up1 - u0, f1 = up2 - up1;
    La = fm1 - f0;
    const R sm = q.m * (fm1 - fm2), s0 = q.c * (f0 - fm1), sp = q.p * (f1 - f0);
    return (sm - s0) + (sp - s0);
}

// M_ab from L_a at the voxel: L_a one step down and up axis B, then the two brackets
template <typename R, int A, int B, typename At>
LAGO_EN_HD R en_bend_pair(At &at, R La) {
    const R cm = en_at2<A, B>(at, 0, -1), cp = en_at2<A, B>(at, 0, 1);
    const R gm = (cm - en_at2<A, B>(at, -1, -1)) - (en_at2<A, B>(at, 1, -1) - cm);
    const R gp = (cp - en_at2<A, B>(at, -1, 1)) - (en_at2<A, B>(at, 1, 1) - cp);
    return (La - gm) + (La - gp);
}

// ---- the four per-voxel results.  q[a]: energy_mask of the voxel's coordinate on axis a (bending only)

template <typename R, int DIM, typename At>
LAGO_EN_HD R energy_diffusion_density(const EnergyWeights<R> &w, At &at) {
    const R u0 = at(0, 0, 0);
    R acc = (R)0;
    if constexpr (DIM == 3) {
        const R f = en_forward<R, 0>(at, u0);
        acc = w.wa[0] * (f * f);
    }
    const R fy = en_forward<R, 1>(at, u0), fz = en_forward<R, 2>(at, u0);
    if constexpr (DIM == 3) acc = acc + w.wa[1] * (fy * fy);
    else acc = w.wa[1] * (fy * fy);
    return acc + w.wa[2] * (fz * fz);
}

template <typename R, int DIM, typename At>
LAGO_EN_HD R energy_diffusion_apply(const EnergyWeights<R> &w, At &at) {
    const R u0 = at(0, 0, 0);
    R acc = (R)0;
    if constexpr (DIM == 3) acc = w.wa[0] * en_laplace<R, 0>(at, u0);
    const R ly = en_laplace<R, 1>(at, u0), lz = en_laplace<R, 2>(at, u0);
    if constexpr (DIM == 3) acc = acc + w.wa[1] * ly;
    else acc = w.wa[1] * ly;
    return acc + w.wa[2] * lz;
}

template <typename R, int DIM, typename At>
LAGO_EN_HD R energy_bending_density(const EnergyWeights<R> &w, const EnergyMask<R> *q, At &at) {
    const R u0 = at(0, 0, 0);
    R acc = (R)0;
    if constexpr (DIM == 3) {
        const R s = en_second<R, 0>(q[0], at, u0);
        acc = w.wa[0] * (s * s);
    }
    const R sy = en_second<R, 1>(q[1], at, u0), sz = en_second<R, 2>(q[2], at, u0);
    if constexpr (DIM == 3) acc = acc + w.wa[1] * (sy * sy);
    else acc = w.wa[1] * (sy * sy);
    acc = acc + w.wa[2] * (sz * sz);
    if constexpr (DIM == 3) {
        const R mxy = en_mixed<R, 0, 1>(at, u0), mxz = en_mixed<R, 0, 2>(at, u0);
        acc = acc + w.wab[0] * (mxy * mxy);
        acc = acc + w.wab[1] * (mxz * mxz);
    }
    const R myz = en_mixed<R, 1, 2>(at, u0);
    return acc + w.wab[2] * (myz * myz);
}

template <typename R, int DIM, typename At>
LAGO_EN_HD R energy_bending_apply(const EnergyWeights<R> &w, const EnergyMask<R> *q, At &at) {
    const R u0 = at(0, 0, 0);
    R Lx = (R)0, Ly, Lz, acc = (R)0;
    if constexpr (DIM == 3) acc = w.wa[0] * en_bend_axis<R, 0>(q[0], at, u0, Lx);
    const R By = en_bend_axis<R, 1>(q[1], at, u0, Ly), Bz = en_bend_axis<R, 2>(q[2], at, u0, Lz);
    if constexpr (DIM == 3) acc = acc + w.wa[1] * By;
    else acc = w.wa[1] * By;
    acc = acc + w.wa[2] * Bz;
    if constexpr (DIM == 3) {
        acc = acc + w.wab[0] * en_bend_pair<R, 0, 1>(at, Lx);
        acc = acc + w.wab[1] * en_bend_pair<R, 0, 2>(at, Lx);
    }
    (void)Lz;
    return acc + w.wab[2] * en_bend_pair<R, 1, 2>(at, Ly);
}

}  // namespace lago
