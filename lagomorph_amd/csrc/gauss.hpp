// The Gaussian passes as gauss.hip and the kernels built on them (lncc.hip) share them: the tap and pass descriptors, the
// border rule, the tile plan, the parsing of the per-axis arguments, the grid and LDS size of a pass, a host entry that
// runs ONE axis pass over a stack of rows, and (device part) the sliding sum and the whole contiguous-axis pass --
// workgroup decomposition, staging, lane mapping -- of which gauss_z_kernel and lncc_moments_kernel are instantiations.
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

// dim, mode, radii and taps of the entry point `name`, as rad / tp per axis of the (nx, ny, nz) geometry (a 2D field is
// (1, H, W)).  `what` names the operation in the dim message, `wider` is what the radius message adds.  LAGO_OK or the
// reported failure.
static int gauss_parse_axes(const char *name, const char *what, const char *wider, int dim, int mode, const int *radii,
                            const double *taps, int (&rad)[3], const double *(&tp)[3]) {
    if (dim != 2 && dim != 3) return fail_invalid("Only two- and three-dimensional %s is supported", what);
    if (mode != LAGO_GAUSS_WRAP && mode != LAGO_GAUSS_ZERO) return fail_invalid("%s: unknown border mode %d", name, mode);
    if (!radii) return fail_invalid("%s: null radii", name);
    for (int a = 0; a < 3; ++a) {
        rad[a] = 0;
        tp[a] = nullptr;
    }
    for (int a = 0; a < dim; ++a) {
        const int r = radii[a];
        if (r < 0 || r > kGaussMaxRadius)
            return fail_invalid("%s: radius %d is outside 0..%d%s", name, r, kGaussMaxRadius, wider);
        if (r > 0 && !taps) return fail_invalid("%s: null taps", name);
        rad[a + 3 - dim] = r;
        tp[a + 3 - dim] = taps ? taps + (size_t)a * (kGaussMaxRadius + 1) : nullptr;
    }
    return LAGO_OK;
}

// workgroups of one pass and its dynamic LDS bytes; the z pass stages `fields` inputs side by side
template <typename R>
static uint32_t gauss_blocks(const GaussPass &p, int axis, int fields, size_t &smem) {
    if (axis == 2) {
        smem = (size_t)fields * p.RT * p.pitch * sizeof(R);
        return (uint32_t)((p.outer + p.RT - 1) / p.RT * p.nseg);
    }
    smem = (size_t)(p.T + 2u * (uint32_t)p.H) * kGaussLanes * sizeof(R);
    return (uint32_t)(p.outer * p.nat * p.nit);
}

// One pass of gauss_z_kernel / gauss_s_kernel (gauss.hip) for the entry point `name` along `axis` (0, 1, 2 of the
// (nx, ny, nz) geometry) with radius r > 0 over `rows` fields: dst = G_axis src, no factor, nothing added.  dst must not
// overlap src.  LAGO_OK or the reported failure (a launch that does not fit a grid is "bad extent").  (Defined in
// gauss.hip for float and double; an error of the launch itself is left to the caller's finish_launch.)
template <typename R>
int gauss_axis_pass(const char *name, R *dst, const R *src, int axis, int r, const double *half, int mode, int64_t rows,
                    const Geom &g, hipStream_t s);

}  // namespace lago

#if defined(__HIPCC__)
namespace lago {

extern __shared__ __attribute__((aligned(32))) unsigned char gauss_smem[];

// The sliding sum of one lane: four outputs of each of M moments from the 2 H + 4 staged positions of its window.
// load4(off, v) fetches the four positions off .. off + 3 of each of the NF staged fields, expand(in, x) forms the M
// summands of one position in double.  Output o sits at window position H + o, so position j carries tap j - H - o.
// Taps are wave-uniform (kernel arguments, uniform index).
template <typename R, int NF, int M, typename LOAD4, typename EXPAND>
__device__ __forceinline__ void gauss_slide(const GaussTaps &taps, int H, LOAD4 load4, EXPAND expand,
                                            double (&acc)[M][4]) {
    double t[7];   // taps of k0 - 3 .. k0 + 3 for the four positions at window offsets k0 .. k0 + 3 (relative to output 0)
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j + 4] = 0.0;   // k = -H-3 .. -H-1: beyond every radius
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[m][o] = 0.0;
    R v[NF][4];
    double in[NF], x[M];
    if (H == 0) {   // radius 0 (the copy pass): the summands themselves, no product with a zero tap (0 * inf), -0 kept
        load4(0, v);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
#pragma unroll
            for (int k = 0; k < NF; ++k) in[k] = (double)v[k][o];
            expand(in, x);
#pragma unroll
            for (int m = 0; m < M; ++m) acc[m][o] = x[m];
        }
        return;
    }
    const int steps = (2 * H + 4) >> 2;
    for (int s = 0; s < steps; ++s) {
        const int k0 = 4 * s - H;
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = t[j + 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + j;
            t[j + 3] = taps.w[k < 0 ? -k : k];
        }
        load4(4 * s, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int k = 0; k < NF; ++k) in[k] = (double)v[k][i];
            expand(in, x);
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int o = 0; o < 4; ++o) acc[m][o] = lg_fma(t[i - o + 3], x[m], acc[m][o]);
        }
    }
}

// The pass along the contiguous axis.  A workgroup stages RT row segments of ZS outputs plus halo of each of the NF
// input fields (field k at lds + k * RT * pitch; pitch = ZS + 2 H is a multiple of 4, so every 4-vector read below is
// aligned), the border rule applied while loading: all loads of a round are issued before its LDS stores.  A lane then
// owns four consecutive outputs at z0 of one row, slides over its window and hands the M x 4 sums to
// store(row, z0, acc), which rounds and writes them (whole 4-vectors where p.vec and z0 + 3 < n, masked scalars else).
template <typename R, int NF, int M, typename EXPAND, typename STORE>
__device__ __forceinline__ void gauss_z_pass(R *lds, const R *const (&in)[NF], const GaussTaps &taps, const GaussPass &p,
                                             EXPAND expand, STORE store) {
    typedef R vec4 __attribute__((ext_vector_type(4)));
    const uint32_t rb = p.dseg.div(blockIdx.x);
    const uint32_t seg = blockIdx.x - rb * p.nseg;
    const uint64_t row0 = (uint64_t)rb * p.RT;
    const int zs0 = (int)(seg * p.ZS);
    const int lo = p.H - p.r, hi = p.H + (int)p.ZS + p.r;   // staged positions outside [lo, hi) carry zero taps only
    const uint32_t staged = p.RT * p.pitch;
    for (uint32_t e0 = threadIdx.x; e0 < staged; e0 += kGaussInFlight * kBlock) {
        R val[NF][kGaussInFlight];
#pragma unroll
        for (int f = 0; f < kGaussInFlight; ++f) {
            const uint32_t e = e0 + (uint32_t)f * kBlock;
            const uint32_t rl = p.dpitch.div(e);
            const int q = (int)(e - rl * p.pitch);
            const uint64_t row = row0 + rl;
#pragma unroll
            for (int k = 0; k < NF; ++k) val[k][f] = (R)0;
            if (e < staged && row < p.outer && q >= lo && q < hi) {
                bool inside;
                const uint32_t u = gauss_resolve<R>(p, zs0 - p.H + q, inside);
                if (inside) {
#pragma unroll
                    for (int k = 0; k < NF; ++k) val[k][f] = in[k][row * p.n + u];
                }
            }
        }
#pragma unroll
        for (int f = 0; f < kGaussInFlight; ++f) {
            const uint32_t e = e0 + (uint32_t)f * kBlock;
            if (e < staged) {
#pragma unroll
                for (int k = 0; k < NF; ++k) lds[k * staged + e] = val[k][f];
            }
        }
    }
    __syncthreads();
    const uint32_t item = threadIdx.x;
    if (item >= p.RT * p.nzc) return;
    const uint32_t rl = p.dzc.div(item);
    const uint32_t c = item - rl * p.nzc;
    const uint64_t row = row0 + rl;
    const uint32_t z0 = (uint32_t)zs0 + 4u * c;
    if (row >= p.outer || z0 >= p.n) return;
    const R *win = lds + rl * p.pitch + 4u * c;
    double acc[M][4];
    gauss_slide<R, NF, M>(taps, p.H, [&](int off, R (&v)[NF][4]) {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            const vec4 x = *reinterpret_cast<const vec4 *>(win + k * staged + off);
            v[k][0] = x.x; v[k][1] = x.y; v[k][2] = x.z; v[k][3] = x.w;
        }
    }, expand, acc);
    store(row, z0, acc);
}

}  // namespace lago
#endif
