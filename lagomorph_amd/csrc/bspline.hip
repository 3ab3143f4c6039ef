// Cubic B-spline interpolation: the prefilter (samples -> coefficients, and its adjoint) and the 4^d-tap gather with
// its backward -- gfx950 HIP kernels.  No counterpart in the reference.
//
// Prefilter.  Per spatial axis of extent n > 1, axes in order, one launch each; c solves B c = f with B the
// (1, 4, 1) / 6 tridiagonal under a whole-sample mirror (rows (4, 2) / 6 and (2, 4) / 6 at the ends): pole
// z = sqrt(3) - 2, gain 6, one causal and one anticausal first-order recursion per line (bs_line below).  The first
// pass reads `in`, the later ones run in place on `out`: a line is read completely by the lane (or the workgroup) that
// owns it before any of it is written, and lines are disjoint, so no scratch tensor is needed.
//
//   bspline_prefilter_s_kernel   a strided axis (x, y; inner = elements between two samples of a line).  One lane per
//                                line, consecutive lanes on consecutive lines, so every global access of a wave is a
//                                coalesced row.  The lane keeps its line in an LDS column (element i of lane l at
//                                i * L + l: consecutive lanes on consecutive banks), four row loads in flight before
//                                their LDS stores; both sweeps run on the column and the anticausal one stores each
//                                finished coefficient straight to memory: one load and one store per element.
//   bspline_prefilter_z_kernel   the contiguous axis.  A workgroup stages Lr whole rows (one contiguous chunk) with
//                                coalesced loads into LDS rows of odd stride n | 1, lane r runs the recursion of row r
//                                (consecutive lanes an odd stride apart: no bank conflict), coalesced stores.
//   bspline_prefilter_g_kernel   lines longer than kBsStagedMax: one lane per line, in place through global memory
//                                (the causal sweep stores c+ to `out`, the anticausal one reads it back).  Slow --
//                                two loads and two stores per element, uncoalesced on the contiguous axis -- but
//                                every geometry works.
//
// The line tile L (Lr) is sized from n and the type so that several workgroups share a CU where the lines are short
// and one still fits where they are long: 256 x 64 lines x 8 B = 128 KiB for float64 at n = 256.
//
// Gather.  interp_bspline_fwd_kernel / interp_bspline_bwd_kernel: one lane per voxel, lanes along z, the block and
// grid mapping of interp_forward (locate).  The position i + dt u(i) is formed with interp_forward's expression
// (sample_pos), clamped to the grid's box, and bspline_weights.hpp gives cell, weights and folded tap indices once per
// voxel; the channel loop takes one wave-uniform plane at a time.  The sum has a fixed order (z innermost, then y,
// then x), so forward and d_u repeat bit for bit; d_C is a scatter of w g onto the 4^d folded taps with hardware float
// atomics onto a target the entry point zeroes on the stream: its last bits vary from call to call.  No tap index
// leaves [0, n - 1] for any position, finite or not.  Registers, LDS and occupancy are in DESIGN.md.
#include "common.hpp"
#include "bspline_weights.hpp"

namespace lago {

constexpr int kBsStagedMax = 256;              // longest line the LDS-staged passes take (both types)
constexpr size_t kBsLdsSmall = 40 * 1024;      // a tile up to this size leaves room for four workgroups per CU

// ------------------------------------------------------------------ prefilter

template <typename R> struct BsConst;
template <> struct BsConst<float> { static constexpr int horizon = 14; };    // |z|^14 = 9.8e-9  < 2^-25
template <> struct BsConst<double> { static constexpr int horizon = 29; };   // |z|^29 = 2.6e-17 < 2^-54

// One line.  src(i): sample i; mset / mget: where the causal sweep keeps c+; dst(i, c): the finished coefficient.
// adjoint (B^T = D B D^-1, D = diag(1/2, 1, ..., 1, 1/2)): the two end samples doubled on the way in and halved on the
// way out; for n <= 2 D is a multiple of the identity and nothing changes.
template <typename R, typename Src, typename MSet, typename MGet, typename Dst>
__device__ __forceinline__ void bs_line(int n, bool adjoint, Src src, MSet mset, MGet mget, Dst dst) {
    const R z = (R)-0.26794919243112270647;   // sqrt(3) - 2
    const bool ends = adjoint && n > 2;
    auto f = [&](int i) {
        const R v = src(i);
        return ends && (i == 0 || i == n - 1) ? v + v : v;
    };
    // causal start: sum_{k < 2n-2} z^k f[mirror k] / (1 - z^(2n-2)), cut after `horizon` terms where the rest is below
    // half an ulp (then the denominator is 1 to the same accuracy); Horner from the far end
    const int per = 2 * n - 2, nk = per < BsConst<R>::horizon ? per : BsConst<R>::horizon;
    R sum = (R)0, zp = (R)1;
    for (int k = nk - 1; k >= 0; --k) {
        sum = lg_fma(z, sum, f(k <= n - 1 ? k : per - k));
        zp *= z;
    }
    if (per <= BsConst<R>::horizon) sum = sum / ((R)1 - zp);   // zp = z^per
    R cp = (R)6 * sum, prev = cp;
    mset(0, cp);
    for (int i = 1; i < n; ++i) {
        prev = cp;
        cp = lg_fma(z, cp, (R)6 * f(i));
        mset(i, cp);
    }
    // anticausal: c[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]), c[i] = z (c[i+1] - c+[i])
    R c = (R)(-0.26794919243112270647 / (0.26794919243112270647 * 0.26794919243112270647 - 1.0)) * lg_fma(z, prev, cp);
    dst(n - 1, ends ? (R)0.5 * c : c);
    for (int i = n - 2; i >= 0; --i) {
        c = z * (c - mget(i));
        dst(i, ends && i == 0 ? (R)0.5 * c : c);
    }
}

// lines = outer * inner lines of one plane (row of the (rows, nvox) view), line l = (o, j): element i at
// (o * n + i) * inner + j.  Grid: bpp blocks per plane times the planes; blockDim.x = L lines per block.
template <typename R>
__global__ __launch_bounds__(256) void bspline_prefilter_s_kernel(R *out, const R *in, uint32_t nvox,
                                                                  uint32_t lines, uint32_t bpp, int n, uint32_t inner,
                                                                  FastDiv dinner, int adjoint) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bs_smem[];
    const uint32_t L = blockDim.x;
    R *col = reinterpret_cast<R *>(bs_smem) + threadIdx.x;
    const uint32_t row = blockIdx.x / bpp;   // uniform
    const uint32_t line = (blockIdx.x - row * bpp) * L + threadIdx.x;
    if (line >= lines) return;               // (no barrier below: a lane touches its own column and its own line only)
    const uint32_t o = dinner.div(line), j = line - o * inner;
    const size_t base = (size_t)row * nvox + (size_t)o * (uint32_t)n * inner + j;
    const R *src = in + base;
    R *dstp = out + base;
    int i = 0;
    for (; i + 4 <= n; i += 4) {   // four rows in flight
        const R a0 = src[(size_t)i * inner], a1 = src[(size_t)(i + 1) * inner], a2 = src[(size_t)(i + 2) * inner],
                a3 = src[(size_t)(i + 3) * inner];
        col[(uint32_t)i * L] = a0;
        col[(uint32_t)(i + 1) * L] = a1;
        col[(uint32_t)(i + 2) * L] = a2;
        col[(uint32_t)(i + 3) * L] = a3;
    }
    for (; i < n; ++i) col[(uint32_t)i * L] = src[(size_t)i * inner];
    bs_line<R>(n, adjoint != 0, [&](int q) { return col[(uint32_t)q * L]; }, [&](int q, R v) { col[(uint32_t)q * L] = v; },
               [&](int q) { return col[(uint32_t)q * L]; }, [&](int q, R v) { dstp[(size_t)q * inner] = v; });
}

// The contiguous axis: `rows` rows of n elements (all planes together), Lr rows per block.
template <typename R>
__global__ __launch_bounds__(256) void bspline_prefilter_z_kernel(R *out, const R *in, uint64_t rows, int n,
                                                                  int Lr, FastDiv dn, int adjoint) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bs_smem[];
    R *tile = reinterpret_cast<R *>(bs_smem);
    const uint32_t ld = (uint32_t)n | 1u;
    const uint64_t row0 = (uint64_t)blockIdx.x * (uint32_t)Lr;
    const uint32_t nr = rows - row0 < (uint64_t)Lr ? (uint32_t)(rows - row0) : (uint32_t)Lr;
    const uint32_t cnt = nr * (uint32_t)n;   // <= 256 * 256
    const R *src = in + row0 * (uint32_t)n;
    R *dstp = out + row0 * (uint32_t)n;
    for (uint32_t e = threadIdx.x; e < cnt; e += 256) {
        const uint32_t r = dn.div(e), c = e - r * (uint32_t)n;
        tile[r * ld + c] = src[e];
    }
    __syncthreads();   // every element of the block's rows is in LDS: from here on `in` is not read (in place is safe)
    if (threadIdx.x < nr) {
        R *my = tile + threadIdx.x * ld;
        bs_line<R>(n, adjoint != 0, [&](int q) { return my[q]; }, [&](int q, R v) { my[q] = v; }, [&](int q) { return my[q]; },
                   [&](int q, R v) { my[q] = v; });
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < cnt; e += 256) {
        const uint32_t r = dn.div(e), c = e - r * (uint32_t)n;
        dstp[e] = tile[r * ld + c];
    }
}

// Lines of any length, any axis: as the strided kernel without the LDS column.
template <typename R>
__global__ __launch_bounds__(256) void bspline_prefilter_g_kernel(R *out, const R *in, uint32_t nvox, uint32_t lines,
                                                                  uint32_t bpp, int n, uint32_t inner, FastDiv dinner,
                                                                  int adjoint) {
    const uint32_t row = blockIdx.x / bpp;
    const uint32_t line = (blockIdx.x - row * bpp) * 256u + threadIdx.x;
    if (line >= lines) return;
    const uint32_t o = dinner.div(line), j = line - o * inner;
    const size_t base = (size_t)row * nvox + (size_t)o * (uint32_t)n * inner + j;
    const R *src = in + base;
    R *dstp = out + base;   // the lane's own line: its stores are seen by its own later loads
    bs_line<R>(n, adjoint != 0, [&](int q) { return src[(size_t)q * inner]; }, [&](int q, R v) { dstp[(size_t)q * inner] = v; },
               [&](int q) { return dstp[(size_t)q * inner]; }, [&](int q, R v) { dstp[(size_t)q * inner] = v; });
}

// lines per block for a staged pass over lines that take n elements of LDS each
template <typename R>
static int bs_tile_lines(int n) {
    const size_t line = (size_t)n * sizeof(R);
    return 256 * line <= kBsLdsSmall ? 256 : 128 * line <= kBsLdsSmall ? 128 : 64;
}

template <typename R>
static int bspline_prefilter_impl(R *out, const R *in, int adjoint, int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz,
                                  void *stream) {
    Volume v;   // nvox * 8 < 2^32: one plane is addressed with 32-bit offsets
    if (const int rc = check_volume(v, "bspline_prefilter", dim, nx, ny, nz, kPlane29, {rows})) return rc;
    const int64_t nvox = v.nvox;
    if (rows == 0 || nvox == 0) return LAGO_OK;   // nothing to write
    if (rows >= (1ll << 31)) return fail_invalid("bspline_prefilter: 2^31 rows or more");
    if (!out || !in) return fail_invalid("bspline_prefilter: null pointer");
    const size_t bytes = (size_t)rows * (size_t)nvox * sizeof(R);
    if (overlaps(out, in, bytes)) return fail_invalid("bspline_prefilter: out must not overlap the input");
    // the launches' grids, before the first of them
    const int64_t ext[3] = {v.nx, v.ny, v.nz}, inner_of[3] = {v.ny * v.nz, v.nz, 1};
    for (int a = 0; a < 3; ++a) {
        if (ext[a] <= 1) continue;
        const int64_t lines = nvox / ext[a];
        const int64_t blocks = a == 2 && ext[a] <= kBsStagedMax ? (lines * rows + 63) / 64 : ((lines + 63) / 64) * rows;
        if (blocks >= (1ll << 31)) return fail_invalid("bspline_prefilter: too many lines for one launch");
    }
    hipStream_t s = (hipStream_t)stream;
    const R *src = in;
    for (int a = 0; a < 3; ++a) {
        const int n = (int)ext[a];
        if (n <= 1) continue;
        const uint32_t inner = (uint32_t)inner_of[a], lines = (uint32_t)(nvox / n);
        hipError_t e = hipSuccess;
        if (n > kBsStagedMax) {
            const uint32_t bpp = (lines + 255u) / 256u;
            e = launch(bspline_prefilter_g_kernel<R>, dim3(bpp * (uint32_t)rows), dim3(256), 0, s, out, src, (uint32_t)nvox, lines, bpp,
                       n, inner, FastDiv(inner), adjoint);
        } else if (a == 2) {
            const int Lr = bs_tile_lines<R>(n | 1);
            const uint64_t allrows = (uint64_t)lines * (uint64_t)rows;
            const size_t smem = (size_t)Lr * (size_t)(n | 1) * sizeof(R);
            e = launch(bspline_prefilter_z_kernel<R>, dim3((uint32_t)((allrows + Lr - 1) / Lr)), dim3(256), smem, s, out, src, allrows, n,
                       Lr, FastDiv((uint32_t)n), adjoint);
        } else {
            const int L = bs_tile_lines<R>(n);
            const uint32_t bpp = (lines + L - 1) / L;
            e = launch(bspline_prefilter_s_kernel<R>, dim3(bpp * (uint32_t)rows), dim3(L), (size_t)L * n * sizeof(R), s, out, src,
                       (uint32_t)nvox, lines, bpp, n, inner, FastDiv(inner), adjoint);
        }
        if (e != hipSuccess) return fail_hip(e, "bspline_prefilter");
        src = out;
    }
    if (src == in) LAGO_HIP_TRY(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, s));   // every extent is 1: the identity
    return finish_launch(s, "bspline_prefilter");
}

// ------------------------------------------------------------------ gather

// What one voxel needs: per axis the weights, and the taps as ELEMENT offsets into a channel plane -- xo[a] the start
// of slab k_x[a], yo[b] the start of row k_y[b] within a slab, the last axis' k the position in the row.  2D: (y, z).
template <typename R, int DIM>
struct BsTaps {
    BsAxis<R> ax[DIM];
    uint32_t xo[4], yo[4];
    bool nan;
    __device__ __forceinline__ void setup(const R *un, size_t nv, const Vox &v, double dt, const Geom &g) {
        if constexpr (DIM == 3) {
            bs_axis(sample_pos<R>(v.i, dt, un[0]), g.nx, ax[0]);
            bs_axis(sample_pos<R>(v.j, dt, un[nv]), g.ny, ax[1]);
            bs_axis(sample_pos<R>(v.k, dt, un[2 * nv]), g.nz, ax[2]);
            nan = ax[0].nan || ax[1].nan || ax[2].nan;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                xo[q] = (uint32_t)ax[0].k[q] * (uint32_t)(g.ny * g.nz);
                yo[q] = (uint32_t)ax[1].k[q] * (uint32_t)g.nz;
            }
        } else {
            bs_axis(sample_pos<R>(v.j, dt, un[0]), g.ny, ax[0]);
            bs_axis(sample_pos<R>(v.k, dt, un[nv]), g.nz, ax[1]);
            nan = ax[0].nan || ax[1].nan;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                xo[q] = 0;
                yo[q] = (uint32_t)ax[0].k[q] * (uint32_t)g.nz;
            }
        }
    }
    // the four taps of the row that starts at element r
    __device__ __forceinline__ void row(const R *__restrict__ plane, uint32_t r, R (&val)[4]) const {
        const int *kl = ax[DIM - 1].k;
#pragma unroll
        for (int c = 0; c < 4; ++c) val[c] = plane[r + (uint32_t)kl[c]];
    }
};

// w . v, ascending from the q = 0 product
template <typename R>
__device__ __forceinline__ R bs_dot4(const R (&w)[4], const R (&v)[4]) {
    R acc = w[0] * v[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) acc = lg_fma(w[q], v[q], acc);
    return acc;
}

// Register pressure (3D).  Left alone the compiler moves everything that does not depend on the channel out of the
// channel loop -- 64 tap offsets, and for the scatter 64 weights -- and issues all 64 gathers together: 250 to 500
// registers, spills in float64.  bs_slab(v) makes a slab's offset (weight) a value the compiler cannot see through, so
// the 16 offsets (weights) of a slab are formed from it where they are used, and bs_slab_fence() keeps the scheduler
// from pulling the next slab's gathers above this slab's sums.  Both change no value.
__device__ __forceinline__ void bs_slab_fence() { __builtin_amdgcn_sched_barrier(0); }
template <typename V>
__device__ __forceinline__ V bs_slab(V v) {
    asm volatile("" : "+v"(v));
    return v;
}

// GATHER = false exists in profiling builds only (lago_debug_bspline_gather(0), tools/time_bspline.py): the taps are
// not loaded -- positions, weights, sums and stores stay -- so the difference is the time of the 4^d gathers.
template <typename R, int DIM, bool BC, bool GATHER = true>
__global__ __launch_bounds__(kBlock) void interp_bspline_fwd_kernel(R *__restrict__ out, const R *__restrict__ C,
                                                                    const R *__restrict__ u, double dt, int nc, Geom g) {
    const Vox v = locate(g);
    if (!v.valid) return;
    const size_t nv = g.nvox;
    const R *Cn = BC ? C : C + (size_t)v.n * nc * nv;
    R *on = out + (size_t)v.n * nc * nv + v.s;
    BsTaps<R, DIM> T;
    T.setup(u + (size_t)v.n * DIM * nv + v.s, nv, v, dt, g);
    const R(&wy)[4] = T.ax[DIM - 2].w, (&wz)[4] = T.ax[DIM - 1].w;
    for (int c = 0; c < nc; ++c) {
        const R *plane = Cn + (size_t)c * nv;   // wave-uniform
        R sx[4];
#pragma unroll
        for (int a = 0; a < (DIM == 3 ? 4 : 1); ++a) {
            R sy[4];
            const uint32_t xa = DIM == 3 ? bs_slab(T.xo[a]) : 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                R val[4];
                if constexpr (GATHER) {
                    T.row(plane, xa + T.yo[b], val);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) val[q] = (R)(xa + T.yo[b] + (uint32_t)T.ax[DIM - 1].k[q]);   // WRONG results
                }
                sy[b] = bs_dot4(wz, val);
            }
            sx[a] = bs_dot4(wy, sy);
            if (DIM == 3) bs_slab_fence();
        }
        on[(size_t)c * nv] = DIM == 3 ? bs_dot4(T.ax[0].w, sx) : sx[0];
    }
}

template <typename R, int DIM, bool BC, bool NEED_C, bool NEED_U>
__global__ __launch_bounds__(kBlock) void interp_bspline_bwd_kernel(R *__restrict__ d_C, R *__restrict__ d_u,
                                                                    const R *__restrict__ go, const R *__restrict__ C,
                                                                    const R *__restrict__ u, double dt, int nc, Geom g) {
    const Vox v = locate(g);
    if (!v.valid) return;
    const size_t nv = g.nvox;
    const R *Cn = BC ? C : C + (size_t)v.n * nc * nv;
    R *dCn = BC ? d_C : d_C + (size_t)v.n * nc * nv;
    const R *gon = go + (size_t)v.n * nc * nv + v.s;
    BsTaps<R, DIM> T;
    T.setup(u + (size_t)v.n * DIM * nv + v.s, nv, v, dt, g);
    const R(&wy)[4] = T.ax[DIM - 2].w, (&wz)[4] = T.ax[DIM - 1].w;
    R dw[DIM][4];
    R acc[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        acc[a] = (R)0;
        if (NEED_U) bs_dweights(T.ax[a], dw[a]);
    }
    const R(&dwy)[4] = dw[DIM - 2], (&dwz)[4] = dw[DIM - 1];
    const int *kl = T.ax[DIM - 1].k;
    for (int c = 0; c < nc; ++c) {
        const R gc = gon[(size_t)c * nv];
        if (NEED_U) {
            const R *plane = Cn + (size_t)c * nv;
            R s0[4], s1[4], s2[4];   // per x tap: value, d/dy and d/dz of the (y, z) sum
#pragma unroll
            for (int a = 0; a < (DIM == 3 ? 4 : 1); ++a) {
                R r0[4], r1[4];
                const uint32_t xa = DIM == 3 ? bs_slab(T.xo[a]) : 0u;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    R val[4];
                    T.row(plane, xa + T.yo[b], val);
                    r0[b] = bs_dot4(wz, val);
                    r1[b] = bs_dot4(dwz, val);
                }
                s0[a] = bs_dot4(wy, r0);
                s1[a] = bs_dot4(dwy, r0);
                s2[a] = bs_dot4(wy, r1);
                if (DIM == 3) bs_slab_fence();
            }
            R gr[DIM];
            if constexpr (DIM == 3) {
                gr[0] = bs_dot4(dw[0], s0);
                gr[1] = bs_dot4(T.ax[0].w, s1);
                gr[2] = bs_dot4(T.ax[0].w, s2);
            } else {
                gr[0] = s1[0];
                gr[1] = s2[0];
            }
#pragma unroll
            for (int a = 0; a < DIM; ++a) acc[a] = c == 0 ? gr[a] * gc : lg_fma(gr[a], gc, acc[a]);
        }
        if (NEED_C && !T.nan) {   // a NaN position adds nothing
            R *dCc = dCn + (size_t)c * nv;
#pragma unroll
            for (int a = 0; a < (DIM == 3 ? 4 : 1); ++a) {
                const uint32_t xa = DIM == 3 ? bs_slab(T.xo[a]) : 0u;
                const R wa = DIM == 3 ? bs_slab(T.ax[0].w[a]) : (R)1;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const R wab = DIM == 3 ? wa * wy[b] : wy[b];   // (w_x w_y) w_z; 2D: w_y w_z
#pragma unroll
                    for (int q = 0; q < 4; ++q) atomic_add(dCc + (xa + T.yo[b] + (uint32_t)kl[q]), (wab * wz[q]) * gc);
                }
                if (DIM == 3) bs_slab_fence();
            }
        }
    }
    if (NEED_U) {
        R *dun = d_u + (size_t)v.n * DIM * nv + v.s;
        const R rdt = (R)dt;
#pragma unroll
        for (int a = 0; a < DIM; ++a)   // exactly zero where the clamp removed the dependence; NaN for a NaN position
            dun[(size_t)a * nv] = T.nan ? (R)__builtin_nan("") : T.ax[a].clamped ? (R)0 : rdt * acc[a];
    }
}

#ifdef LAGO_PROFILING
static std::atomic<int> g_bs_dbg_gather{1};
#endif

// The checks the two gather entry points share, before any device call.  LAGO_OK with `empty` set: nothing to do.
static int bspline_geom(const char *what, Geom &g, Volume &v, bool &empty, int dim, int64_t nn, int64_t nc, int64_t nx,
                        int64_t ny, int64_t nz, bool scatter) {
    if (const int rc = check_volume(v, what, dim, nx, ny, nz, kPlane29, {nn, nc})) return rc;
    if (nc > INT_MAX) return fail_invalid("%s: 2^31 channels or more", what);
    empty = nn == 0 || nc == 0 || v.nvox == 0;
    if (!empty && !make_geom(g, v, nn, kBlock, scatter)) return fail_invalid("%s: bad extent", what);
    return LAGO_OK;
}

template <typename R>
static int interp_bspline_impl(R *out, const R *C, const R *u, double dt, int dim, int64_t nn, int64_t nc, int64_t nx,
                               int64_t ny, int64_t nz, int bc, void *stream) {
    Geom g;
    Volume v;
    bool empty;
    if (const int rc = bspline_geom("interp_bspline", g, v, empty, dim, nn, nc, nx, ny, nz, false)) return rc;
    if (empty) return LAGO_OK;   // nothing to write
    const GatherBytes b(sizeof(R), sizeof(R), dim, nn, nc, v.nvox, v.nvox, bc);
    if (const int rc = check_gather("interp_bspline", out, C, u, b); rc != kLaunchNow) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    with_dim(dim, [&](auto DIM) {
        with_flags([&](auto BC) {
#ifdef LAGO_PROFILING
            if (!g_bs_dbg_gather) {
                e = launch(interp_bspline_fwd_kernel<R, DIM(), BC(), false>, dim3(g.nblocks), dim3(kBlock), 0, s, out, C, u, dt, (int)nc, g);
                return;
            }
#endif
            e = launch(interp_bspline_fwd_kernel<R, DIM(), BC()>, dim3(g.nblocks), dim3(kBlock), 0, s, out, C, u, dt, (int)nc, g);
        }, bc != 0);
    });
    return launched(e, s, "interp_bspline");
}

template <typename R>
static int interp_bspline_backward_impl(R *d_C, R *d_u, const R *go, const R *C, const R *u, double dt, int dim, int64_t nn,
                                        int64_t nc, int64_t nx, int64_t ny, int64_t nz, int bc, int need_C, int need_u,
                                        void *stream) {
    Geom g;
    Volume v;
    bool empty;
    if (const int rc = bspline_geom("interp_bspline_backward", g, v, empty, dim, nn, nc, nx, ny, nz, need_C != 0)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const GatherBytes b(sizeof(R), sizeof(R), dim, nn, nc, v.nvox, v.nvox, bc);
    const int rc = check_gather_backward("interp_bspline_backward", d_C, d_u, go, C, u, b, need_C != 0, need_u != 0, empty, s);
    if (rc != kLaunchNow) return rc;
    hipError_t e = hipSuccess;
    with_dim(dim, [&](auto DIM) {
        with_flags([&](auto BC, auto NEED_C, auto NEED_U) {
            if constexpr (NEED_C() || NEED_U())   // (neither: the call was done above)
                e = launch(interp_bspline_bwd_kernel<R, DIM(), BC(), NEED_C(), NEED_U()>, dim3(g.nblocks), dim3(kBlock), 0, s, d_C,
                           d_u, go, C, u, dt, (int)nc, g);
        }, bc != 0, need_C != 0, need_u != 0);
    });
    return launched(e, s, "interp_bspline_backward");
}

}  // namespace lago

#ifdef LAGO_PROFILING
extern "C" void lago_debug_bspline_gather(int on) { lago::g_bs_dbg_gather = on; }
#endif

extern "C" {
#define LAGO_DEFINE(REAL, SUF)                                                                                           \
    int lago_bspline_prefilter##SUF(REAL *out, const REAL *in, int adjoint, int dim, int64_t rows, int64_t nx,           \
                                    int64_t ny, int64_t nz, void *stream) {                                              \
        return lago::bspline_prefilter_impl<REAL>(out, in, adjoint, dim, rows, nx, ny, nz, stream);                      \
    }                                                                                                                    \
    int lago_interp_bspline##SUF(REAL *out, const REAL *C, const REAL *u, double dt, int dim, int64_t nn, int64_t nc,    \
                                 int64_t nx, int64_t ny, int64_t nz, int broadcast_C, void *stream) {                    \
        return lago::interp_bspline_impl<REAL>(out, C, u, dt, dim, nn, nc, nx, ny, nz, broadcast_C, stream);             \
    }                                                                                                                    \
    int lago_interp_bspline_backward##SUF(REAL *d_C, REAL *d_u, const REAL *grad_out, const REAL *C, const REAL *u,      \
                                          double dt, int dim, int64_t nn, int64_t nc, int64_t nx, int64_t ny,            \
                                          int64_t nz, int broadcast_C, int need_C, int need_u, void *stream) {           \
        return lago::interp_bspline_backward_impl<REAL>(d_C, d_u, grad_out, C, u, dt, dim, nn, nc, nx, ny, nz,           \
                                                        broadcast_C, need_C, need_u, stream);                            \
    }
LAGO_DEFINE(float, _f32)
LAGO_DEFINE(double, _f64)
#undef LAGO_DEFINE
}
