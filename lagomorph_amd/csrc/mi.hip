// mutual information: the Parzen-window joint histogram of two (rows, nx, ny[, nz]) fields and its backward -- gfx950 HIP
// kernels.  No counterpart in the reference.  The per-voxel arithmetic (cubic B-spline windows on both images, in double
// for both precisions) is mi_window.hpp; the entropies on the tiny (rows, B, B) table are left to the caller.
//
//   H[kI + a][kJ + b] += llrint(wI_a wJ_b 2^32)   a, b = 0..3, a signed 64-bit integer sum per bin
//   P = H / (nvox 2^32)
//   dI(x) = (sum_a wI_a'(I(x)) (sum_b wJ_b(J(x)) G[kI + a][kJ + b])) / nvox,  dJ the same with the roles swapped
//
//   mi_hist_kernel     grid rows x chunks: a workgroup walks its chunk of one row with 16-byte loads (scalar head and
//                      tail) and adds the 16 fixed-point products of every voxel into REP replicas of the B x B table in
//                      LDS with LDS integer atomics (a smooth image sends a whole wave to the same 16 bins: lanes
//                      256 / REP apart share a replica).  It then sums the replicas and writes its partial table with
//                      plain stores to the slab (rows, chunks, B, B).  Every slab entry is written: nothing is cleared.
//   mi_reduce_kernel   sums the chunks of each bin and writes P.
//   mi_bwd_kernel      the row's G in LDS as doubles; a lane takes 8 bytes of I and J at a time, reads the 4 x 4
//                      window of G once per voxel and forms the sums for the outputs that are wanted.  A pure gather.
//
// The integer sum is associative: P has the same bits from call to call, for any chunking and any replica count, and
// equals a sequential sum integer for integer.  No global atomic, no memset.
#include <initializer_list>

#include "common.hpp"
#include "mi_window.hpp"

namespace lago {

constexpr int kMiChunkMin = 4096;            // voxels a histogram workgroup walks at least (16 a lane)
constexpr int64_t kMiSlabBytes = 8ll << 20;  // the partial tables of all rows stay below this (or one table a row)
constexpr int kMiBwdChunk = 8192;            // voxels a backward workgroup takes (it stages B x B doubles first)
constexpr size_t kMiLdsBytes = 64 * 1024;    // what the replicas of one workgroup may take
#ifndef LAGO_MI_MAX_REP
#define LAGO_MI_MAX_REP 8   // replicas of the table at most (A/B builds: LAGO_HIPCC_EXTRA="-DLAGO_MI_MAX_REP=2")
#endif
#ifndef LAGO_MI_BWD_VEC
#define LAGO_MI_BWD_VEC 8   // bytes of I and of J a backward lane takes at a time (A/B builds: 16 costs the float kernel 268 registers)
#endif

struct MiArgs {
    MiAxis aI, aJ;
    int B;
    uint32_t nvox;     // of one row
    uint32_t chunks;   // workgroups per row
    uint32_t chunk;    // voxels per workgroup
};

extern __shared__ unsigned long long mi_smem[];

// The walk both kernels share: voxels [c0, c0 + n) of one row as a scalar head up to the first vector boundary, vectors
// of VW elements (16 bytes in the histogram, LAGO_MI_BWD_VEC in the backward), and a scalar tail.  `mis`: the misalignment of every pointer involved, in elements; when they differ no
// vector is formed.  scalar(i) and vector(i) are given the voxel index within the row.
template <uint32_t VW, typename FS, typename FV>
__device__ __forceinline__ void mi_walk(uint32_t c0, uint32_t n, bool same, uint32_t mis, FS &&scalar, FV &&vector) {
    const uint32_t head = same ? min((VW - mis) % VW, n) : n;
    const uint32_t nvec = (n - head) / VW;
    const uint32_t tail = head + nvec * VW;
    for (uint32_t i = threadIdx.x; i < head; i += kBlock) scalar(c0 + i);
    for (uint32_t v = threadIdx.x; v < nvec; v += kBlock) vector(c0 + head + v * VW);
    for (uint32_t i = tail + threadIdx.x; i < n; i += kBlock) scalar(c0 + i);
}

template <uint32_t VW, typename R>
__device__ __forceinline__ uint32_t mi_misalign(const R *p) {   // in elements, against a vector of VW
    return (uint32_t)(((uintptr_t)p / sizeof(R)) % VW);
}

template <typename R, int REP>
__global__ __launch_bounds__(kBlock) void mi_hist_kernel(long long *slab, const R *I, const R *J, MiArgs p) {
    typedef R vec __attribute__((ext_vector_type(16 / sizeof(R))));
    constexpr int VW = 16 / sizeof(R);
    const int B = p.B, BB = B * B;
    for (int e = threadIdx.x; e < REP * BB; e += kBlock) mi_smem[e] = 0ull;
    __syncthreads();
    const uint32_t row = blockIdx.x / p.chunks, ch = blockIdx.x - row * p.chunks;   // uniform
    const uint32_t c0 = ch * p.chunk;
    const uint32_t n = c0 < p.nvox ? min(p.chunk, p.nvox - c0) : 0u;
    const R *Ir = I + (size_t)row * p.nvox, *Jr = J + (size_t)row * p.nvox;
    unsigned long long *tab = mi_smem + (threadIdx.x / (kBlock / REP)) * BB;
    auto add = [&](double vi, double vj) {
        double tI, tJ, wI[4], wJ[4];
        const int kI = mi_locate(vi, p.aI, B, tI), kJ = mi_locate(vj, p.aJ, B, tJ);
        mi_weights(tI, wI);
        mi_weights(tJ, wJ);
        unsigned long long *q = tab + kI * B + kJ;   // kI, kJ in [0, B - 4]: q[3 B + 3] is the table's last entry at most
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) atomicAdd(q + a * B + b, (unsigned long long)mi_fixed(wI[a], wJ[b]));
    };
    const uint32_t mI = mi_misalign<VW>(Ir + c0), mJ = mi_misalign<VW>(Jr + c0);
    mi_walk<VW>(c0, n, mI == mJ, mI, [&](uint32_t i) { add((double)Ir[i], (double)Jr[i]); }, [&](uint32_t i) {
        const vec x = *reinterpret_cast<const vec *>(Ir + i), y = *reinterpret_cast<const vec *>(Jr + i);
#pragma unroll
        for (int k = 0; k < VW; ++k) add((double)x[k], (double)y[k]);
    });
    __syncthreads();
    long long *out = slab + (size_t)blockIdx.x * BB;
    for (int e = threadIdx.x; e < BB; e += kBlock) {
        unsigned long long sum = mi_smem[e];
#pragma unroll
        for (int r = 1; r < REP; ++r) sum += mi_smem[r * BB + e];
        out[e] = (long long)sum;
    }
}

// One workgroup per 64 bins of one row (the last group of a row is ragged where B x B is no multiple of 64): lane
// (part, e) sums the chunks part, part + 4, ... of its bin with eight loads in flight, the four parts meet in LDS.
// denom = (double)nvox * 2^32.  An integer sum: the order does not show.
__global__ __launch_bounds__(kBlock) void mi_reduce_kernel(double *P, const long long *slab, uint32_t chunks, uint32_t BB,
                                                           uint32_t groups, double denom) {
    __shared__ long long part[4][64];
    const uint32_t row = blockIdx.x / groups, e = (blockIdx.x - row * groups) * 64 + (threadIdx.x & 63u);   // row: uniform
    const uint32_t p = threadIdx.x >> 6;
    long long sum = 0;
    if (e < BB) {
        const long long *s = slab + (size_t)row * chunks * BB + e;
#pragma unroll 8
        for (uint32_t c = p; c < chunks; c += 4) sum += s[(size_t)c * BB];
    }
    part[p][threadIdx.x & 63u] = sum;
    __syncthreads();
    if (p == 0 && e < BB) {
        const uint32_t t = threadIdx.x;
        P[(size_t)row * BB + e] = (double)(part[0][t] + part[1][t] + part[2][t] + part[3][t]) / denom;
    }
}

template <typename R, bool NEED_I, bool NEED_J>
__global__ __launch_bounds__(kBlock) void mi_bwd_kernel(R *dI, R *dJ, const double *G, const R *I, const R *J, MiArgs p) {
    constexpr int VW = LAGO_MI_BWD_VEC / sizeof(R) > 1 ? LAGO_MI_BWD_VEC / sizeof(R) : 1;
    typedef R vec __attribute__((ext_vector_type(VW)));
    const int B = p.B, BB = B * B;
    double *g = reinterpret_cast<double *>(mi_smem);
    const uint32_t row = blockIdx.x / p.chunks, ch = blockIdx.x - row * p.chunks;   // uniform
    for (int e = threadIdx.x; e < BB; e += kBlock) g[e] = G[(size_t)row * BB + e];
    __syncthreads();
    const uint32_t c0 = ch * p.chunk;
    const uint32_t n = c0 < p.nvox ? min(p.chunk, p.nvox - c0) : 0u;
    const size_t base = (size_t)row * p.nvox;
    const R *Ir = I + base, *Jr = J + base;
    R *dIr = NEED_I ? dI + base : nullptr, *dJr = NEED_J ? dJ + base : nullptr;
    const double nv = (double)p.nvox;
    auto one = [&](double vi, double vj, R &oi, R &oj) {
        double tI, tJ, wI[4], wJ[4], dw[4], m[4][4];
        const int kI = mi_locate(vi, p.aI, B, tI), kJ = mi_locate(vj, p.aJ, B, tJ);
        mi_weights(tI, wI);
        mi_weights(tJ, wJ);
        const double *q = g + kI * B + kJ;   // in the table for every value: mi_locate
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) m[a][b] = q[a * B + b];
        if (NEED_I) {
            mi_derivs(vi, tI, p.aI, dw);
            oi = (R)(mi_grad_sum<false>(dw, wJ, m) / nv);
        }
        if (NEED_J) {
            mi_derivs(vj, tJ, p.aJ, dw);
            oj = (R)(mi_grad_sum<true>(dw, wI, m) / nv);
        }
    };
    const uint32_t mI = mi_misalign<VW>(Ir + c0);
    const bool same = mI == mi_misalign<VW>(Jr + c0) && (!NEED_I || mI == mi_misalign<VW>(dIr + c0)) &&
                      (!NEED_J || mI == mi_misalign<VW>(dJr + c0));
    mi_walk<VW>(c0, n, same, mI, [&](uint32_t i) {
        R oi, oj;
        one((double)Ir[i], (double)Jr[i], oi, oj);
        if (NEED_I) dIr[i] = oi;
        if (NEED_J) dJr[i] = oj;
    }, [&](uint32_t i) {
        const vec x = *reinterpret_cast<const vec *>(Ir + i), y = *reinterpret_cast<const vec *>(Jr + i);
        vec oi, oj;
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            R a, b;
            one((double)x[k], (double)y[k], a, b);
            if (NEED_I) oi[k] = a;
            if (NEED_J) oj[k] = b;
        }
        if (NEED_I) *reinterpret_cast<vec *>(dIr + i) = oi;
        if (NEED_J) *reinterpret_cast<vec *>(dJr + i) = oj;
    });
}

// ---- host side

// what the two entry points check alike; nvox = 0: nothing to do (with LAGO_OK)
static int mi_check(const char *name, int bins, double loI, double hiI, double loJ, double hiJ, int dim, int64_t rows,
                    int64_t nx, int64_t ny, int64_t nz, MiArgs &p) {
    if (const int rc = check_dim(name, dim)) return rc;
    if (bins < LAGO_MI_MIN_BINS || bins > LAGO_MI_MAX_BINS)
        return fail_invalid("%s: bins must be in %d..%d, got %d", name, LAGO_MI_MIN_BINS, LAGO_MI_MAX_BINS, bins);
    p.B = bins;
    p.aI = mi_axis(loI, hiI, bins);
    p.aJ = mi_axis(loJ, hiJ, bins);
    for (const MiAxis *ax : {&p.aI, &p.aJ}) {
        // (a NaN bound fails the first comparison; s is not finite for a range wider or narrower than a double holds)
        if (!(ax->lo < ax->hi) || !(ax->hi - ax->lo <= 1.7976931348623157e308) || !(ax->lo >= -1.7976931348623157e308) ||
            !(ax->s > 0.0 && ax->s <= 1.7976931348623157e308))
            return fail_invalid("%s: a range needs finite bounds lo < hi with a finite bin scale, got (%g, %g)", name, ax->lo, ax->hi);
    }
    Volume v;
    if (const int rc = check_volume(v, name, dim, nx, ny, nz, kPlane30, {rows})) return rc;
    if (rows >= (1ll << 31)) return fail_invalid("%s: 2^31 rows or more", name);
    p.nvox = (uint32_t)v.nvox;
    return LAGO_OK;
}

// chunks per row and voxels per chunk (a multiple of four, no chunk empty) for at most `want` chunks of at least `least`
static void mi_split(MiArgs &p, int64_t want, int64_t least) {
    int64_t c = (p.nvox + least - 1) / least;
    c = c < want ? c : want;
    c = c < 1 ? 1 : c;
    int64_t per = (p.nvox + c - 1) / c;
    per = (per + 3) / 4 * 4;
    p.chunk = (uint32_t)per;
    p.chunks = (uint32_t)((p.nvox + per - 1) / per);
}

static int64_t mi_tables_wanted(int bins, int64_t rows, int64_t nvox) {
    const int64_t by_size = (nvox + kMiChunkMin - 1) / kMiChunkMin;
    const int64_t cap = kMiSlabBytes / ((int64_t)bins * bins * 8) / (rows > 1 ? rows : 1);
    const int64_t c = by_size < cap ? by_size : cap;
    return c < 1 ? 1 : c;
}

template <typename R>
static int mi_histogram_impl(double *P, const R *I, const R *J, long long *scratch, int64_t scratch_tables, int bins,
                             double loI, double hiI, double loJ, double hiJ, int dim, int64_t rows, int64_t nx,
                             int64_t ny, int64_t nz, void *stream) {
    MiArgs p;
    const int rc = mi_check("mi_histogram", bins, loI, hiI, loJ, hiJ, dim, rows, nx, ny, nz, p);
    if (rc != LAGO_OK) return rc;
    if (rows == 0 || p.nvox == 0) return LAGO_OK;
    if (!P || !I || !J || !scratch) return fail_invalid("mi_histogram: null pointer");
    if (scratch_tables < 1) return fail_invalid("mi_histogram: scratch must hold at least one table per row");
    const int64_t want = mi_tables_wanted(bins, rows, p.nvox);
    mi_split(p, want < scratch_tables ? want : scratch_tables, kMiChunkMin);
    const int BB = bins * bins;
    const uint64_t nb = (uint64_t)rows * p.chunks;
    const uint32_t groups = (uint32_t)((BB + 63) / 64);   // of the reducer
    if (nb >= (1ull << 31) || (uint64_t)rows * groups >= (1ull << 31)) return fail_invalid("mi_histogram: bad extent");
    const size_t ibytes = (size_t)rows * p.nvox * sizeof(R), sbytes = (size_t)nb * BB * 8, pbytes = (size_t)rows * BB * 8;
    if (any_overlap({{P, pbytes}, {scratch, sbytes}}, {{I, ibytes}, {J, ibytes}}))
        return fail_invalid("mi_histogram: P and scratch must not alias an input or each other");
    hipStream_t s = (hipStream_t)stream;
    // as many replicas of the table as 64 KB hold, eight at most: B <= 32 eight, B <= 45 four, else two
    const auto fits = [&](int r) { return r <= LAGO_MI_MAX_REP && (size_t)r * BB * 8 <= kMiLdsBytes; };
    const int rep = fits(8) ? 8 : (fits(4) ? 4 : 2);
    hipError_t e = hipSuccess;
    with_int<2, 4, 8>(rep, [&](auto REP) {
        e = launch(mi_hist_kernel<R, REP()>, dim3((uint32_t)nb), dim3(kBlock), (size_t)REP() * BB * 8, s, scratch, I, J, p);
    });
    if (e != hipSuccess) return fail_hip(e, "mi_histogram");
    e = launch(mi_reduce_kernel, dim3((uint32_t)rows * groups), dim3(kBlock), 0, s, P, (const long long *)scratch, p.chunks,
               (uint32_t)BB, groups, (double)p.nvox * kMiOne);
    return launched(e, s, "mi_histogram");
}

template <typename R>
static int mi_backward_impl(R *dI, R *dJ, const double *G, const R *I, const R *J, int bins, double loI, double hiI,
                            double loJ, double hiJ, int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz,
                            void *stream) {
    MiArgs p;
    const int rc = mi_check("mi_backward", bins, loI, hiI, loJ, hiJ, dim, rows, nx, ny, nz, p);
    if (rc != LAGO_OK) return rc;
    if (rows == 0 || p.nvox == 0 || (!dI && !dJ)) return LAGO_OK;
    if (!G || !I || !J) return fail_invalid("mi_backward: null pointer");
    mi_split(p, (int64_t)1 << 30, kMiBwdChunk);
    const int BB = bins * bins;
    const uint64_t nb = (uint64_t)rows * p.chunks;
    if (nb >= (1ull << 31)) return fail_invalid("mi_backward: bad extent");
    const size_t ibytes = (size_t)rows * p.nvox * sizeof(R), gbytes = (size_t)rows * BB * 8;
    if (any_overlap({{dI, ibytes}, {dJ, ibytes}}, {{I, ibytes}, {J, ibytes}, {G, gbytes}}))
        return fail_invalid("mi_backward: an output must not alias an input or the other output");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    with_flags([&](auto NEED_I, auto NEED_J) {
        if constexpr (NEED_I() || NEED_J())
            e = launch(mi_bwd_kernel<R, NEED_I(), NEED_J()>, dim3((uint32_t)nb), dim3(kBlock), (size_t)BB * 8, s, dI, dJ, G,
                       I, J, p);
    }, dI != nullptr, dJ != nullptr);
    return launched(e, s, "mi_backward");
}

}  // namespace lago

extern "C" {
int lago_mi_scratch_tables(int bins, int64_t rows, int64_t nvox) {
    if (bins < LAGO_MI_MIN_BINS || bins > LAGO_MI_MAX_BINS || rows < 0 || nvox < 0 || nvox > (1ll << 30)) return 1;
    return (int)lago::mi_tables_wanted(bins, rows, nvox);
}
#define LAGO_DEFINE(REAL, SUF)                                                                                      \
    int lago_mi_histogram##SUF(double *P, const REAL *I, const REAL *J, long long *scratch, int64_t scratch_tables, \
                               int bins, double loI, double hiI, double loJ, double hiJ, int dim, int64_t rows,    \
                               int64_t nx, int64_t ny, int64_t nz, void *stream) {                                 \
        return lago::mi_histogram_impl<REAL>(P, I, J, scratch, scratch_tables, bins, loI, hiI, loJ, hiJ, dim, rows, \
                                             nx, ny, nz, stream);                                                   \
    }                                                                                                               \
    int lago_mi_backward##SUF(REAL *dI, REAL *dJ, const double *G, const REAL *I, const REAL *J, int bins,         \
                              double loI, double hiI, double loJ, double hiJ, int dim, int64_t rows, int64_t nx,   \
                              int64_t ny, int64_t nz, void *stream) {                                              \
        return lago::mi_backward_impl<REAL>(dI, dJ, G, I, J, bins, loI, hiI, loJ, hiJ, dim, rows, nx, ny, nz,       \
                                            stream);                                                                \
    }
LAGO_DEFINE(float, _f32)
LAGO_DEFINE(double, _f64)
#undef LAGO_DEFINE
}
