// mutual information: the Parzen-window joint histogram of two (rows, nx, ny[, nz]) fields and its backward -- gfx950 HIP
// kernels.  No counterpart in the reference.  The per-voxel arithmetic (cubic B-spline windows on both images, in double
// for both precisions) is mi_window.hpp; the entropies on the tiny (rows, B, B) table are left to the caller.
//
//   H[kI + a][kJ + b] += llrint(wI_a wJ_b 2^32)   a, b = 0..3, a signed 64-bit integer sum per bin
//   P = H / (nvox 2^32)
//   dI(x) = (sum_a wI_a'(I(x)) (sum_b wJ_b(J(x)) G[kI + a][kJ + b])) / nvox,  dJ the same with the roles swapped
//
//   mi_hist_kernel     the scheme of chunk_table.hpp with 16-byte loads, REP replicas of the B x B table of 64-bit
//                      counters and a reducer that writes P: every voxel adds its 16 fixed-point products with LDS
//                      integer atomics (a smooth image sends a whole wave to the same 16 bins: lanes 256 / REP apart
//                      share a replica).
//   mi_bwd_kernel      the row's G in LDS as doubles; a lane takes 8 bytes of I and J at a time, reads the 4 x 4
//                      window of G once per voxel and forms the sums for the outputs that are wanted.  A pure gather.
// The integer sum is associative: P has the same bits from call to call, for any chunking and any replica count, and
// equals a sequential sum integer for integer.  No global atomic, no memset.
#include "chunk_table.hpp"   // (and common.hpp)
#include "mi_window.hpp"

namespace lago {

constexpr int kMiChunkMin = 4096;            // voxels a histogram workgroup walks at least (16 a lane)
constexpr int kMiBwdChunk = 8192;            // voxels a backward workgroup takes (it stages B x B doubles first)
#ifndef LAGO_MI_MAX_REP
#define LAGO_MI_MAX_REP 8   // replicas of the table at most (A/B builds: LAGO_HIPCC_EXTRA="-DLAGO_MI_MAX_REP=2")
#endif
#ifndef LAGO_MI_BWD_VEC
#define LAGO_MI_BWD_VEC 8   // bytes of I and of J a backward lane takes at a time (A/B builds: 16 costs the float kernel 268 registers)
#endif

struct MiArgs { MiAxis aI, aJ; int B; RowChunks rc; };

extern __shared__ unsigned long long mi_smem[];

template <typename R, int REP>
__global__ __launch_bounds__(kBlock) void mi_hist_kernel(long long *slab, const R *I, const R *J, MiArgs p) {
    typedef R vec __attribute__((ext_vector_type(16 / sizeof(R))));
    constexpr int VW = 16 / sizeof(R);
    const int B = p.B, BB = B * B;
    tables_zero(mi_smem, BB, REP);
    const ChunkOfRow c = chunk_of_block(p.rc);
    const R *Ir = I + (size_t)c.row * p.rc.nvox, *Jr = J + (size_t)c.row * p.rc.nvox;
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
    const uint32_t mI = misalign<VW>(Ir + c.c0);
    chunk_walk<VW>(c.c0, c.n, mI == misalign<VW>(Jr + c.c0), mI, [&](uint32_t i) { add((double)Ir[i], (double)Jr[i]); }, [&](uint32_t i) {
        const vec x = *reinterpret_cast<const vec *>(Ir + i), y = *reinterpret_cast<const vec *>(Jr + i);
#pragma unroll
        for (int k = 0; k < VW; ++k) add((double)x[k], (double)y[k]);
    });
    tables_store(slab, mi_smem, BB, REP);
}

// what table_reduce_kernel does with a finished sum: P = H / denom, denom = (double)nvox * 2^32
struct MiFinish { double *P, denom; __device__ void operator()(size_t i, long long sum) const { P[i] = (double)sum / denom; } };

template <typename R, bool NEED_I, bool NEED_J>
__global__ __launch_bounds__(kBlock) void mi_bwd_kernel(R *dI, R *dJ, const double *G, const R *I, const R *J, MiArgs p) {
    constexpr int VW = LAGO_MI_BWD_VEC / sizeof(R) > 1 ? LAGO_MI_BWD_VEC / sizeof(R) : 1;
    typedef R vec __attribute__((ext_vector_type(VW)));
    const int B = p.B, BB = B * B;
    double *g = reinterpret_cast<double *>(mi_smem);
    const ChunkOfRow c = chunk_of_block(p.rc);
    for (int e = threadIdx.x; e < BB; e += kBlock) g[e] = G[(size_t)c.row * BB + e];
    __syncthreads();
    const size_t base = (size_t)c.row * p.rc.nvox;
    const R *Ir = I + base, *Jr = J + base;
    R *dIr = NEED_I ? dI + base : nullptr, *dJr = NEED_J ? dJ + base : nullptr;
    const double nv = (double)p.rc.nvox;
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
    const uint32_t mI = misalign<VW>(Ir + c.c0);
    const bool same = mI == misalign<VW>(Jr + c.c0) && (!NEED_I || mI == misalign<VW>(dIr + c.c0)) &&
                      (!NEED_J || mI == misalign<VW>(dJr + c.c0));
    chunk_walk<VW>(c.c0, c.n, same, mI, [&](uint32_t i) {
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
    p.rc.nvox = (uint32_t)v.nvox;
    return LAGO_OK;
}

template <typename R>
static int mi_histogram_impl(double *P, const R *I, const R *J, long long *scratch, int64_t scratch_tables, int bins,
                             double loI, double hiI, double loJ, double hiJ, int dim, int64_t rows, int64_t nx,
                             int64_t ny, int64_t nz, void *stream) {
    MiArgs p;
    const int rc = mi_check("mi_histogram", bins, loI, hiI, loJ, hiJ, dim, rows, nx, ny, nz, p);
    if (rc != LAGO_OK) return rc;
    if (rows == 0 || p.rc.nvox == 0) return LAGO_OK;
    if (!P || !I || !J || !scratch) return fail_invalid("mi_histogram: null pointer");
    const int BB = bins * bins;
    size_t sbytes;
    if (const int rc = plan_tables<long long>(p.rc, sbytes, "mi_histogram", BB, rows, p.rc.nvox, kMiChunkMin, scratch_tables); rc != kLaunchNow)
        return rc;
    const size_t ibytes = (size_t)rows * p.rc.nvox * sizeof(R), pbytes = (size_t)rows * BB * 8;
    if (any_overlap({{P, pbytes}, {scratch, sbytes}}, {{I, ibytes}, {J, ibytes}}))
        return fail_invalid("mi_histogram: P and scratch must not alias an input or each other");
    hipStream_t s = (hipStream_t)stream;
    // as many replicas of the table as 64 KB hold, eight at most: B <= 32 eight, B <= 45 four, else two
    const auto fits = [&](int r) { return r <= LAGO_MI_MAX_REP && (size_t)r * BB * 8 <= kTableLdsBytes; };
    const int rep = fits(8) ? 8 : (fits(4) ? 4 : 2);
    hipError_t e = hipSuccess;
    with_int<2, 4, 8>(rep, [&](auto REP) {
        e = launch(mi_hist_kernel<R, REP()>, dim3((uint32_t)rows * p.rc.chunks), dim3(kBlock), (size_t)REP() * BB * 8, s, scratch, I, J, p);
    });
    return reduce_tables("mi_histogram", e, s, p.rc, rows, BB, (const long long *)scratch, MiFinish{P, (double)p.rc.nvox * kMiOne});
}

template <typename R>
static int mi_backward_impl(R *dI, R *dJ, const double *G, const R *I, const R *J, int bins, double loI, double hiI,
                            double loJ, double hiJ, int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz,
                            void *stream) {
    MiArgs p;
    const int rc = mi_check("mi_backward", bins, loI, hiI, loJ, hiJ, dim, rows, nx, ny, nz, p);
    if (rc != LAGO_OK) return rc;
    if (rows == 0 || p.rc.nvox == 0 || (!dI && !dJ)) return LAGO_OK;
    if (!G || !I || !J) return fail_invalid("mi_backward: null pointer");
    p.rc = split_row(p.rc.nvox, (int64_t)1 << 30, kMiBwdChunk);
    const int BB = bins * bins;
    const uint64_t nb = (uint64_t)rows * p.rc.chunks;
    if (nb >= (1ull << 31)) return fail_invalid("mi_backward: bad extent");
    const size_t ibytes = (size_t)rows * p.rc.nvox * sizeof(R), gbytes = (size_t)rows * BB * 8;
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
    return lago::scratch_chunks(bins >= LAGO_MI_MIN_BINS && bins <= LAGO_MI_MAX_BINS, (int64_t)bins * bins * 8, rows, nvox, lago::kMiChunkMin);
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
