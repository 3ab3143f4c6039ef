// gaussian_smooth: separable Gaussian filtering of (rows, nx, ny, nz) fields -- gfx950 HIP kernels.
//
// out = alpha * G_z G_y G_x in (+ out), each G_a a 1-D correlation with 2 r_a + 1 symmetric taps along one axis, the border
// either periodic ("wrap": indices modulo the extent, however large r_a is relative to it) or zero.  No counterpart in
// the reference.  One launch per axis with r_a > 0, ping-pong between `out` and ONE scratch tensor, taps by value in the
// kernel arguments, no atomics: every element is written once per pass by its own lane, from a sum in a fixed order.
//
// Both kernels stage a tile plus its halo in LDS with the border rule applied WHILE LOADING (a wrapped index or a zero),
// so the filter itself is a plain sliding sum over LDS (gauss_slide of gauss.hpp).  A lane owns four consecutive outputs
// along the filtered axis and walks its window of 2 H + 4 staged values (H = r rounded up to 4; taps beyond r are zero)
// four at a time: each staged value is read from LDS once per lane and feeds four fused multiply-adds, (2 H + 4) / 4 LDS
// reads per output instead of 2 r + 1.
//
//   gauss_z_kernel   the contiguous axis.  A workgroup stages RT whole row segments (RT x (ZS + 2 H)) with coalesced loads;
//                    a lane reads its window as aligned 4-vectors (lanes 16 / 32 bytes apart: conflict-free) and stores
//                    one 4-vector.  The pass itself is gauss_z_pass of gauss.hpp (one field, one sum; lncc.hip
//                    instantiates it with two and five): this kernel adds the alpha / accumulate store.
//   gauss_s_kernel   a strided axis (y: stride nz, x: stride ny nz).  Lanes run along the contiguous direction, so every
//                    global access is a coalesced 256-byte row; the workgroup stages a (T + 2 H) x 64 slab and a lane walks
//                    it down its own column (consecutive lanes, consecutive banks).
//
// A pass whose workgroups each stage the WHOLE extent of their lines (one z segment per row, one axis tile per column)
// reads everything it needs before its barrier and writes after it, and no other workgroup touches those lines: such a
// pass may run in place.  The three-pass accumulate form uses that (see gauss_impl).
#include "gauss.hpp"   // the descriptors, the plan, gauss_slide and gauss_z_pass: shared with lncc.hip

namespace lago {

template <typename R>
__device__ __forceinline__ R gauss_epilogue(const GaussPass &p, R alpha, double dsum, R prev) {
    const R sum = (R)dsum;
    if (!p.final) return sum;
    const R val = alpha * sum;
    return p.accumulate ? prev + val : val;   // (accumulate is set on the last pass only)
}

template <typename R>
__global__ __launch_bounds__(kBlock) void gauss_z_kernel(R *out, const R *in, GaussTaps taps, R alpha, GaussPass p) {
    typedef R vec4 __attribute__((ext_vector_type(4)));
    const R *const fields[1] = {in};
    gauss_z_pass<R, 1, 1>(reinterpret_cast<R *>(gauss_smem), fields, taps, p,
                          [](const double (&v)[1], double (&x)[1]) { x[0] = v[0]; },
                          [&](uint64_t row, uint32_t z0, const double (&acc)[1][4]) {
        R *o = out + row * p.n + z0;
        if (p.vec && z0 + 3u < p.n) {
            vec4 x = {(R)0, (R)0, (R)0, (R)0};
            if (p.accumulate) x = *reinterpret_cast<const vec4 *>(o);
            x.x = gauss_epilogue<R>(p, alpha, acc[0][0], x.x);
            x.y = gauss_epilogue<R>(p, alpha, acc[0][1], x.y);
            x.z = gauss_epilogue<R>(p, alpha, acc[0][2], x.z);
            x.w = gauss_epilogue<R>(p, alpha, acc[0][3], x.w);
            *reinterpret_cast<vec4 *>(o) = x;
            return;
        }
        R prev[4] = {(R)0, (R)0, (R)0, (R)0};
        if (p.accumulate) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (z0 + (uint32_t)k < p.n) prev[k] = o[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (z0 + (uint32_t)k < p.n) o[k] = gauss_epilogue<R>(p, alpha, acc[0][k], prev[k]);
    });
}

template <typename R>
__global__ __launch_bounds__(kBlock) void gauss_s_kernel(R *out, const R *in, GaussTaps taps, R alpha, GaussPass p) {
    R *lds = reinterpret_cast<R *>(gauss_smem);
    uint32_t b = blockIdx.x;
    uint32_t q1 = p.dit.div(b);
    const uint32_t it = b - q1 * p.nit;
    const uint32_t ot = p.dat.div(q1);
    const uint32_t at = q1 - ot * p.nat;
    const int a0 = (int)(at * p.T);
    const uint32_t lane = threadIdx.x & (kGaussLanes - 1), grp = threadIdx.x / kGaussLanes;
    const uint32_t ii = it * kGaussLanes + lane;
    const bool lane_ok = ii < p.inner;
    const size_t base = (size_t)ot * p.n * p.inner;   // (outer, n, inner): one line set
    const R *src = in + base;
    const uint32_t nrows = p.T + 2u * (uint32_t)p.H;
    const int lo = p.H - p.r, hi = p.H + (int)p.T + p.r;
    constexpr uint32_t kGroups = kBlock / kGaussLanes;
    for (uint32_t q0 = grp; q0 < nrows; q0 += kGaussInFlight * kGroups) {   // loads first, then the LDS stores
        R val[kGaussInFlight];
#pragma unroll
        for (int f = 0; f < kGaussInFlight; ++f) {
            const uint32_t q = q0 + (uint32_t)f * kGroups;
            val[f] = (R)0;
            if (q < nrows && lane_ok && (int)q >= lo && (int)q < hi) {
                bool inside;
                const uint32_t u = gauss_resolve<R>(p, a0 - p.H + (int)q, inside);
                if (inside) val[f] = src[(size_t)u * p.inner + ii];
            }
        }
#pragma unroll
        for (int f = 0; f < kGaussInFlight; ++f) {
            const uint32_t q = q0 + (uint32_t)f * kGroups;
            if (q < nrows) lds[q * kGaussLanes + lane] = val[f];
        }
    }
    __syncthreads();
    if (!lane_ok) return;
    R *dst = out + base;
    for (uint32_t c = grp; c < p.T / 4u; c += kGroups) {
        const uint32_t a = (uint32_t)a0 + 4u * c;
        if (a >= p.n) break;
        const R *win = lds + (size_t)(4u * c) * kGaussLanes + lane;
        double acc[1][4];
        gauss_slide<R, 1, 1>(taps, p.H, [&](int off, R (&v)[1][4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[0][i] = win[(off + i) * kGaussLanes];
        }, [](const double (&v)[1], double (&x)[1]) { x[0] = v[0]; }, acc);
        R *o = dst + (size_t)a * p.inner + ii;
        R prev[4] = {(R)0, (R)0, (R)0, (R)0};
        if (p.accumulate) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (a + (uint32_t)k < p.n) prev[k] = o[(size_t)k * p.inner];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (a + (uint32_t)k < p.n) o[(size_t)k * p.inner] = gauss_epilogue<R>(p, alpha, acc[0][k], prev[k]);
    }
}

// whether every workgroup of the pass stages the whole extent of its lines: the pass may then run in place
static bool gauss_whole_lines(const GaussPass &p, int axis) { return axis == 2 ? p.nseg == 1 : p.nat == 1; }

template <typename R>
static hipError_t gauss_launch(const GaussPass &p, int axis, R *dst, const R *src, const GaussTaps &taps, R alpha,
                               hipStream_t s) {
    size_t smem;
    const uint32_t nb = gauss_blocks<R>(p, axis, 1, smem);
    return launch(axis == 2 ? gauss_z_kernel<R> : gauss_s_kernel<R>, dim3(nb), dim3(kBlock), smem, s, dst, src, taps,
                  alpha, p);
}

template <typename R>
static int gauss_impl(R *out, const R *in, R *scratch, const int *radii, const double *taps, int mode, double alpha,
                      int accumulate, int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz, void *stream) {
    int rad[3];
    const double *tp[3];
    const int rc = gauss_parse_axes("gaussian_smooth", "gaussian smoothing", " (wider kernels: use the FFT operator)", dim,
                                    mode, radii, taps, rad, tp);
    if (rc != LAGO_OK) return rc;
    Geom g;
    if (!make_geom(g, dim, rows, nx, ny, nz)) return fail_invalid("gaussian_smooth: bad extent");
    if (g.nblocks == 0) return LAGO_OK;
    if (!out || !in) return fail_invalid("gaussian_smooth: null pointer");
    const size_t bytes = (size_t)rows * g.nvox * sizeof(R);
    if (overlaps(out, in, bytes)) return fail_invalid("gaussian_smooth: out must not alias in");

    // the passes, outermost axis first.  Three passes that accumulate onto `out` cannot use it as a stage: the middle
    // one runs in place on the scratch tensor, which needs a pass that stages whole lines (see the head of this file);
    // such a pass is moved to the middle whether or not this call accumulates
    int order[3], m = 0;
    for (int a = 0; a < 3; ++a)
        if (rad[a] > 0) order[m++] = a;
    GaussPass pass[3];
    GaussTaps tw[3];
    if (m == 0) {   // nothing to filter: the z pass with the single tap 1 is the copy / alpha / accumulate pass
        order[m++] = 2;
    }
    for (int i = 0; i < m; ++i) {
        const int a = order[i];
        if (!gauss_plan<R>(pass[i], a, rad[a], mode, rows, g, out)) return fail_invalid("gaussian_smooth: bad extent");
        gauss_fill_taps<R>(tw[i], rad[a], tp[a]);
    }
    if (m == 3) {   // (the same order with and without accumulate: the same sums, the same bits)
        int mid = -1;
        for (int i = 0; i < 3 && mid < 0; ++i)
            if (gauss_whole_lines(pass[i], order[i])) mid = i;
        if (mid < 0 && accumulate)
            return fail_invalid("gaussian_smooth: accumulate with three passes needs one axis staged whole "
                                "(nz <= 1024, or nx or ny <= %d)", sizeof(R) == 4 ? 64 : 32);
        if (mid >= 0 && mid != 1) {
            std::swap(pass[mid], pass[1]);
            std::swap(tw[mid], tw[1]);
            std::swap(order[mid], order[1]);
        }
    }
    if (m >= 2) {
        if (!scratch) return fail_invalid("gaussian_smooth: two or more passes need the scratch tensor");
        if (any_overlap({{scratch, bytes}}, {{in, bytes}, {out, bytes}}))
            return fail_invalid("gaussian_smooth: scratch must not alias in or out");
    }
    // pass.vec was planned against `out`; the scratch tensor must allow the same stores
    const bool scratch_vec = scratch && (uintptr_t)scratch % (4 * sizeof(R)) == 0;
    hipStream_t s = (hipStream_t)stream;
    const R al = (R)alpha;
    const R *src = in;
    for (int i = 0; i < m; ++i) {
        const bool last = i == m - 1;
        R *dst;
        if (last) dst = out;
        else if (m == 2) dst = scratch;
        else if (accumulate) dst = scratch;                 // in -> scratch -> scratch (in place) -> out
        else dst = i == 0 ? out : scratch;                  // in -> out -> scratch -> out
        GaussPass p = pass[i];
        p.final = last;
        p.accumulate = last && accumulate;
        if (dst == scratch) p.vec = p.vec && scratch_vec;
        const hipError_t e = gauss_launch<R>(p, order[i], dst, src, tw[i], al, s);
        if (e != hipSuccess) return fail_hip(e, "gaussian_smooth");
        src = dst;
    }
    return finish_launch(s, "gaussian_smooth");
}

template <typename R>
int gauss_axis_pass(const char *name, R *dst, const R *src, int axis, int r, const double *half, int mode, int64_t rows,
                    const Geom &g, hipStream_t s) {
    GaussPass p;
    GaussTaps tw;
    if (!gauss_plan<R>(p, axis, r, mode, rows, g, dst)) return fail_invalid("%s: bad extent", name);
    gauss_fill_taps<R>(tw, r, half);
    const hipError_t e = gauss_launch<R>(p, axis, dst, src, tw, (R)1, s);   // (final = 0: the rounded sum as it is)
    return e != hipSuccess ? fail_hip(e, name) : LAGO_OK;
}
template int gauss_axis_pass<float>(const char *, float *, const float *, int, int, const double *, int, int64_t,
                                    const Geom &, hipStream_t);
template int gauss_axis_pass<double>(const char *, double *, const double *, int, int, const double *, int, int64_t,
                                     const Geom &, hipStream_t);

}  // namespace lago

extern "C" {
#define LAGO_DEFINE(REAL, SUF)                                                                                      \
    int lago_gauss_smooth##SUF(REAL *out, const REAL *in, REAL *scratch, const int *radii, const double *taps,     \
                               int mode, double alpha, int accumulate, int dim, int64_t rows, int64_t nx,          \
                               int64_t ny, int64_t nz, void *stream) {                                             \
        return lago::gauss_impl<REAL>(out, in, scratch, radii, taps, mode, alpha, accumulate, dim, rows, nx, ny,   \
                                      nz, stream);                                                                  \
    }
LAGO_DEFINE(float, _f32)
LAGO_DEFINE(double, _f64)
#undef LAGO_DEFINE
}
