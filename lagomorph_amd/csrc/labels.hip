// Label maps: warping a segmentation through a deformation, and the overlap counts of two segmentations -- gfx950 HIP
// kernels.  No counterpart in the reference.  Labels are int32 VALUES (any bit pattern), never blended: the per-voxel
// arithmetic of the warp is label_vote.hpp.
//
//   warp_labels_kernel         one lane per output voxel (2D, and 3D volumes too small or too flat for the slab walk):
//                              the 2^d corner labels are 4-byte buffer loads, the (z, z + 1) pair of a row ONE 8-byte
//                              load at zb = min(lo, nz - 2) as Lerp3 forms it.  Where all corners carry one label -- the
//                              interior of every structure -- it is written without forming a weight; the double vote
//                              sits behind that branch (lanes decide for themselves, a wave with no such lane skips it).
//   warp_labels3_unroll_kernel the slab-interleaved walk of interp_fwd3_unroll_kernel (its reasons are in interp.hip):
//                              U voxels a lane, every load and gather of a wave within ~256 contiguous bytes, the U * 4
//                              pair gathers issued back to back.
//   label_overlap_kernel       the scheme of chunk_table.hpp in its wave-uniform form with 16-byte loads of A and B and a
//                              (K, 3) table of 32-bit counters, one replica a wave while 64 KB hold them; the reducer
//                              gives int64.  A wave first aggregates: the lanes that hold the first pending lane's
//                              (a, b) pair are found with a ballot and ONE lane adds their number (inside a structure
//                              the whole wave is one round, at a boundary two); lanes still pending after two rounds
//                              add for themselves.
//
// No float atomic, no global atomic, no memset: both operators give the same bits from call to call, and the counts
// are those of a sequential pass for any chunking.
#include "chunk_table.hpp"   // (and common.hpp)
#include "label_vote.hpp"

#ifndef LAGO_NT_LABELS_ST
#define LAGO_NT_LABELS_ST 1   // the warped labels are written once and not re-read by the kernel: non-temporal, as interp_forward's output
#endif
#ifndef LAGO_LABELS_CHUNK
#define LAGO_LABELS_CHUNK 16384   // voxels of a row per overlap workgroup, 64 a lane: 4096, 8192 and 32768 measured slower (profiles/labels_timing.md)
#endif
#ifndef LAGO_LABELS_ROUNDS
#define LAGO_LABELS_ROUNDS 2  // wave-aggregation rounds of label_overlap_kernel before the lanes left add for themselves
#endif

namespace lago {

// ------------------------------------------------------------------ warp_labels

// two adjacent labels with ONE load (through a scalar integer of the full width: see buf_load2 of common.hpp)
__device__ __forceinline__ void buf_load2_i32(BufRsrc r, uint32_t off, int32_t &lo, int32_t &hi) {
    const lg_u32x2 p = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
    const unsigned long long q = __builtin_bit_cast(unsigned long long, p);
    lo = (int32_t)(unsigned int)q;
    hi = (int32_t)(unsigned int)(q >> 32);
}
__device__ __forceinline__ int32_t buf_load1_i32(BufRsrc r, uint32_t off) {
    return (int32_t)__builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0);
}

// The corners of one sample in a plane of int32 labels.  Axes are Geom's (nx = 1 in 2D, which then has the rows y lo / y
// hi only).  Every offset lies inside the plane: the corners are clamped (label_vote.hpp: lv_axis) and zb + 1 <= nz - 1.
// THIN_OK = false promises nz >= 2 at compile time, as for Lerp3.
template <typename R, int DIM, bool THIN_OK = true>
struct LabelTaps {
    static constexpr int NR = DIM == 3 ? 4 : 2, NC = 2 * NR;
    LvAxis ax, ay, az;   // (ax unused in 2D)
    int ny, nz;
    uint32_t bytes;      // of the plane (uniform)
    __device__ __forceinline__ void setup(int i, int j, int k, double dt, R ux, R uy, R uz, const Geom &g) {
        if (DIM == 3) ax = lv_axis<R>(lv_sample_pos<R>(i, dt, ux), g.nx);
        ay = lv_axis<R>(lv_sample_pos<R>(j, dt, uy), g.ny);
        az = lv_axis<R>(lv_sample_pos<R>(k, dt, uz), g.nz);
        ny = g.ny;
        nz = g.nz;
        bytes = g.nvox * 4u;
    }
    __device__ __forceinline__ uint32_t row(int x, int y) const {   // byte offset of row (x, y)
        return (DIM == 3 ? (uint32_t)x * (uint32_t)ny + (uint32_t)y : (uint32_t)y) * (uint32_t)nz * 4u;
    }
    __device__ __forceinline__ int32_t nearest(const int32_t *__restrict__ L) const {
        return buf_load1_i32(make_rsrc(L, bytes), row(DIM == 3 ? ax.nearest() : 0, ay.nearest()) + (uint32_t)az.nearest() * 4u);
    }
    // corner q = 4 (x hi) + 2 (y hi) + (z hi) in 3D, 2 (y hi) + (z hi) in 2D
    __device__ __forceinline__ void fetch(const int32_t *__restrict__ L, int32_t (&c)[NC]) const {
        const BufRsrc r = make_rsrc(L, bytes);
        const bool thin = THIN_OK && nz < 2;
        const int zb = thin ? 0 : min(az.lo, nz - 2);
        const bool f_hi = az.lo != zb, c_lo = az.hi == zb;   // the lower corner is the pair's second / the upper its first
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            const uint32_t o = row(DIM == 3 ? ((q & 2) ? ax.hi : ax.lo) : 0, (q & 1) ? ay.hi : ay.lo) + (uint32_t)zb * 4u;
            int32_t lo, hi;
            if (thin)
                lo = hi = buf_load1_i32(r, o);
            else
                buf_load2_i32(r, o, lo, hi);
            c[2 * q] = f_hi ? hi : lo;
            c[2 * q + 1] = c_lo ? lo : hi;
        }
    }
    // the label of corners c: their common one without a weight, else the vote
    __device__ __forceinline__ int32_t vote(const int32_t (&c)[NC]) const {
        bool same = true;
#pragma unroll
        for (int q = 1; q < NC; ++q) same = same && c[q] == c[0];
        int32_t lab = c[0];
        if (!same) {
            double w[NC];
            if constexpr (DIM == 3) lv_weights(ax.t, ay.t, az.t, w);
            else lv_weights(ay.t, az.t, w);
            lab = lv_vote<NC>(c, w);
        }
        return lab;
    }
};

template <typename R, int DIM, bool BC, bool VOTE>
__global__ __launch_bounds__(kBlock) void warp_labels_kernel(int32_t *__restrict__ out, const int32_t *__restrict__ L,
                                                             const R *__restrict__ u, double dt, Geom g) {
    const Vox v = locate(g);
    if (!v.valid) return;
    const size_t nv = g.nvox;
    const R *un = u + (size_t)v.n * DIM * nv + v.s;
    const int32_t *Ln = BC ? L : L + (size_t)v.n * nv;
    LabelTaps<R, DIM> T;
    if (DIM == 3) T.setup(v.i, v.j, v.k, dt, un[0], un[nv], un[2 * nv], g);
    else T.setup(0, v.j, v.k, dt, (R)0, un[0], un[nv], g);
    int32_t lab;
    if (VOTE) {
        int32_t c[LabelTaps<R, DIM>::NC];
        T.fetch(Ln, c);
        lab = T.vote(c);
    } else {
        lab = T.nearest(Ln);
    }
    st_pol<LAGO_NT_LABELS_ST>(out + (size_t)v.n * nv + v.s, lab);
}

template <typename R, bool BC, bool VOTE, int U>
__global__ __launch_bounds__(kBlock) void warp_labels3_unroll_kernel(int32_t *__restrict__ out, const int32_t *__restrict__ L,
                                                                     const R *__restrict__ u, double dt, Geom g,
                                                                     uint32_t nbx_u, uint32_t nblocks_u) {
    const Slabs<U> sl(g, nbx_u, nblocks_u);
    const size_t nv = g.nvox;
    const R *un = u + (size_t)sl.n * 3 * nv;
    const int32_t *Ln = BC ? L : L + (size_t)sl.n * nv;
    int32_t *on = out + (size_t)sl.n * nv;
    R ux[U], uy[U], uz[U];
#pragma unroll
    for (int e = 0; e < U; ++e) {
        ux[e] = un[sl.s[e]];
        uy[e] = un[nv + sl.s[e]];
        uz[e] = un[2 * nv + sl.s[e]];
    }
    LabelTaps<R, 3, false> T[U];   // nz >= 2 guaranteed by the host (slab_grid)
    sl.walk(g, [&](int e, int i, int j, int k) { T[e].setup(i, j, k, dt, ux[e], uy[e], uz[e], g); });
    int32_t lab[U];
    if (VOTE) {
        int32_t c[U][8];
#pragma unroll
        for (int e = 0; e < U; ++e) T[e].fetch(Ln, c[e]);
#pragma unroll
        for (int e = 0; e < U; ++e) lab[e] = T[e].vote(c[e]);
    } else {
#pragma unroll
        for (int e = 0; e < U; ++e) lab[e] = T[e].nearest(Ln);
    }
#pragma unroll
    for (int e = 0; e < U; ++e)
        if (sl.ok[e]) st_pol<LAGO_NT_LABELS_ST>(on + sl.s[e], lab[e]);
}

template <typename R>
static int warp_labels_impl(int32_t *out, const int32_t *L, const R *u, double dt, int mode, int bc, int dim, int64_t nn,
                            int64_t nx, int64_t ny, int64_t nz, void *stream) {
    if (const int rc = check_dim("warp_labels", dim)) return rc;
    if (mode != LAGO_LABELS_NEAREST && mode != LAGO_LABELS_VOTE)
        return fail_invalid("warp_labels: mode must be LAGO_LABELS_NEAREST or LAGO_LABELS_VOTE, got %d", mode);
    Volume v;
    if (const int rc = check_volume(v, "warp_labels", dim, nx, ny, nz, kPlane29, {nn})) return rc;
    if (nn == 0 || v.nvox == 0) return LAGO_OK;   // nothing to write
    Geom g;
    if (!make_geom(g, v, nn)) return fail_invalid("warp_labels: bad extent");
    // one 4-byte label a voxel, gathered at the voxels' own positions
    if (const int rc = check_gather("warp_labels", out, L, u, GatherBytes(4, sizeof(R), dim, nn, 1, v.nvox, v.nvox, bc)); rc != kLaunchNow)
        return rc;
    hipStream_t s = (hipStream_t)stream;
    constexpr int U = 2;
    hipError_t e = hipSuccess;
    uint32_t nbx_u, nb;
    if (dim == 3 && g_interp_vec && slab_grid(g, nn, U, nbx_u, nb)) {
        with_flags([&](auto BC, auto VOTE) {
            e = launch(warp_labels3_unroll_kernel<R, BC(), VOTE(), U>, dim3(nb), dim3(kBlock), 0, s, out, L, u, dt, g, nbx_u, nb);
        }, bc != 0, mode == LAGO_LABELS_VOTE);
        note_path(LP_VECTOR_GATHER);
    } else {
        with_dim(dim, [&](auto DIM) {
            with_flags([&](auto BC, auto VOTE) {
                e = launch(warp_labels_kernel<R, DIM(), BC(), VOTE()>, dim3(g.nblocks), dim3(kBlock), 0, s, out, L, u, dt, g);
            }, bc != 0, mode == LAGO_LABELS_VOTE);
        });
    }
    return launched(e, s, "warp_labels");
}

// ------------------------------------------------------------------ label_overlap

constexpr int kLabChunkMin = LAGO_LABELS_CHUNK;   // voxels an overlap workgroup walks where the slab's cap allows

struct OverlapArgs {
    int K, rep;   // rep: replicas of the table in LDS, 1, 2 or 4 (a wave adds into replica wave % rep)
    RowChunks rc;
};

extern __shared__ uint32_t lab_smem[];

// One step of a wave: every lane with `valid` holds one voxel's pair (a, b).  Wave-uniform control flow throughout
// (chunk_walk_uniform's loops are): `todo` is a scalar mask.
__device__ __forceinline__ void overlap_add(uint32_t *tab, uint32_t K, bool valid, int32_t a, int32_t b) {
    const auto add = [&](int32_t x, int32_t y, uint32_t n) {
        if ((uint32_t)x < K) atomicAdd(tab + 3u * (uint32_t)x, n);
        if ((uint32_t)y < K) atomicAdd(tab + 3u * (uint32_t)y + 1u, n);
        if (x == y && (uint32_t)x < K) atomicAdd(tab + 3u * (uint32_t)x + 2u, n);
    };
    const uint32_t lane = __lane_id();
    unsigned long long todo = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
    for (int round = 0; round < LAGO_LABELS_ROUNDS; ++round) {
        if (todo == 0) return;
        const uint32_t first = (uint32_t)__builtin_ctzll(todo);
        const int32_t fa = __builtin_amdgcn_readlane(a, first), fb = __builtin_amdgcn_readlane(b, first);
        const unsigned long long m = __builtin_amdgcn_ballot_w64(valid && a == fa && b == fb) & todo;
        if (lane == first) add(fa, fb, (uint32_t)__builtin_popcountll(m));
        todo &= ~m;
    }
    if ((todo >> lane) & 1ull) add(a, b, 1u);
}

__global__ __launch_bounds__(kBlock) void label_overlap_kernel(uint32_t *__restrict__ slab, const int32_t *__restrict__ A,
                                                               const int32_t *__restrict__ B, OverlapArgs p) {
    typedef int32_t vec __attribute__((ext_vector_type(4)));
    constexpr uint32_t VW = 4;
    const uint32_t K3 = 3u * (uint32_t)p.K;
    tables_zero(lab_smem, K3, p.rep);
    const ChunkOfRow c = chunk_of_block(p.rc);
    const int32_t *Ac = A + (size_t)c.row * p.rc.nvox + c.c0, *Bc = B + (size_t)c.row * p.rc.nvox + c.c0;   // of the chunk
    uint32_t *tab = lab_smem + ((threadIdx.x >> 6) & (uint32_t)(p.rep - 1)) * K3;
    const uint32_t mA = misalign<VW>(Ac);
    chunk_walk_uniform<VW>(c.n, mA == misalign<VW>(Bc), mA, [&](uint32_t i, bool valid) {
        overlap_add(tab, (uint32_t)p.K, valid, valid ? Ac[i] : 0, valid ? Bc[i] : 0);
    }, [&](uint32_t first, uint32_t i, bool valid) {
        vec x = {0, 0, 0, 0}, y = {0, 0, 0, 0};
        if (valid) {
            x = *reinterpret_cast<const vec *>(Ac + first + i);
            y = *reinterpret_cast<const vec *>(Bc + first + i);
        }
#pragma unroll
        for (uint32_t k = 0; k < VW; ++k) overlap_add(tab, (uint32_t)p.K, valid, x[k], y[k]);
    });
    tables_store(slab, lab_smem, K3, p.rep);
}

// what table_reduce_kernel does with a finished sum: stored as it is
struct CountFinish { long long *counts; __device__ void operator()(size_t i, long long sum) const { counts[i] = sum; } };

static int label_overlap_impl(long long *counts, const int32_t *A, const int32_t *B, uint32_t *scratch, int64_t scratch_chunks,
                              int K, int64_t rows, int64_t nvox, void *stream) {
    if (K < 1 || K > LAGO_LABELS_MAX) return fail_invalid("label_overlap: num_labels must be in 1..%d, got %d", LAGO_LABELS_MAX, K);
    if (rows < 0 || nvox < 0 || rows >= (1ll << 31)) return fail_invalid("label_overlap: bad extent");
    if (nvox > (1ll << 30)) return fail_invalid("label_overlap: more than 2^30 voxels in a row");
    if (rows == 0) return LAGO_OK;
    if (!counts || !scratch || (nvox && (!A || !B))) return fail_invalid("label_overlap: null pointer");
    const uint32_t K3 = 3u * (uint32_t)K;
    OverlapArgs p;
    p.K = K;
    size_t sbytes;
    if (const int rc = plan_tables<uint32_t>(p.rc, sbytes, "label_overlap", K3, rows, nvox, kLabChunkMin, scratch_chunks); rc != kLaunchNow)
        return rc;
    const auto fits = [&](int r) { return (size_t)r * K3 * 4 <= kTableLdsBytes; };
    p.rep = fits(4) ? 4 : (fits(2) ? 2 : 1);   // K <= 1365 four, K <= 2730 two, else one (4096 labels: 48 KB)
    const size_t ibytes = (size_t)rows * nvox * 4, cbytes = (size_t)rows * K3 * 8;
    if (any_overlap({{counts, cbytes}, {scratch, sbytes}}, {{A, ibytes}, {B, ibytes}}))
        return fail_invalid("label_overlap: counts and scratch must not overlap an input or each other");
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = launch(label_overlap_kernel, dim3((uint32_t)rows * p.rc.chunks), dim3(kBlock), (size_t)p.rep * K3 * 4, s, scratch, A, B, p);
    return reduce_tables("label_overlap", e, s, p.rc, rows, K3, (const uint32_t *)scratch, CountFinish{counts});
}

}  // namespace lago

extern "C" {
int lago_label_overlap_scratch_chunks(int num_labels, int64_t rows, int64_t nvox) {
    return lago::scratch_chunks(num_labels >= 1 && num_labels <= LAGO_LABELS_MAX, (int64_t)num_labels * 12, rows, nvox, lago::kLabChunkMin);
}
int lago_label_overlap(long long *counts, const int32_t *A, const int32_t *B, uint32_t *scratch, int64_t scratch_chunks,
                       int num_labels, int64_t rows, int64_t nvox, void *stream) {
    return lago::label_overlap_impl(counts, A, B, scratch, scratch_chunks, num_labels, rows, nvox, stream);
}
#define LAGO_DEFINE(REAL, SUF)                                                                                       \
    int lago_warp_labels##SUF(int32_t *out, const int32_t *L, const REAL *u, double dt, int mode, int broadcast,    \
                              int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz, void *stream) {               \
        return lago::warp_labels_impl<REAL>(out, L, u, dt, mode, broadcast, dim, nn, nx, ny, nz, stream);            \
    }
LAGO_DEFINE(float, _f32)
LAGO_DEFINE(double, _f64)
#undef LAGO_DEFINE
}
