// The exact Euclidean distance transform of a label map -- gfx950 HIP kernels.  No counterpart in the reference.  The
// per-line arithmetic (feature predicate, candidate, minimum) is edt_line.hpp; this file stages lines and walks them.
//
// The squared distance separates: one pass per spatial axis, the contiguous axis first, each computing per line
// out[i] = min_j g[j] + (s (i - j))^2.  The first pass forms g (0 on a feature, +inf elsewhere) from L as it loads the
// line -- the surface stencil included, no mask volume is written -- and writes `out`; the later passes run IN PLACE on
// `out`: a workgroup owns a tile of whole lines, has all of it in LDS before its first store, and no other workgroup
// touches those lines, so no second buffer is needed.  The last pass takes the square root unless the caller wants the
// squared distance.
//
//   edt_pass_kernel<FIRST, SQRT, TZ>   256 lanes, one tile of TZ lines a workgroup, TZ in {64, 32, 16} by the line's
//     extent n (n <= 256, <= 512, <= 1024) so that the tile stays within 64 KB of LDS.
//     FIRST (the contiguous axis, g from L): the tile is TZ rows x n, a wave loads a row with consecutive lanes on
//       consecutive voxels.  Row r keeps voxel j at r * stride + (j ^ r), stride = n rounded up to 64: the load phase
//       (one r, consecutive j) and the walk (one j, consecutive r) both touch distinct banks, without padding a row
//       beyond the budget (r < 64, so j ^ r stays inside j's block of 64).
//     otherwise (a strided axis, g from `out`): the tile is n x TZ contiguous voxels, element (j, c) at j * TZ + c;
//       loads, LDS reads and stores all have consecutive lanes on consecutive addresses.
//     The walk is the same for both: lane (line = tid % TZ, block = tid / TZ) holds EDT_BLOCK outputs of its line in
//     registers and reads g[j] of that line once for all of them (the 256 / TZ lanes of a wave on one line read one
//     address: a broadcast), then stores them.  Plain brute force over j, n^2 / EDT_BLOCK LDS reads a line; the costs
//     (s (i - j))^2 of a lane's outputs move up by one output from a source to the next, so one is formed per source
//     and a candidate is an add and a min (edt_line.hpp: EdtBlock).  The walk takes EDT_BLOCK sources a trip; the tile
//     holds +inf, which offers nothing, from n up to the next multiple.
//
// No atomics: the same bits from call to call.
#include "common.hpp"
#include "edt_line.hpp"

namespace lago {

struct EdtArgs {
    int n;            // extent of the pass's axis
    float s;          // its spacing
    // FIRST
    int dim, nx, ny, nz, where;
    int32_t label;
    int stride;       // of a row in LDS
    int64_t rows;     // nn * nx * ny lines of nz voxels
    // strided
    uint32_t inner;   // elements between two voxels of a line; a line's column is in [0, inner)
    uint32_t ntc;     // column tiles: ceil(inner / TZ)
};

extern __shared__ float edt_smem[];

template <bool FIRST, bool SQRT, int TZ>
__global__ __launch_bounds__(kBlock) void edt_pass_kernel(float *io, const int32_t *__restrict__ L, EdtArgs p) {
    static_assert(kBlock % TZ == 0 && !(FIRST && SQRT), "a volume has at least two passes: the first is never the last");
    constexpr int NB = kBlock / TZ;   // output blocks of one line in flight
    const int n = p.n, n8 = (n + EDT_BLOCK - 1) / EDT_BLOCK * EDT_BLOCK;   // the walk takes EDT_BLOCK sources a trip: +inf up to n8
    const int line = (int)threadIdx.x % TZ, blk = (int)threadIdx.x / TZ;
    float *o;          // the lane's line: voxel i at o[i * ostep]
    size_t ostep;
    bool valid;
    if (FIRST) {
        const int64_t row0 = (int64_t)blockIdx.x * TZ;
        const int64_t per_item = (int64_t)p.nx * p.ny;
        for (int r = (int)threadIdx.x >> 6; r < TZ; r += kBlock / 64) {   // a wave a row (uniform)
            const int64_t q = row0 + r;
            if (q >= p.rows) break;
            const int64_t item = q / per_item;
            const int rem = (int)(q - item * per_item);
            const int x = rem / p.ny, y = rem - x * p.ny;
            const int32_t *Lv = L + (size_t)item * ((size_t)per_item * n);
            for (int j = (int)threadIdx.x & 63; j < n8; j += 64)
                edt_smem[r * p.stride + (j ^ r)] = edt_g0(j < n && edt_feature(Lv, p.where, p.label, p.dim, x, y, j, p.nx, p.ny, n));
        }
        valid = row0 + line < p.rows;
        o = io + (size_t)(row0 + line) * n;
        ostep = 1;
    } else {
        const uint32_t outer = blockIdx.x / p.ntc, c0 = (blockIdx.x - outer * p.ntc) * TZ;   // uniform
        float *base = io + (size_t)outer * n * p.inner + c0;
        const uint32_t left = p.inner - c0;   // columns from c0 on (>= 1)
        for (int e = threadIdx.x; e < n8 * TZ; e += kBlock) {
            const int j = e / TZ, c = e % TZ;
            edt_smem[e] = j < n && (uint32_t)c < left ? base[(size_t)j * p.inner + c] : __builtin_inff();
        }
        valid = (uint32_t)line < left;
        o = base + line;
        ostep = p.inner;
    }
    __syncthreads();
    if (!valid) return;   // (no barrier below)
    for (int i0 = blk * EDT_BLOCK; i0 < n; i0 += NB * EDT_BLOCK) {
        EdtBlock b;
        b.start(p.s, i0);
        for (int j0 = 0; j0 < n8; j0 += EDT_BLOCK) {
#pragma unroll
            for (int u = 0; u < EDT_BLOCK; ++u) {   // unrolled: the block's costs move through registers by renaming
                const int j = j0 + u;
                b.source(FIRST ? edt_smem[line * p.stride + (j ^ line)] : edt_smem[j * TZ + line], p.s);
            }
        }
#pragma unroll
        for (int r = 0; r < EDT_BLOCK; ++r)
            if (i0 + r < n) o[(size_t)(i0 + r) * ostep] = SQRT ? __builtin_sqrtf(b.acc[r]) : b.acc[r];
    }
}

static int edt_tile(int n) { return n <= 256 ? 64 : (n <= 512 ? 32 : 16); }

template <bool FIRST>
static hipError_t edt_pass_launch(float *io, const int32_t *L, const EdtArgs &p, bool sqrt_out, uint32_t lines_outer, hipStream_t s) {
    hipError_t e = hipSuccess;
    const int tz = edt_tile(p.n);
    with_int<64, 32, 16>(tz, [&](auto TZ) {
        with_flags([&](auto SQRT) {
            if constexpr (!(FIRST && SQRT())) {
                const size_t smem = (size_t)(FIRST ? p.stride : (p.n + EDT_BLOCK - 1) / EDT_BLOCK * EDT_BLOCK) * TZ() * sizeof(float);   // <= 64 KB
                const uint32_t nb = FIRST ? (uint32_t)((p.rows + TZ() - 1) / TZ()) : lines_outer * ((p.inner + TZ() - 1) / TZ());
                EdtArgs q = p;
                q.ntc = (p.inner + TZ() - 1) / TZ();
                e = launch(edt_pass_kernel<FIRST, SQRT(), TZ()>, dim3(nb), dim3(kBlock), smem, s, io, L, q);
            }
        }, sqrt_out);
    });
    return e;
}

static int distance_transform_impl(float *out, const int32_t *L, int where, int32_t label, const double *spacing, int squared,
                                   int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz, void *stream) {
    if (const int rc = check_dim("distance_transform", dim)) return rc;
    if (where != LAGO_EDT_NONZERO && where != LAGO_EDT_EQUAL && where != LAGO_EDT_NOT_EQUAL && where != LAGO_EDT_SURFACE)
        return fail_invalid("distance_transform: where must be one of LAGO_EDT_*, got %d", where);
    if (!spacing) return fail_invalid("distance_transform: null pointer");
    for (int a = 0; a < dim; ++a)
        if (!(spacing[a] > 0.0) || !((float)spacing[a] > 0.0f) || !((float)spacing[a] < __builtin_inff()))
            return fail_invalid("distance_transform: spacing must be positive and finite in float32 (axis %d: %g)", a, spacing[a]);
    Volume v;   // (the extents are bounded just below)
    if (const int rc = check_volume(v, "distance_transform", dim, nx, ny, nz, kPlaneAny, {nn})) return rc;
    as_volume(dim, nx, ny, nz);
    if (nx > EDT_MAX_EXTENT || ny > EDT_MAX_EXTENT || nz > EDT_MAX_EXTENT)
        return fail_invalid("distance_transform: an extent above %d (%lld, %lld, %lld)", EDT_MAX_EXTENT, (long long)nx, (long long)ny, (long long)nz);
    if (nn == 0 || v.nvox == 0) return LAGO_OK;   // nothing to write
    if (!out || !L) return fail_invalid("distance_transform: null pointer");
    const int64_t rows = nn * nx * ny;
    // no pass has more workgroups than there are voxels
    if (nn >= (1ll << 31) || rows * nz >= (1ll << 31)) return fail_invalid("distance_transform: 2^31 voxels or more");
    const size_t bytes = (size_t)rows * nz * 4;
    if (overlaps(out, L, bytes)) return fail_invalid("distance_transform: out must not overlap L");
    hipStream_t s = (hipStream_t)stream;
    const float sx = dim == 3 ? (float)spacing[0] : 1.0f, sy = (float)spacing[dim - 2], sz = (float)spacing[dim - 1];
    EdtArgs p = {};
    p.n = (int)nz;
    p.s = sz;
    p.dim = dim;
    p.nx = (int)nx;
    p.ny = (int)ny;
    p.nz = (int)nz;
    p.where = where;
    p.label = label;
    p.stride = ((int)nz + 63) / 64 * 64;
    p.rows = rows;
    p.inner = 1;
    hipError_t e = edt_pass_launch<true>(out, L, p, false, 0, s);
    if (e != hipSuccess) return fail_hip(e, "distance_transform");
    p.n = (int)ny;
    p.s = sy;
    p.inner = (uint32_t)nz;
    e = edt_pass_launch<false>(out, L, p, dim == 2 && !squared, (uint32_t)(nn * nx), s);
    if (e != hipSuccess) return fail_hip(e, "distance_transform");
    if (dim == 3) {
        p.n = (int)nx;
        p.s = sx;
        p.inner = (uint32_t)(ny * nz);
        e = edt_pass_launch<false>(out, L, p, !squared, (uint32_t)nn, s);
    }
    return launched(e, s, "distance_transform");
}

}  // namespace lago

extern "C" int lago_distance_transform(float *out, const int32_t *L, int where, int32_t label, const double *spacing, int squared,
                                       int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz, void *stream) {
    return lago::distance_transform_impl(out, L, where, label, spacing, squared, dim, nn, nx, ny, nz, stream);
}
