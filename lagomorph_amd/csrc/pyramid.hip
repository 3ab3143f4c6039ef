// Image pyramid by a factor of two: the reduce R (binomial 1 4 6 4 1 / 16 at every second voxel, clamped border), the
// linear expand E, and their exact transposes -- gfx950 HIP kernels.  No counterpart in the reference.  The definition
// is in include/lagomorph_hip.h (lago_pyramid_down); the per-axis matrices, the tap ranges, the evaluation order and
// the rounding count are in pyramid_weights.hpp, which a host compiler builds too.
//
//   out[r, ...] = scale (Mx (x) My (x) Mz) in[r, ...]        r = batch item x channel; 2D fields are (y, z)
//
// Two kernels, each instantiated with the two matrices (PyrReduce, PyrExpand): four operators.  Both work on FINE tiles
// of TX x TY x TZ = 8 x 8 x 64 (2D: 64 x 64) voxels of one row r -- 4 x 4 x 32 (32 x 32) coarse voxels, tile origins
// even -- z the contiguous axis, 256 lanes a tile, blocks in xcd_swizzle order.  The weights of the tile's coordinates
// go to an LDS table first (one entry per coordinate and tap, none per voxel).
//
// pyramid_down_kernel (coarse out, fine in: R and E^T; one streaming read, an eighth of it written).  The fine tile is
// staged once with a halo of two voxels, every coordinate clamped (halo_tile.hpp: 12 x 12 x 68 cells, 38 KB in float32,
// 77 KB in float64; a tap beyond the grid weighs exactly 0, so what the clamp puts there is multiplied away).  The axes
// are contracted in LDS, the contiguous axis first:
//      a1[px][py][jz] = sum_k Wz[jz, k] tile[px][py][2 jz + k]     lane = jz: a lane reads its cells 2 jz ... 2 jz + 5 as
//                                                                  three aligned pairs, consecutive lanes consecutive
//                                                                  pairs -- conflict-free where five single reads at a
//                                                                  stride of two cells would be 2-way conflicts
//      a2[px][jy][jz] = sum_k Wy[jy, k] a1[px][2 jy + k][jz]       lanes along jz: consecutive cells
//      out[jx][jy][jz] = sum_k Wx[jx, k] a2[2 jx + k][jy][jz]      (3D only; a2 takes the place of the tile)
// and a wave stores two rows of 32 coarse voxels.
//
// pyramid_up_kernel (fine out, coarse in: E and R^T; one streaming write).  The (T/2 + 2)^d coarse box a tile reaches
// -- 6 x 6 x 34 cells, zero beyond the grid -- is staged in LDS and contracted x, then y in LDS; the z contraction runs
// in registers, lane = z, a wave storing one whole row at a time (lanes 2 i and 2 i + 1 read the same cells: broadcast).
//
// Every output element has one owner: no atomics, no memset, no scratch; the bits repeat from call to call, on any
// stream.  Every LDS index stays inside the launch's allocation: down reads cells 2 j + k <= 2 (T/2 - 1) + 5 = T + 3
// of T + 4 per row, up reads cells (l >> 1) + t <= T/2 + 1 of T/2 + 2.  Every global index is a clamped coordinate or
// a coordinate tested against the extents.
#include "common.hpp"
#include "halo_tile.hpp"
#include "pyramid_weights.hpp"

namespace lago {

template <int DIM> struct PyrTile {
    static constexpr int TX = DIM == 3 ? 8 : 1, TY = DIM == 3 ? 8 : 64, TZ = 64, ROWS = TX * TY;
    static constexpr int CX = DIM == 3 ? TX / 2 : 1, CY = TY / 2, CZ = TZ / 2;   // coarse voxels of a tile
    static constexpr int BX = DIM == 3 ? CX + 2 : 1, BY = CY + 2, BZ = CZ + 2;   // the coarse box `up` stages
};
template <typename R, int DIM> using PyrHaloTile = HaloTile<R, DIM, PyrTile<DIM>::TX, PyrTile<DIM>::TY, PyrTile<DIM>::TZ, 2, 2>;

struct PyrGeom {
    int n[3], m[3];         // fine and coarse voxels per axis (x, y, z); 2D: n[0] = m[0] = 1
    uint32_t nt[3];         // tiles per axis
    uint32_t ntiles, nvox, mvox, nblocks;   // tiles, fine and coarse voxels of a row; tiles in all
    FastDiv dtiles, dtyz, dtz;
    double scale;
};

struct PyrBlock {
    uint32_t row;
    int o[3];   // the tile's fine origin (even)
};
template <int DIM>
__device__ __forceinline__ PyrBlock pyr_block(const PyrGeom &g) {
    using T = PyrTile<DIM>;
    PyrBlock b;
    const uint32_t id = xcd_swizzle(blockIdx.x, g.nblocks);
    b.row = g.dtiles.div(id);
    const uint32_t t = id - b.row * g.ntiles;
    const uint32_t tx = g.dtyz.div(t), r = t - tx * (g.nt[1] * g.nt[2]);
    const uint32_t ty = g.dtz.div(r), tz = r - ty * g.nt[2];
    b.o[0] = (int)tx * T::TX;
    b.o[1] = (int)ty * T::TY;
    b.o[2] = (int)tz * T::TZ;
    return b;
}

template <typename R> struct alignas(2 * sizeof(R)) PyrPair { R a, b; };

template <typename R, int DIM, typename W>
__global__ __launch_bounds__(256) void pyramid_down_kernel(R *__restrict__ out, const R *__restrict__ in, PyrGeom g) {
    using T = PyrTile<DIM>;
    using H = PyrHaloTile<R, DIM>;
    constexpr int K = kPyrDownTaps;
    constexpr uint32_t CX = T::CX, CY = T::CY, CZ = T::CZ, PX = H::PX, PY = H::PY, LD = H::LD;
    static_assert(CZ == 32 && LD % 2 == 0, "a lane's cells start at an aligned pair; 256 lanes keep their jz");
    extern __shared__ __attribute__((aligned(16))) unsigned char pyr_smem[];
    R *tile = reinterpret_cast<R *>(pyr_smem);   // the staged tile [PX][PY][LD]; then a2 [PX][CY][CZ] (3D)
    R *a1 = tile + H::CELLS;                     // [PX][PY][CZ]
    R *wt = a1 + PX * PY * CZ;                   // [CX + CY + CZ][K]: x, then y, then z
    const uint32_t tid = threadIdx.x;
    const PyrBlock b = pyr_block<DIM>(g);

    for (uint32_t e = tid; e < (CX + CY + CZ) * K; e += 256) {
        const uint32_t c = e / K, k = e - c * K;
        const int a = c < CX ? 0 : c < CX + CY ? 1 : 2;
        const int l = (int)c - (a == 0 ? 0 : a == 1 ? (int)CX : (int)(CX + CY));
        const int o = a == 0 ? b.o[0] : a == 1 ? b.o[1] : b.o[2], n = a == 0 ? g.n[0] : a == 1 ? g.n[1] : g.n[2];   // (no private array)
        wt[e] = pyr_down_weight<R, W>(o / 2 + l, (int)k, n);
    }
    H::stage(tile, in + (size_t)b.row * g.nvox, b.o, g.n, tid, 256u);
    __syncthreads();
    {   // z
        const uint32_t jz = tid & (CZ - 1);
        R w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = wt[(CX + CY + jz) * K + k];
        for (uint32_t e = tid; e < PX * PY * CZ; e += 256) {
            const PyrPair<R> *p = reinterpret_cast<const PyrPair<R> *>(tile + (e / CZ) * LD + 2 * jz);
            const PyrPair<R> p0 = p[0], p1 = p[1], p2 = p[2];
            const R v[K] = {p0.a, p0.b, p1.a, p1.b, p2.a};
            a1[e] = pyr_dot<K>(w, [&](int k) { return v[k]; });
        }
    }
    __syncthreads();   // the tile is dead: it becomes a2
    R *dst = out + (size_t)b.row * g.mvox;
    const int cz = b.o[2] / 2 + (int)(tid & (CZ - 1));
    for (uint32_t e = tid; e < PX * CY * CZ; e += 256) {   // y
        const uint32_t jz = e & (CZ - 1), t = e / CZ, px = t / CY, jy = t - px * CY;
        const R *src = a1 + (px * PY + 2 * jy) * CZ + jz;
        const R acc = pyr_dot<K>(wt + (CX + jy) * K, [&](int k) { return src[(uint32_t)k * CZ]; });
        if constexpr (DIM == 3) {
            tile[e] = acc;
        } else {
            const int cy = b.o[1] / 2 + (int)jy;
            if (cy < g.m[1] && cz < g.m[2]) dst[(size_t)cy * g.m[2] + (uint32_t)cz] = pyr_scale(acc, g.scale);
        }
    }
    if constexpr (DIM == 3) {
        __syncthreads();
        for (uint32_t e = tid; e < CX * CY * CZ; e += 256) {   // x
            const uint32_t jz = e & (CZ - 1), t = e / CZ, jx = t / CY, jy = t - jx * CY;
            const R *src = tile + (2 * jx * CY + jy) * CZ + jz;
            const R acc = pyr_dot<K>(wt + jx * K, [&](int k) { return src[(uint32_t)k * (CY * CZ)]; });
            const int cx = b.o[0] / 2 + (int)jx, cy = b.o[1] / 2 + (int)jy;
            if (cx < g.m[0] && cy < g.m[1] && cz < g.m[2]) dst[((size_t)cx * g.m[1] + cy) * g.m[2] + (uint32_t)cz] = pyr_scale(acc, g.scale);
        }
    }
}

template <typename R, int DIM, typename W>
__global__ __launch_bounds__(256) void pyramid_up_kernel(R *__restrict__ out, const R *__restrict__ in, PyrGeom g) {
    using T = PyrTile<DIM>;
    constexpr int K = kPyrUpTaps;
    constexpr uint32_t TX = T::TX, TY = T::TY, TZ = T::TZ, BX = T::BX, BY = T::BY, BZ = T::BZ, P = BY * BZ;
    __shared__ R box[BX * P];                         // the coarse box, zero beyond the grid
    __shared__ R b1[DIM == 3 ? TX * P : 1];           // [TX][BY][BZ] (3D)
    __shared__ R b2[T::ROWS * BZ];                    // [TX][TY][BZ]
    __shared__ R wt[(TX + TY + TZ) * K];              // x, then y, then z
    const uint32_t tid = threadIdx.x;
    const PyrBlock b = pyr_block<DIM>(g);
    const int lo[3] = {DIM == 3 ? b.o[0] / 2 - 1 : 0, b.o[1] / 2 - 1, b.o[2] / 2 - 1};

    for (uint32_t e = tid; e < (TX + TY + TZ) * K; e += 256) {
        const uint32_t c = e / K, t = e - c * K;
        const int a = c < TX ? 0 : c < TX + TY ? 1 : 2;
        const int l = (int)c - (a == 0 ? 0 : a == 1 ? (int)TX : (int)(TX + TY));
        const int o = a == 0 ? b.o[0] : a == 1 ? b.o[1] : b.o[2], n = a == 0 ? g.n[0] : a == 1 ? g.n[1] : g.n[2];   // (no private array)
        wt[e] = pyr_up_weight<R, W>(o + l, (int)t, n);
    }
    {
        const R *src = in + (size_t)b.row * g.mvox;
        for (uint32_t e = tid; e < BX * P; e += 256) {
            const uint32_t ba = e / P, bc = e - ba * P, bb = bc / BZ, cc = bc - bb * BZ;
            const int ja = lo[0] + (int)ba, jb = lo[1] + (int)bb, jc = lo[2] + (int)cc;
            R v = (R)0;
            if (ja >= 0 && ja < g.m[0] && jb >= 0 && jb < g.m[1] && jc >= 0 && jc < g.m[2]) v = src[((size_t)ja * g.m[1] + jb) * g.m[2] + jc];
            box[e] = v;
        }
    }
    __syncthreads();
    if constexpr (DIM == 3) {
        for (uint32_t e = tid; e < TX * P; e += 256) {   // x
            const uint32_t x = e / P, bc = e - x * P;
            const R *src = box + (x >> 1) * P + bc;
            b1[e] = pyr_dot<K>(wt + x * K, [&](int t) { return src[(uint32_t)t * P]; });
        }
        __syncthreads();
    }
    for (uint32_t e = tid; e < T::ROWS * BZ; e += 256) {   // y
        const uint32_t r = e / BZ, c = e - r * BZ, x = r / TY, y = r - x * TY;
        const R *src = (DIM == 3 ? b1 + x * P : box) + (y >> 1) * BZ + c;
        b2[e] = pyr_dot<K>(wt + (TX + y) * K, [&](int t) { return src[(uint32_t)t * BZ]; });
    }
    __syncthreads();
    const uint32_t lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (a scalar: the rows are wave-uniform)
    const int z = b.o[2] + (int)lane;
    if (z >= g.n[2]) return;   // (no barrier below)
    R wz[K];
#pragma unroll
    for (int t = 0; t < K; ++t) wz[t] = wt[(TX + TY + lane) * K + t];
    R *dst = out + (size_t)b.row * g.nvox + (uint32_t)z;
    for (uint32_t r = wave; r < (uint32_t)T::ROWS; r += 4) {   // z; wave-uniform rows
        const int x = b.o[0] + (int)(r / TY), y = b.o[1] + (int)(r % TY);
        if (x >= g.n[0] || y >= g.n[1]) continue;
        const R *v = b2 + r * BZ + (lane >> 1);
        dst[((size_t)x * g.n[1] + y) * g.n[2]] = pyr_scale(pyr_dot<K>(wz, [&](int t) { return v[t]; }), g.scale);
    }
}

// The checks both entry points share, before any device call.  LAGO_OK with `empty` set: nothing to do.
static int pyr_geom(const char *what, PyrGeom &g, bool &empty, int op, int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz, double scale) {
    Volume v;
    if (const int rc = check_volume(v, what, dim, nx, ny, nz, kPlane29, {rows})) return rc;
    if (op != kPyramidReduce && op != kPyramidExpand) return fail_invalid("%s: unknown op %d (LAGO_PYRAMID_REDUCE, LAGO_PYRAMID_EXPAND)", what, op);
    empty = rows == 0 || v.nvox == 0;
    if (empty) return LAGO_OK;
    const int64_t n[3] = {v.nx, v.ny, v.nz};
    const int tile[3] = {dim == 3 ? PyrTile<3>::TX : PyrTile<2>::TX, dim == 3 ? PyrTile<3>::TY : PyrTile<2>::TY, PyrTile<3>::TZ};
    int64_t ntiles = 1, mvox = 1, blocks;
    for (int a = 0; a < 3; ++a) {
        g.n[a] = (int)n[a];
        g.m[a] = (int)pyr_coarse_extent(n[a]);
        g.nt[a] = (uint32_t)((n[a] + tile[a] - 1) / tile[a]);
        ntiles *= g.nt[a];
        mvox *= g.m[a];
    }
    if (rows >= (1ll << 31) || __builtin_mul_overflow(rows, ntiles, &blocks) || blocks >= (1ll << 31))
        return fail_invalid("%s: too many tiles for one launch", what);
    g.ntiles = (uint32_t)ntiles;
    g.nvox = (uint32_t)v.nvox;
    g.mvox = (uint32_t)mvox;
    g.nblocks = (uint32_t)blocks;
    g.dtiles = FastDiv(g.ntiles);
    g.dtyz = FastDiv(g.nt[1] * g.nt[2]);
    g.dtz = FastDiv(g.nt[2]);
    g.scale = scale;
    return LAGO_OK;
}

template <typename R, bool UP>
static int pyramid_impl(R *out, const R *in, int op, int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz, double scale, void *stream) {
    const char *what = UP ? "pyramid_up" : "pyramid_down";
    PyrGeom g;
    bool empty;
    if (const int rc = pyr_geom(what, g, empty, op, dim, rows, nx, ny, nz, scale)) return rc;
    if (empty) return LAGO_OK;   // nothing is written
    if (!out || !in) return fail_invalid("%s: null pointer", what);
    const size_t fine = (size_t)rows * g.nvox * sizeof(R), coarse = (size_t)rows * g.mvox * sizeof(R);
    if (overlaps(out, UP ? fine : coarse, in, UP ? coarse : fine)) return fail_invalid("%s: out must not overlap in", what);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    with_dim(dim, [&](auto DIM) {
        with_flags([&](auto EXPAND) {
            using W = std::conditional_t<EXPAND(), PyrExpand, PyrReduce>;
            if constexpr (UP) {
                e = launch(pyramid_up_kernel<R, DIM(), W>, dim3(g.nblocks), dim3(256), 0, s, out, in, g);
            } else {
                using H = PyrHaloTile<R, DIM()>;
                using T = PyrTile<DIM()>;
                const size_t smem = ((size_t)H::CELLS + (size_t)H::PX * H::PY * T::CZ + (size_t)(T::CX + T::CY + T::CZ) * kPyrDownTaps) * sizeof(R);
                e = launch(pyramid_down_kernel<R, DIM(), W>, dim3(g.nblocks), dim3(256), smem, s, out, in, g);
            }
        }, op == kPyramidExpand);
    });
    return launched(e, s, what);
}

}  // namespace lago

extern "C" {
#define LAGO_DEFINE(REAL, SUF)                                                                                              \
    int lago_pyramid_down##SUF(REAL *out, const REAL *in, int op, int dim, int64_t rows, int64_t nx, int64_t ny,            \
                               int64_t nz, double scale, void *stream) {                                                    \
        return lago::pyramid_impl<REAL, false>(out, in, op, dim, rows, nx, ny, nz, scale, stream);                          \
    }                                                                                                                       \
    int lago_pyramid_up##SUF(REAL *out, const REAL *in, int op, int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz,  \
                             double scale, void *stream) {                                                                  \
        return lago::pyramid_impl<REAL, true>(out, in, op, dim, rows, nx, ny, nz, scale, stream);                           \
    }
LAGO_DEFINE(float, _f32)
LAGO_DEFINE(double, _f64)
#undef LAGO_DEFINE
}
