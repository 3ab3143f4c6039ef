// Free-form deformation: a control lattice expanded to a dense field by its uniform cubic B-spline, and the adjoint
// (dense gradient -> control lattice) -- gfx950 HIP kernels.  No counterpart in the reference.
//
//   out[r, x, y, z]    = sum_{a, b, c} Wx[x, a] Wy[y, b] Wz[z, c] ctrl[r, a, b, c]          r = batch item x channel
//   d_ctrl[r, a, b, c] = sum_{x, y, z} Wx[x, a] Wy[y, b] Wz[z, c] g[r, x, y, z]
//
// with the banded per-axis matrices of ffd_weights.hpp: voxel x of an axis with spacing s has the taps i ... i + 3,
// i = x / s, weighed by the cubic B-spline at t = (x % s) / s.  2D fields are (y, z) with no x axis.  Both kernels work
// on voxel tiles of TX x TY x TZ = 8 x 8 x 64 (2D: 64 x 64) voxels of one row r, z the contiguous axis, 256 lanes a
// tile.  A tile reaches at most C_a = (T_a + s_a - 2) / s_a + 4 control points along axis a: that box of the lattice
// is what a workgroup keeps in LDS, and the LDS a launch asks for is sized from the spacings (a few KB at s >= 4, up
// to 115 KB for float64 at s = 1, where the lattice is as dense as the field).
//
// ffd_expand_kernel (forward; bound by its one store per voxel).  Per tile: the weights and tap offsets of the tile's
// TX + TY + TZ coordinates go to an LDS table (one ffd_axis per coordinate, none per voxel); the tile's control box is
// staged in LDS; then the three axes are contracted one after the other, non-contiguous axes first,
//      tmp[x][b][c]   = sum_a Wx[x, a] box[a][b][c]        4 taps, TX CY CZ sums        (3D only)
//      mid[x][y][c]   = sum_b Wy[y, b] tmp[x][b][c]        4 taps, TX TY CZ sums
//      out[x][y][z]   = sum_c Wz[z, c] mid[x][y][c]        4 taps per voxel, lane = z: the four weights of a lane stay in
//                                                          registers over the tile's 64 rows, a wave stores one whole row
// Every 4-tap sum runs tap 0 first: the product w_0 v_0, then one fma per tap, ascending (ffd_dot4).  x innermost, then
// y, then z: a fixed order without atomics, so the bits repeat from call to call, on any stream.
//
// ffd_restrict_tile_kernel + ffd_restrict_sum_kernel (adjoint; bound by its one load per voxel).  A workgroup loads its
// voxel tile of g once (coalesced rows, zero beyond the grid) and reduces it in LDS, contiguous axis first:
//      p1[y][c][x]    = sum_{z in tile} Wz[z, c] g[x][y][z]     lane = row (x, y), c wave-uniform: conflict-free reads of
//                                                               the tile (row stride 65) and wave-uniform loop bounds
//      p2[x][b][c]    = sum_{y in tile} Wy[y, b] p1[y][c][x]
//      part[a][b][c]  = sum_{x in tile} Wx[x, a] p2[x][b][c]    (3D only)
// Each sum is a gather: for its control point the taps q = 0 ... 3 in order (cell = point - q, so cells descending), the
// voxels of a cell ascending, acc = fma(w, v, acc) from 0 (ffd_gather_axis; four accumulators side by side, one per tap,
// with a full trip count for every lane measured the same at spacing 4 and 28 % slower at spacing 8).  The C_x C_y C_z
// partial sums of the tile go to the caller's scratch with plain stores -- no tile reads another tile's voxels, and no
// float atomic touches memory.  The second kernel owns one control point per lane and adds the partials of the tiles
// that reach it, tiles ascending (x slowest).  Control points that no voxel reaches, or only with weight 0, come out as
// exactly 0; the bits repeat from call to call.
//
// Every LDS index stays inside the launch's allocation for any spacing in 1..32 and any extent, partial tiles included:
// a coordinate l of a tile has the offset (g0 + l) / s - g0 / s <= (T - 1 + s - 1) / s = C - 4, whether or not the
// voxel exists, and control points beyond the lattice are staged as 0 and never loaded.
#include "common.hpp"
#include "ffd_weights.hpp"

namespace lago {

constexpr int kFfdTZ = 64;
template <int DIM> struct FfdTile {
    static constexpr int TX = DIM == 3 ? 8 : 1, TY = DIM == 3 ? 8 : 64, TZ = kFfdTZ, ROWS = TX * TY, COORDS = TX + TY + TZ;
};
static_assert(FfdTile<2>::ROWS == 64 && FfdTile<3>::ROWS == 64, "a wave of rows");

struct FfdGeom {
    int n[3], s[3], m[3];   // voxels, spacing, control points per axis (x, y, z); 2D: n[0] = s[0] = m[0] = 1
    int c[3];               // control points a tile reaches per axis (the LDS box); 2D: c[0] = 1
    uint32_t nt[3];         // tiles per axis
    uint32_t ntiles, nvox, mvox, bpr;   // tiles, voxels, control points of a row; blocks per row of the sum kernel
    FastDiv dtiles, dtyz, dtz;          // block -> row, tile
    FastDiv dcyz, dcz, dczx;            // box element -> (a, b, c); (CZ TX)
    FastDiv dmyz, dmz, dbpr;            // control point -> (a, b, c); block of the sum kernel -> row
};

template <typename R>
__device__ __forceinline__ R ffd_dot4(const R *w, R v0, R v1, R v2, R v3) {
    R acc = w[0] * v0;
    acc = lg_fma(w[1], v1, acc);
    acc = lg_fma(w[2], v2, acc);
    return lg_fma(w[3], v3, acc);
}

// the tile of this block: row, voxel origin o[], first control point lo[] of its box
struct FfdBlock {
    uint32_t row;
    int o[3], lo[3];
};
template <int DIM>
__device__ __forceinline__ FfdBlock ffd_block(const FfdGeom &g) {
    using T = FfdTile<DIM>;
    FfdBlock b;
    b.row = g.dtiles.div(blockIdx.x);
    const uint32_t t = blockIdx.x - b.row * g.ntiles;
    const uint32_t tx = g.dtyz.div(t), r = t - tx * (g.nt[1] * g.nt[2]);
    const uint32_t ty = g.dtz.div(r), tz = r - ty * g.nt[2];
    b.o[0] = (int)tx * T::TX;
    b.o[1] = (int)ty * T::TY;
    b.o[2] = (int)tz * T::TZ;
#pragma unroll
    for (int a = 0; a < 3; ++a) b.lo[a] = b.o[a] / g.s[a];
    return b;
}

template <typename R, int DIM>
__global__ __launch_bounds__(256) void ffd_expand_kernel(R *__restrict__ out, const R *__restrict__ ctrl, FfdGeom g) {
    using T = FfdTile<DIM>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ffd_smem[];
    const uint32_t CX = g.c[0], CY = g.c[1], CZ = g.c[2], P = CY * CZ;
    const uint32_t asz = (CX * CY > (uint32_t)T::ROWS ? CX * CY : (uint32_t)T::ROWS) * CZ;
    R *wt = reinterpret_cast<R *>(ffd_smem);   // [COORDS][4]
    R *A = wt + 4 * T::COORDS;                 // the control box [CX][CY][CZ] (3D), then mid [ROWS][CZ]
    R *B = A + asz;                            // tmp [TX][CY][CZ]; 2D: the control box [CY][CZ]
    int *off = reinterpret_cast<int *>(B + T::TX * P);   // [COORDS]
    const uint32_t tid = threadIdx.x;
    const FfdBlock b = ffd_block<DIM>(g);

    if (tid < (uint32_t)T::COORDS) {   // the tile's coordinates: x, then y, then z
        const int a = tid < (uint32_t)T::TX ? 0 : tid < (uint32_t)(T::TX + T::TY) ? 1 : 2;
        const int l = (int)tid - (a == 0 ? 0 : a == 1 ? T::TX : T::TX + T::TY);
        const int o = a == 0 ? b.o[0] : a == 1 ? b.o[1] : b.o[2], lo = a == 0 ? b.lo[0] : a == 1 ? b.lo[1] : b.lo[2];   // (no private array)
        const int x = o + l, s = a == 0 ? g.s[0] : a == 1 ? g.s[1] : g.s[2], i = x / s;
        const FfdAxis<R> ax = ffd_axis<R>(x - i * s, s);
        off[tid] = i - lo;
#pragma unroll
        for (int q = 0; q < 4; ++q) wt[4 * tid + q] = ax.w[q];
    }
    {   // the control box, zero beyond the lattice
        const R *src = ctrl + (size_t)b.row * g.mvox;
        R *dst = DIM == 3 ? A : B;
        for (uint32_t e = tid; e < CX * P; e += 256) {
            const uint32_t a = g.dcyz.div(e), bc = e - a * P, bb = g.dcz.div(bc), cc = bc - bb * CZ;
            const int ga = b.lo[0] + (int)a, gb = b.lo[1] + (int)bb, gc = b.lo[2] + (int)cc;
            R v = (R)0;
            if (ga < g.m[0] && gb < g.m[1] && gc < g.m[2]) v = src[((size_t)ga * g.m[1] + gb) * g.m[2] + gc];
            dst[e] = v;
        }
    }
    __syncthreads();
    if constexpr (DIM == 3) {
        for (uint32_t e = tid; e < (uint32_t)T::TX * P; e += 256) {
            const uint32_t x = g.dcyz.div(e), bc = e - x * P;
            const R *v = A + (uint32_t)off[x] * P + bc;
            B[e] = ffd_dot4(wt + 4 * x, v[0], v[P], v[2 * P], v[3 * P]);
        }
        __syncthreads();   // the box is dead: A becomes mid
    }
    for (uint32_t e = tid; e < (uint32_t)T::ROWS * CZ; e += 256) {
        const uint32_t xy = g.dcz.div(e), c = e - xy * CZ, x = xy / T::TY, y = xy % T::TY;
        const R *v = B + x * P + (uint32_t)off[T::TX + y] * CZ + c;
        A[e] = ffd_dot4(wt + 4 * (T::TX + y), v[0], v[CZ], v[2 * CZ], v[3 * CZ]);
    }
    __syncthreads();
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const int z = b.o[2] + (int)lane;
    if (z >= g.n[2]) return;   // (no barrier below)
    R wz[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wz[q] = wt[4 * (T::TX + T::TY + lane) + q];
    const uint32_t oz = (uint32_t)off[T::TX + T::TY + lane];
    R *dst = out + (size_t)b.row * g.nvox + (uint32_t)z;
    for (uint32_t r = wave; r < (uint32_t)T::ROWS; r += 4) {   // wave-uniform rows
        const int x = b.o[0] + (int)(r / T::TY), y = b.o[1] + (int)(r % T::TY);
        if (x >= g.n[0] || y >= g.n[1]) continue;
        const R *v = A + r * CZ + oz;
        dst[((size_t)x * g.n[1] + y) * g.n[2]] = ffd_dot4(wz, v[0], v[1], v[2], v[3]);
    }
}

// sum over the voxels [o, o + T) n [0, n) of one axis that reach control point `p` (global index) of the taps' products:
// val(l) is the value at tile coordinate l, W the axis' weight table [s][4]
template <typename R, typename Val>
__device__ __forceinline__ R ffd_gather_axis(const R *W, int p, int s, int o, int end, Val val) {
    R acc = (R)0;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
        const int first = (p - q) * s;   // the cell whose tap q is p (negative for cells before the grid: empty range)
        const int lo = first > o ? first : o, hi = first + s < end ? first + s : end;
        for (int x = lo; x < hi; ++x) acc = lg_fma(W[4 * (x - first) + q], val(x - o), acc);
    }
    return acc;
}

template <typename R, int DIM>
__global__ __launch_bounds__(256) void ffd_restrict_tile_kernel(R *__restrict__ scratch, const R *__restrict__ gin, FfdGeom g) {
    using T = FfdTile<DIM>;
    constexpr uint32_t LD = T::TZ + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char ffd_smem[];
    const uint32_t CX = g.c[0], CY = g.c[1], CZ = g.c[2], P = CY * CZ;
    R *W = reinterpret_cast<R *>(ffd_smem);   // [3][kFfdMaxSpacing][4]
    R *G = W + 3 * kFfdMaxSpacing * 4;        // the voxel tile [ROWS][LD]
    R *P1 = G + T::ROWS * LD;                 // [TY][CZ][TX]
    R *P2 = P1 + T::ROWS * CZ;                // [TX][CY][CZ] (3D)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const FfdBlock b = ffd_block<DIM>(g);
    int end[3];   // the tile's end, cut at the grid
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int full = b.o[a] + (a == 0 ? T::TX : a == 1 ? T::TY : T::TZ);
        end[a] = full < g.n[a] ? full : g.n[a];
    }

    if (tid < 3u * kFfdMaxSpacing) {
        const int a = (int)tid / kFfdMaxSpacing, r = (int)tid % kFfdMaxSpacing;
        if (r < g.s[a]) {
            const FfdAxis<R> ax = ffd_axis<R>(r, g.s[a]);
#pragma unroll
            for (int q = 0; q < 4; ++q) W[4 * tid + q] = ax.w[q];
        }
    }
    {
        const R *src = gin + (size_t)b.row * g.nvox;
        const int z = b.o[2] + (int)lane;
        R v[T::ROWS / 4];   // a wave's 16 rows: every load is issued before the first LDS store waits for one
#pragma unroll
        for (int k = 0; k < T::ROWS / 4; ++k) {
            const uint32_t r = wave + 4u * k;
            const int x = b.o[0] + (int)(r / T::TY), y = b.o[1] + (int)(r % T::TY);
            v[k] = (R)0;
            if (x < g.n[0] && y < g.n[1] && z < g.n[2]) v[k] = src[((size_t)x * g.n[1] + y) * g.n[2] + (uint32_t)z];
        }
#pragma unroll
        for (int k = 0; k < T::ROWS / 4; ++k) G[(wave + 4u * k) * LD + lane] = v[k];
    }
    __syncthreads();
    {   // z: lane = row, c wave-uniform
        const R *Wz = W + 2 * kFfdMaxSpacing * 4, *mine = G + lane * LD;
        const uint32_t x = lane / T::TY, y = lane % T::TY;
        for (uint32_t c = wave; c < CZ; c += 4)
            P1[(y * CZ + c) * T::TX + x] = ffd_gather_axis<R>(Wz, b.lo[2] + (int)c, g.s[2], b.o[2], end[2], [&](int l) { return mine[l]; });
    }
    __syncthreads();
    {   // y: element (b, c, x), lanes along (c, x)
        const R *Wy = W + kFfdMaxSpacing * 4;
        const uint32_t czx = CZ * T::TX;
        R *dst = DIM == 3 ? P2 : scratch + (size_t)blockIdx.x * (CX * P);
        for (uint32_t e = tid; e < CY * czx; e += 256) {
            const uint32_t bb = g.dczx.div(e), cx = e - bb * czx;
            const R *col = P1 + cx;
            const R acc = ffd_gather_axis<R>(Wy, b.lo[1] + (int)bb, g.s[1], b.o[1], end[1], [&](int l) { return col[(uint32_t)l * czx]; });
            if constexpr (DIM == 3) dst[(cx % T::TX) * P + bb * CZ + cx / T::TX] = acc;
            else dst[e] = acc;
        }
    }
    if constexpr (DIM == 3) {
        __syncthreads();
        R *dst = scratch + (size_t)blockIdx.x * (CX * P);
        for (uint32_t e = tid; e < CX * P; e += 256) {
            const uint32_t a = g.dcyz.div(e), bc = e - a * P;
            const R *col = P2 + bc;
            dst[e] = ffd_gather_axis<R>(W, b.lo[0] + (int)a, g.s[0], b.o[0], end[0], [&](int l) { return col[(uint32_t)l * P]; });
        }
    }
}

// the tiles along one axis that hold a voxel reaching control point p: voxels [(p - 3) s, (p + 1) s) n [0, n)
template <int TT>
__device__ __forceinline__ void ffd_tile_range(int p, int s, int n, int &t0, int &t1) {
    const int v0 = (p - 3) * s > 0 ? (p - 3) * s : 0, v1 = (p + 1) * s - 1 < n - 1 ? (p + 1) * s - 1 : n - 1;
    t0 = v0 / TT;
    t1 = v1 / TT;   // v0 <= v1 for every p of the lattice: (m - 4) s <= n - 1
}

template <typename R, int DIM>
__global__ __launch_bounds__(256) void ffd_restrict_sum_kernel(R *__restrict__ d_ctrl, const R *__restrict__ scratch, FfdGeom g) {
    using T = FfdTile<DIM>;
    const uint32_t row = g.dbpr.div(blockIdx.x), p = (blockIdx.x - row * g.bpr) * 256u + threadIdx.x;
    if (p >= g.mvox) return;
    const uint32_t a = g.dmyz.div(p), bc = p - a * (uint32_t)(g.m[1] * g.m[2]), bb = g.dmz.div(bc), cc = bc - bb * (uint32_t)g.m[2];
    int x0, x1, y0, y1, z0, z1;
    ffd_tile_range<T::TX>((int)a, g.s[0], g.n[0], x0, x1);
    ffd_tile_range<T::TY>((int)bb, g.s[1], g.n[1], y0, y1);
    ffd_tile_range<T::TZ>((int)cc, g.s[2], g.n[2], z0, z1);
    const uint32_t CY = g.c[1], CZ = g.c[2], box = (uint32_t)g.c[0] * CY * CZ;
    const R *src = scratch + (size_t)row * g.ntiles * box;
    R acc = (R)0;
    for (int tx = x0; tx <= x1; ++tx) {
        const uint32_t la = a - (uint32_t)(tx * T::TX / g.s[0]);
        for (int ty = y0; ty <= y1; ++ty) {
            const uint32_t lb = bb - (uint32_t)(ty * T::TY / g.s[1]);
            for (int tz = z0; tz <= z1; ++tz) {
                const uint32_t lc = cc - (uint32_t)(tz * T::TZ / g.s[2]);
                const uint32_t tile = ((uint32_t)tx * g.nt[1] + (uint32_t)ty) * g.nt[2] + (uint32_t)tz;
                acc += src[(size_t)tile * box + (la * CY + lb) * CZ + lc];
            }
        }
    }
    d_ctrl[(size_t)row * g.mvox + p] = acc;
}

// The checks every entry point shares, before any device call.  LAGO_OK with `empty` set: nothing to do.
static int ffd_geom(const char *what, FfdGeom &g, bool &empty, int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz,
                    int sx, int sy, int sz) {
    Volume v;
    if (const int rc = check_volume(v, what, dim, nx, ny, nz, kPlane29, {rows})) return rc;
    if (dim == 2) sz = sy, sy = sx, sx = 1;   // the spacings follow the extents to (1, H, W)
    if (sx < 1 || sx > kFfdMaxSpacing || sy < 1 || sy > kFfdMaxSpacing || sz < 1 || sz > kFfdMaxSpacing)
        return fail_invalid("%s: a spacing outside 1..%d", what, kFfdMaxSpacing);
    empty = rows == 0 || v.nvox == 0;
    if (empty) return LAGO_OK;
    if (rows >= (1ll << 31)) return fail_invalid("%s: 2^31 rows or more", what);
    const int64_t n[3] = {v.nx, v.ny, v.nz};
    const int s[3] = {sx, sy, sz};
    const int tile[3] = {dim == 3 ? FfdTile<3>::TX : FfdTile<2>::TX, dim == 3 ? FfdTile<3>::TY : FfdTile<2>::TY, kFfdTZ};
    int64_t mvox = 1, ntiles = 1;
    for (int a = 0; a < 3; ++a) {
        const bool none = dim == 2 && a == 0;   // no x axis
        g.n[a] = (int)n[a];
        g.s[a] = s[a];
        g.m[a] = none ? 1 : (int)ffd_ctrl_extent(n[a], s[a]);
        g.c[a] = none ? 1 : (tile[a] + s[a] - 2) / s[a] + 4;
        g.nt[a] = (uint32_t)((n[a] + tile[a] - 1) / tile[a]);
        mvox *= g.m[a];
        ntiles *= g.nt[a];
    }
    if (mvox >= (1ll << 31)) return fail_invalid("%s: a control grid of 2^31 points or more", what);
    const int64_t bpr = (mvox + 255) / 256;
    if (ntiles * rows >= (1ll << 31) || bpr * rows >= (1ll << 31)) return fail_invalid("%s: too many tiles for one launch", what);
    g.ntiles = (uint32_t)ntiles;
    g.nvox = (uint32_t)v.nvox;
    g.mvox = (uint32_t)mvox;
    g.bpr = (uint32_t)bpr;
    g.dtiles = FastDiv(g.ntiles);
    g.dtyz = FastDiv(g.nt[1] * g.nt[2]);
    g.dtz = FastDiv(g.nt[2]);
    g.dcyz = FastDiv((uint32_t)(g.c[1] * g.c[2]));
    g.dcz = FastDiv((uint32_t)g.c[2]);
    g.dczx = FastDiv((uint32_t)(g.c[2] * tile[0]));
    g.dmyz = FastDiv((uint32_t)(g.m[1] * g.m[2]));
    g.dmz = FastDiv((uint32_t)g.m[2]);
    g.dbpr = FastDiv(g.bpr);
    return LAGO_OK;
}

static int64_t ffd_box(const FfdGeom &g) { return (int64_t)g.c[0] * g.c[1] * g.c[2]; }

template <typename R>
static int ffd_expand_impl(R *out, const R *ctrl, int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz, int sx, int sy,
                           int sz, void *stream) {
    FfdGeom g;
    bool empty;
    if (const int rc = ffd_geom("ffd_expand", g, empty, dim, rows, nx, ny, nz, sx, sy, sz)) return rc;
    if (empty) return LAGO_OK;   // nothing to write
    if (!out || !ctrl) return fail_invalid("ffd_expand: null pointer");
    if (overlaps(out, (size_t)rows * g.nvox * sizeof(R), ctrl, (size_t)rows * g.mvox * sizeof(R)))
        return fail_invalid("ffd_expand: out must not overlap the control grid");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    with_dim(dim, [&](auto DIM) {
        using T = FfdTile<DIM()>;
        const size_t cxy = (size_t)g.c[0] * g.c[1], asz = (cxy > (size_t)T::ROWS ? cxy : (size_t)T::ROWS) * g.c[2];
        const size_t smem = (4 * T::COORDS + asz + (size_t)T::TX * g.c[1] * g.c[2]) * sizeof(R) + T::COORDS * sizeof(int);
        e = launch(ffd_expand_kernel<R, DIM()>, dim3(g.ntiles * (uint32_t)rows), dim3(256), smem, s, out, ctrl, g);
    });
    return launched(e, s, "ffd_expand");
}

template <typename R>
static int ffd_expand_adjoint_impl(R *d_ctrl, const R *go, R *scratch, int64_t scratch_elems, int dim, int64_t rows, int64_t nx,
                                   int64_t ny, int64_t nz, int sx, int sy, int sz, void *stream) {
    FfdGeom g;
    bool empty;
    if (const int rc = ffd_geom("ffd_expand_adjoint", g, empty, dim, rows, nx, ny, nz, sx, sy, sz)) return rc;
    if (empty) return LAGO_OK;   // no voxel, or no row
    if (!d_ctrl || !go || !scratch) return fail_invalid("ffd_expand_adjoint: null pointer");
    const int64_t need = rows * (int64_t)g.ntiles * ffd_box(g);
    if (scratch_elems < need)
        return fail_invalid("ffd_expand_adjoint: scratch of %lld elements, %lld needed (lago_ffd_scratch_elems)", (long long)scratch_elems,
                            (long long)need);
    const size_t cb = (size_t)rows * g.mvox * sizeof(R), gb = (size_t)rows * g.nvox * sizeof(R), sb = (size_t)need * sizeof(R);
    if (any_overlap({{d_ctrl, cb}, {scratch, sb}}, {{go, gb}}))
        return fail_invalid("ffd_expand_adjoint: d_ctrl, grad_out and scratch must not overlap");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    with_dim(dim, [&](auto DIM) {
        using T = FfdTile<DIM()>;
        const size_t smem = (3 * kFfdMaxSpacing * 4 + (size_t)T::ROWS * (T::TZ + 1) + (size_t)T::ROWS * g.c[2] +
                             (DIM() == 3 ? (size_t)T::TX * g.c[1] * g.c[2] : 0)) * sizeof(R);
        e = launch(ffd_restrict_tile_kernel<R, DIM()>, dim3(g.ntiles * (uint32_t)rows), dim3(256), smem, s, scratch, go, g);
        if (e == hipSuccess)
            e = launch(ffd_restrict_sum_kernel<R, DIM()>, dim3(g.bpr * (uint32_t)rows), dim3(256), 0, s, d_ctrl, (const R *)scratch, g);
    });
    return launched(e, s, "ffd_expand_adjoint");
}

}  // namespace lago

extern "C" {
long long lago_ffd_scratch_elems(int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz, int sx, int sy, int sz) {
    lago::FfdGeom g;
    bool empty;
    if (lago::ffd_geom("ffd_scratch_elems", g, empty, dim, rows, nx, ny, nz, sx, sy, sz)) return -1;
    return empty ? 0 : rows * (int64_t)g.ntiles * lago::ffd_box(g);
}
#define LAGO_DEFINE(REAL, SUF)                                                                                           \
    int lago_ffd_expand##SUF(REAL *out, const REAL *ctrl, int dim, int64_t rows, int64_t nx, int64_t ny, int64_t nz,     \
                             int sx, int sy, int sz, void *stream) {                                                     \
        return lago::ffd_expand_impl<REAL>(out, ctrl, dim, rows, nx, ny, nz, sx, sy, sz, stream);                        \
    }                                                                                                                    \
    int lago_ffd_expand_adjoint##SUF(REAL *d_ctrl, const REAL *grad_out, REAL *scratch, int64_t scratch_elems, int dim,  \
                                     int64_t rows, int64_t nx, int64_t ny, int64_t nz, int sx, int sy, int sz,           \
                                     void *stream) {                                                                     \
        return lago::ffd_expand_adjoint_impl<REAL>(d_ctrl, grad_out, scratch, scratch_elems, dim, rows, nx, ny, nz, sx,  \
                                                   sy, sz, stream);                                                      \
    }
LAGO_DEFINE(float, _f32)
LAGO_DEFINE(double, _f64)
#undef LAGO_DEFINE
}
