// Diffusion and bending energy of a field u (nn, nc, sp) and the operator A of E = <u, A u> / V -- gfx950 HIP kernels.
// No counterpart in the reference.  The definition is in include/lagomorph_hip.h (lago_field_energy); the arithmetic of
// one voxel, its evaluation order and its rounding count are in energy_stencil.hpp, which a host compiler builds too.
//
// Every kernel works on voxel tiles of TX x TY x TZ = 8 x 8 x 64 (dim 2: 64 x 64) voxels of one channel plane, z the
// contiguous axis, 256 lanes a tile, lane = z: a wave owns a row (x, y) of the tile at a time, so the x and y
// predicates are wave-uniform and a lane's z predicates are the same for all its rows.  The tile is staged in LDS with
// its halo, every coordinate clamped (halo_tile.hpp): one voxel on the high side for the diffusion energy, one on each
// side for the bending energy and the diffusion operator, two for the bending operator (12 x 12 x 68 cells, 38 KB in
// float32, 77 KB in float64).  A voxel then reads its 4 to 25 neighbours from LDS at compile-time offsets.
//
// energy_tile_kernel + energy_sum_kernel.  Every lane adds the densities of its voxels, rows ascending, in the field's
// precision; the lanes' sums are added in double -- within a wave by a fixed shuffle tree, the four waves ascending --
// and the tile's sum goes to the caller's scratch with a plain store (one element of R per tile: nn nc tiles).  The
// second kernel has one workgroup per item: lane t adds the partials t, t + 256, ... of the item's nc tiles-per-plane
// partials ascending in double, the same tree adds the lanes, and E[n] = sum / V is written in the field's precision.
// No atomics: the bits repeat from call to call, on any stream.
//
// energy_operator_kernel.  out = scale[n] (A u): one load (plus the halo, from cache) and one store per element.
//
// Every LDS index stays inside the launch's allocation: a tile voxel's cell is at least LO cells from every face of the
// staged box and the header reads offsets within -LO ... +HI only (EnergyHalo below ties the halo to the kind).
// Every global index is a clamped coordinate or a coordinate tested against the extents.
#include "common.hpp"
#include "energy_stencil.hpp"
#include "halo_tile.hpp"

#include <cmath>

namespace lago {

constexpr int kEnergyTZ = 64;
template <int DIM> struct EnergyTile {
    static constexpr int TX = DIM == 3 ? 8 : 1, TY = DIM == 3 ? 8 : 64, TZ = kEnergyTZ, ROWS = TX * TY;
};
static_assert(EnergyTile<2>::ROWS == 64 && EnergyTile<3>::ROWS == 64, "16 rows a wave");

struct EnergyGeom {
    int n[3];                       // voxels per axis (x, y, z); 2D: n[0] = 1
    uint32_t nt[3];                 // tiles per axis
    uint32_t ntiles, nvox, nc, nblocks;   // tiles and voxels of a plane, channels, tiles in all
    FastDiv dtiles, dtyz, dtz, dnc;
};

// halo of the staged tile: what the header reads for this kind (energy: forward differences only for diffusion)
template <int KIND, bool OPERATOR> struct EnergyHalo {
    static constexpr int LO = KIND == kEnergyBending ? (OPERATOR ? 2 : 1) : (OPERATOR ? 1 : 0);
    static constexpr int HI = KIND == kEnergyBending && OPERATOR ? 2 : 1;
};
template <typename R, int DIM, int KIND, bool OPERATOR>
using EnergyHaloTile = HaloTile<R, DIM, EnergyTile<DIM>::TX, EnergyTile<DIM>::TY, EnergyTile<DIM>::TZ, EnergyHalo<KIND, OPERATOR>::LO,
                                EnergyHalo<KIND, OPERATOR>::HI>;

struct EnergyBlock {
    uint32_t id, plane;   // logical block (the scratch slot), channel plane n nc + k
    int o[3];
};
template <int DIM>
__device__ __forceinline__ EnergyBlock energy_block(const EnergyGeom &g) {
    using T = EnergyTile<DIM>;
    EnergyBlock b;
    b.id = xcd_swizzle(blockIdx.x, g.nblocks);
    b.plane = g.dtiles.div(b.id);
    const uint32_t t = b.id - b.plane * g.ntiles;
    const uint32_t tx = g.dtyz.div(t), r = t - tx * (g.nt[1] * g.nt[2]);
    const uint32_t ty = g.dtz.div(r), tz = r - ty * g.nt[2];
    b.o[0] = (int)tx * T::TX;
    b.o[1] = (int)ty * T::TY;
    b.o[2] = (int)tz * T::TZ;
    return b;
}

// the sum of v over the workgroup's 256 lanes in a fixed order (valid in thread 0): a wave's lanes by the shuffle tree
// 32, 16, ... 1, then the four waves ascending
__device__ __forceinline__ double energy_block_sum(double v, double *waves) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63u) == 0) waves[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((waves[0] + waves[1]) + waves[2]) + waves[3];
}

template <typename R, int DIM, int KIND>
__global__ __launch_bounds__(256) void energy_tile_kernel(R *__restrict__ scratch, const R *__restrict__ u, EnergyGeom g, EnergyWeights<R> w) {
    using T = EnergyTile<DIM>;
    using H = EnergyHaloTile<R, DIM, KIND, false>;
    extern __shared__ __attribute__((aligned(16))) unsigned char energy_smem[];
    __shared__ double waves[4];
    R *tile = reinterpret_cast<R *>(energy_smem);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (a scalar: the rows are wave-uniform)
    const EnergyBlock b = energy_block<DIM>(g);
    H::stage(tile, u + (size_t)b.plane * g.nvox, b.o, g.n, tid, 256u);
    __syncthreads();
    const int z = b.o[2] + (int)lane;
    R acc = (R)0;
    if (z < g.n[2]) {
        EnergyMask<R> q[3];
        q[2] = energy_mask<R>(z, g.n[2]);
        for (uint32_t r = wave; r < (uint32_t)T::ROWS; r += 4) {   // wave-uniform rows
            const uint32_t lx = r / T::TY, ly = r % T::TY;
            const int x = b.o[0] + (int)lx, y = b.o[1] + (int)ly;
            if (x >= g.n[0] || y >= g.n[1]) continue;
            const R *c = tile + H::cell(lx, ly, lane);
            auto at = [&](int dx, int dy, int dz) { return c[(dx * H::PY + dy) * H::LD + dz]; };
            if constexpr (KIND == kEnergyBending) {
                q[0] = energy_mask<R>(x, g.n[0]);
                q[1] = energy_mask<R>(y, g.n[1]);
                acc = acc + energy_bending_density<R, DIM>(w, q, at);
            } else {
                acc = acc + energy_diffusion_density<R, DIM>(w, at);
            }
        }
    }
    const double sum = energy_block_sum((double)acc, waves);
    if (tid == 0) scratch[b.id] = (R)sum;
}

template <typename R>
__global__ __launch_bounds__(256) void energy_sum_kernel(R *__restrict__ energy, const R *__restrict__ scratch, uint32_t per_item, double nvox) {
    __shared__ double waves[4];
    const R *src = scratch + (size_t)blockIdx.x * per_item;
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < per_item; i += 256) acc += (double)src[i];
    const double sum = energy_block_sum(acc, waves);
    if (threadIdx.x == 0) energy[blockIdx.x] = (R)(sum / nvox);
}

template <typename R, int DIM, int KIND>
__global__ __launch_bounds__(256) void energy_operator_kernel(R *__restrict__ out, const R *__restrict__ u, const R *__restrict__ scale,
                                                              EnergyGeom g, EnergyWeights<R> w) {
    using T = EnergyTile<DIM>;
    using H = EnergyHaloTile<R, DIM, KIND, true>;
    extern __shared__ __attribute__((aligned(16))) unsigned char energy_smem[];
    R *tile = reinterpret_cast<R *>(energy_smem);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (a scalar: the rows are wave-uniform)
    const EnergyBlock b = energy_block<DIM>(g);
    H::stage(tile, u + (size_t)b.plane * g.nvox, b.o, g.n, tid, 256u);
    __syncthreads();
    const int z = b.o[2] + (int)lane;
    if (z >= g.n[2]) return;   // (no barrier below)
    const R s = scale ? scale[g.dnc.div(b.plane)] : (R)1;
    EnergyMask<R> q[3];
    q[2] = energy_mask<R>(z, g.n[2]);
    R *dst = out + (size_t)b.plane * g.nvox + (uint32_t)z;
    for (uint32_t r = wave; r < (uint32_t)T::ROWS; r += 4) {   // wave-uniform rows
        const uint32_t lx = r / T::TY, ly = r % T::TY;
        const int x = b.o[0] + (int)lx, y = b.o[1] + (int)ly;
        if (x >= g.n[0] || y >= g.n[1]) continue;
        const R *c = tile + H::cell(lx, ly, lane);
        auto at = [&](int dx, int dy, int dz) { return c[(dx * H::PY + dy) * H::LD + dz]; };
        R v;
        if constexpr (KIND == kEnergyBending) {
            q[0] = energy_mask<R>(x, g.n[0]);
            q[1] = energy_mask<R>(y, g.n[1]);
            v = energy_bending_apply<R, DIM>(w, q, at);
        } else {
            v = energy_diffusion_apply<R, DIM>(w, at);
        }
        dst[((size_t)x * g.n[1] + y) * g.n[2]] = s * v;
    }
}

// The checks every entry point shares, before any device call.  LAGO_OK with `empty` set: nothing to do.  h: the
// spacings of the axes as laid out in memory (x, y, z)
static int energy_geom(const char *what, EnergyGeom &g, bool &empty, double (&h)[3], int kind, int dim, int64_t nn, int64_t nc, int64_t nx,
                       int64_t ny, int64_t nz, const double *spacing, bool need_spacing) {
    Volume v;
    if (const int rc = check_volume(v, what, dim, nx, ny, nz, kPlane29, {nn, nc})) return rc;
    if (kind != kEnergyDiffusion && kind != kEnergyBending) return fail_invalid("%s: unknown kind %d (LAGO_ENERGY_DIFFUSION, LAGO_ENERGY_BENDING)", what, kind);
    h[0] = h[1] = h[2] = 1.0;
    if (need_spacing) {
        if (!spacing) return fail_invalid("%s: null pointer (spacing)", what);
        for (int a = 0; a < dim; ++a) {
            if (!(spacing[a] > 0.0) || !std::isfinite(spacing[a])) return fail_invalid("%s: a spacing that is not positive and finite", what);
            h[3 - dim + a] = spacing[a];   // the spacings follow the extents to (1, H, W)
        }
    }
    empty = nn == 0 || nc == 0 || v.nvox == 0;
    if (empty) return LAGO_OK;
    const int64_t n[3] = {v.nx, v.ny, v.nz};
    const int tile[3] = {dim == 3 ? EnergyTile<3>::TX : EnergyTile<2>::TX, dim == 3 ? EnergyTile<3>::TY : EnergyTile<2>::TY, kEnergyTZ};
    int64_t ntiles = 1;
    for (int a = 0; a < 3; ++a) {
        g.n[a] = (int)n[a];
        g.nt[a] = (uint32_t)((n[a] + tile[a] - 1) / tile[a]);
        ntiles *= g.nt[a];
    }
    int64_t planes, blocks;
    if (nn >= (1ll << 31) || __builtin_mul_overflow(nn, nc, &planes) || __builtin_mul_overflow(planes, ntiles, &blocks) || blocks >= (1ll << 31))
        return fail_invalid("%s: too many tiles for one launch", what);
    g.ntiles = (uint32_t)ntiles;
    g.nvox = (uint32_t)v.nvox;
    g.nc = (uint32_t)nc;
    g.nblocks = (uint32_t)blocks;
    g.dtiles = FastDiv(g.ntiles);
    g.dtyz = FastDiv(g.nt[1] * g.nt[2]);
    g.dtz = FastDiv(g.nt[2]);
    g.dnc = FastDiv(g.nc);
    return LAGO_OK;
}

template <typename R>
static int field_energy_impl(R *energy, const R *u, R *scratch, int64_t scratch_elems, int kind, int dim, int64_t nn, int64_t nc, int64_t nx,
                             int64_t ny, int64_t nz, const double *spacing, void *stream) {
    EnergyGeom g;
    bool empty;
    double h[3];
    if (const int rc = energy_geom("field_energy", g, empty, h, kind, dim, nn, nc, nx, ny, nz, spacing, true)) return rc;
    if (empty) return LAGO_OK;   // nothing is written
    if (!energy || !u || !scratch) return fail_invalid("field_energy: null pointer");
    const int64_t need = (int64_t)g.nblocks;
    if (scratch_elems < need)
        return fail_invalid("field_energy: scratch of %lld elements, %lld needed (lago_field_energy_scratch_elems)", (long long)scratch_elems,
                            (long long)need);
    const size_t ub = (size_t)nn * nc * g.nvox * sizeof(R);
    if (any_overlap({{energy, (size_t)nn * sizeof(R)}, {scratch, (size_t)need * sizeof(R)}}, {{u, ub}}))
        return fail_invalid("field_energy: energy, scratch and u must not overlap");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    const EnergyWeights<R> w = energy_weights<R>(kind, h);
    with_dim(dim, [&](auto DIM) {
        with_flags([&](auto BENDING) {
            constexpr int KIND = BENDING() ? kEnergyBending : kEnergyDiffusion;
            using H = EnergyHaloTile<R, DIM(), KIND, false>;
            e = launch(energy_tile_kernel<R, DIM(), KIND>, dim3(g.nblocks), dim3(256), (size_t)H::CELLS * sizeof(R), s, scratch, u, g, w);
        }, kind == kEnergyBending);
    });
    if (e == hipSuccess)
        e = launch(energy_sum_kernel<R>, dim3((uint32_t)nn), dim3(256), 0, s, energy, (const R *)scratch, g.nc * g.ntiles, (double)g.nvox);
    return launched(e, s, "field_energy");
}

template <typename R>
static int field_energy_operator_impl(R *out, const R *u, const R *scale, int kind, int dim, int64_t nn, int64_t nc, int64_t nx, int64_t ny,
                                      int64_t nz, const double *spacing, void *stream) {
    EnergyGeom g;
    bool empty;
    double h[3];
    if (const int rc = energy_geom("field_energy_operator", g, empty, h, kind, dim, nn, nc, nx, ny, nz, spacing, true)) return rc;
    if (empty) return LAGO_OK;   // nothing is written
    if (!out || !u) return fail_invalid("field_energy_operator: null pointer");
    const size_t ub = (size_t)nn * nc * g.nvox * sizeof(R);
    if (any_overlap({{out, ub}}, {{u, ub}, {scale, (size_t)nn * sizeof(R)}}))
        return fail_invalid("field_energy_operator: out must not overlap u or scale");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    const EnergyWeights<R> w = energy_weights<R>(kind, h);
    with_dim(dim, [&](auto DIM) {
        with_flags([&](auto BENDING) {
            constexpr int KIND = BENDING() ? kEnergyBending : kEnergyDiffusion;
            using H = EnergyHaloTile<R, DIM(), KIND, true>;
            e = launch(energy_operator_kernel<R, DIM(), KIND>, dim3(g.nblocks), dim3(256), (size_t)H::CELLS * sizeof(R), s, out, u, scale, g, w);
        }, kind == kEnergyBending);
    });
    return launched(e, s, "field_energy_operator");
}

}  // namespace lago

extern "C" {
long long lago_field_energy_scratch_elems(int kind, int dim, int64_t nn, int64_t nc, int64_t nx, int64_t ny, int64_t nz) {
    lago::EnergyGeom g;
    bool empty;
    double h[3];
    if (lago::energy_geom("field_energy_scratch_elems", g, empty, h, kind, dim, nn, nc, nx, ny, nz, nullptr, false)) return -1;
    return empty ? 0 : (long long)g.nblocks;
}
#define LAGO_DEFINE(REAL, SUF)                                                                                               \
    int lago_field_energy##SUF(REAL *energy, const REAL *u, REAL *scratch, int64_t scratch_elems, int kind, int dim,          \
                               int64_t nn, int64_t nc, int64_t nx, int64_t ny, int64_t nz, const double *spacing,             \
                               void *stream) {                                                                               \
        return lago::field_energy_impl<REAL>(energy, u, scratch, scratch_elems, kind, dim, nn, nc, nx, ny, nz, spacing,       \
                                             stream);                                                                        \
    }                                                                                                                        \
    int lago_field_energy_operator##SUF(REAL *out, const REAL *u, const REAL *scale, int kind, int dim, int64_t nn,           \
                                        int64_t nc, int64_t nx, int64_t ny, int64_t nz, const double *spacing,                \
                                        void *stream) {                                                                      \
        return lago::field_energy_operator_impl<REAL>(out, u, scale, kind, dim, nn, nc, nx, ny, nz, spacing, stream);         \
    }
LAGO_DEFINE(float, _f32)
LAGO_DEFINE(double, _f64)
#undef LAGO_DEFINE
}
