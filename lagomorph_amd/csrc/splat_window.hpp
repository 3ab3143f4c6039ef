// The frame the LDS-window splat kernels share (splat.hip, affine.hip's box kernel, interp.hip's 2D splat).
//
// Every one of them accumulates the corner contributions of a tile of source voxels in a float64 LDS window
// (why float64: splat.hip) and flushes the touched cells with one global atomic each.  What they have in common is
// written once here: the workgroup -> tile decode, the reference's sequentially flipped weights, the sheared window's
// placement, its eight adds, the eight clamped atomics of a footprint that misses it, and the two flushes.  What makes
// a kernel what it is (loop structure, what it keeps in registers, its scheduling fences) stays in the kernel.
#pragma once
#include "common.hpp"

namespace lago {

__device__ __forceinline__ void lds_add(double *p, double v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Sequentially flipped weights (include/interp.h:431-453) times the voxel's grad_out value: x outer, y, z inner.
// ddx, ddy, ddz = 1 - fraction.
template <typename R>
__device__ __forceinline__ void flipped_weights(R (&w)[8], R ddx, R ddy, R ddz, R gv) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        w[q] = (ddx * ddy * ddz) * gv;
        ddz = (R)1.f - ddz;
        if (q & 1) ddy = (R)1.f - ddy;
        if ((q & 3) == 3) ddx = (R)1.f - ddx;
    }
}

// workgroup -> (batch item, tile) for a geometry with ntx / nty / ntz tiles of TX x TY x TZ voxels per item of an
// snx x sny x snz grid (TileGeom, ShearGeom): origin and the extent that lies inside the grid
struct TileAt {
    uint32_t n;
    int x0, y0, z0, ex, ey, ez;
};
template <typename G>
__device__ __forceinline__ TileAt tile_at(const G &g, int snx, int sny, int snz) {
    const uint32_t L = block_order(blockIdx.x, g.total, g.rev);
    const uint32_t n = g.d_tiles.div(L);
    uint32_t r = L - n * g.tiles_per_item;
    const uint32_t bx = g.d_tyz.div(r);
    r -= bx * (g.nty * g.ntz);
    const uint32_t by = g.d_tz.div(r);
    const uint32_t bz = r - by * g.ntz;
    const int x0 = bx * g.TX, y0 = by * g.TY, z0 = bz * g.TZ;
    return {n, x0, y0, z0, min(g.TX, snx - x0), min(g.TY, sny - y0), min(g.TZ, snz - z0)};
}

// Flush of one window row by one wave, lanes along the row: one atomic per non-zero cell.  The kernels walk their rows
// one wave per row, so that the row decode and both base addresses are wave-uniform (scalar); REZERO leaves the row
// zeroed for the next channel.
template <bool REZERO, typename R>
__device__ __forceinline__ void flush_row(double *wrow, R *grow, int len) {
    for (int lz = threadIdx.x & 63; lz < len; lz += 64) {
        const double acc = wrow[lz];
        if (acc != 0.0) {
            if (REZERO) wrow[lz] = 0.0;
            atomic_add(grow + lz, (R)acc);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The sheared window (float32 displacement fields; the scheme is described in splat.hip).
struct ShearGeom {
    int nx, ny, nz;
    int TX, TY, TZ;        // source tile
    int WX, WY, WZ;        // window cells; x / y in virtual coordinates [-1, n], z inside the grid
    int MX, MY, MZ;
    int nseg;              // 16-cell z segments of the window
    uint32_t ntx, nty, ntz, tiles_per_item, total, tile_vox, win_cells;
    int rev;               // launch direction (common.hpp)
    FastDiv d_tiles, d_tyz, d_tz, d_TyTz, d_Tz, d_wy;
};

// Placement: returns the window's z origin -- 16-aligned (flush rows start on 64-byte boundaries), inside the grid --
// and has the first nseg threads write the (x, y) origin of every z segment, the displacement of the tile's centre
// column at the segment's height, into org[] (read after the caller's next barrier).
__device__ __forceinline__ int shear_place(int2 *org, const ShearGeom &sg, const TileAt &tl, const float *un, double dt,
                                           int wez) {
    const int nx = sg.nx, ny = sg.ny, nz = sg.nz;
    const uint32_t nv = (uint32_t)nx * ny * nz;
    const int cxs = tl.x0 + tl.ex / 2, cys = tl.y0 + tl.ey / 2;
    int wz0;
    {
        const float fdt = (float)dt;
        const size_t sc = ((size_t)cxs * ny + cys) * nz + (tl.z0 + tl.ez / 2);
        const int bzo = tl.z0 + (int)floorf(fdt * un[sc + 2 * (size_t)nv]);
        wz0 = max(0, min((bzo - sg.MZ) & ~15, nz - wez));
    }
    if ((int)threadIdx.x < sg.nseg) {
        const float fdt = (float)dt;
        const int zc = min(wz0 + (int)threadIdx.x * 16 + 8, nz - 1);
        const size_t sc = ((size_t)cxs * ny + cys) * nz + zc;
        int2 o;
        o.x = max(-1, min(tl.x0 + (int)floorf(fdt * un[sc]) - sg.MX, nx + 1 - sg.WX));
        o.y = max(-1, min(tl.y0 + (int)floorf(fdt * un[sc + nv]) - sg.MY, ny + 1 - sg.WY));
        org[threadIdx.x] = o;
    }
    return wz0;
}

// A footprint inside the window: its eight float64 adds at the byte addresses of its two z cells (+ one row, + one slab)
__device__ __forceinline__ void window_add8(unsigned char *smem, uint32_t a0, uint32_t a1, uint32_t sxB, uint32_t syB,
                                            const float (&wq)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
        lds_add(reinterpret_cast<double *>(smem + ((q & 1) ? a1 : a0) + ((q & 4) ? sxB : 0u) + ((q & 2) ? syB : 0u)), (double)wq[q]);
}

// A footprint beyond the window: the reference's clamped global atomics (include/interp.h:330-401, :431-453) at the
// byte offsets of its clamped slabs, rows and z cells
__device__ __forceinline__ void global_add8(BufRsrc rdI, uint32_t X0, uint32_t X1, uint32_t Y0, uint32_t Y1, uint32_t Z0,
                                            uint32_t Z1, const float (&wq)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
        (void)__builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(wq[q], rdI, ((q & 4) ? X1 : X0) + ((q & 2) ? Y1 : Y0) + ((q & 1) ? Z1 : Z0), 0, 0);
}

// Flush of the sheared window's touched cells: one wave per window row (lx, ly), lanes along z; the (x, y) a cell
// belongs to is its segment's origin + (lx, ly), folded onto the grid (the clamp of the reference).  REZERO leaves the
// window zeroed for the next channel.
template <int NT, bool REZERO>
__device__ __forceinline__ void shear_flush(double *win, const int2 *org, const ShearGeom &sg, BufRsrc rdI, int wez, int wz0,
                                            uint32_t gxB, uint32_t gyB) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t nrows = (uint32_t)(sg.WX * sg.WY);
    for (uint32_t row = wave; row < nrows; row += NT / 64) {
        const uint32_t lx = sg.d_wy.div(row), ly = row - lx * (uint32_t)sg.WY;
        double *wrow = win + row * (uint32_t)sg.WZ;
        for (int lz = lane; lz < wez; lz += 64) {
            const double acc = wrow[lz];
            if (acc != 0.0) {
                if (REZERO) wrow[lz] = 0.0;
                const int2 o = org[lz >> 4];
                const uint32_t off = __umul24((uint32_t)clamp1(o.x + (int)lx, sg.nx), gxB) +
                                     __umul24((uint32_t)clamp1(o.y + (int)ly, sg.ny), gyB) + (uint32_t)(wz0 + lz) * 4u;
                (void)__builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32((float)acc, rdI, off, 0, 0);
            }
        }
    }
}

}  // namespace lago
