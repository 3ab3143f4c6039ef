// A voxel tile of one channel plane in LDS with a halo of up to two voxels, every coordinate clamped to its axis: the
// wider sibling of stencil_tile.hpp's RowTile (one voxel, clamped rows), for the stencils of energy.hip.  Device only.
//
// The tile holds TX x TY x TZ voxels from origin o[], LO cells before and HI cells after them on every axis that the
// field has (dim 2: no x axis, TX = 1).  Cell (px, py, pz) holds u at the coordinates o - LO + p, each clamped to
// [0, n - 1]: every load is inside the plane for any extent >= 1 and any origin inside it, partial tiles included, and
// a stencil finds the replicated border value wherever its neighbour does not exist.  z is the contiguous axis: lanes
// read and write consecutive cells, a row of LD = TZ + LO + HI cells.
#pragma once

#include "common.hpp"

namespace lago {

template <typename R, int DIM, int TX_, int TY_, int TZ_, int LO_, int HI_>
struct HaloTile {
    static constexpr int TX = TX_, TY = TY_, TZ = TZ_, LO = LO_, HI = HI_;
    static constexpr int LOX = DIM == 3 ? LO : 0;
    static constexpr int PX = TX + (DIM == 3 ? LO + HI : 0), PY = TY + LO + HI, LD = TZ + LO + HI;
    static constexpr int CELLS = PX * PY * LD;
    static_assert(DIM == 3 || TX == 1, "a 2D tile has no x axis");
    static_assert(TZ == 64, "a row of the tile is a wave of lanes");

    // all `nthreads` threads of the workgroup (whole waves); the caller synchronises before the first read.  A wave
    // takes whole rows: the row's coordinates and base address are wave-uniform (scalar registers), lane l loads cell l
    // of the row at its own clamped z, computed once; the LD - 64 cells a row has beyond a wave's width follow in a
    // second loop over all rows, lanes along (row, cell).
    static __device__ __forceinline__ void stage(R *__restrict__ tile, const R *__restrict__ plane, const int (&o)[3], const int (&n)[3],
                                                 uint32_t tid, uint32_t nthreads) {
        static_assert(LD >= 64 && LD - 64 <= 4 && ((LD - 64) & (LD - 65)) == 0, "a wave's width and a power-of-two remainder");
        constexpr uint32_t ROWS = PX * PY, REM = LD - 64;
        const uint32_t lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nthreads >> 6;
        const uint32_t zc = (uint32_t)lg_med3(o[2] - LO + (int)lane, 0, n[2] - 1);
        for (uint32_t row = wave; row < ROWS; row += nwaves) {
            const uint32_t px = row / (uint32_t)PY, py = row - px * (uint32_t)PY;
            const int gx = max(0, min(o[0] - LOX + (int)px, n[0] - 1)), gy = max(0, min(o[1] - LO + (int)py, n[1] - 1));   // (scalar)
            tile[row * (uint32_t)LD + lane] = plane[((uint32_t)gx * (uint32_t)n[1] + (uint32_t)gy) * (uint32_t)n[2] + zc];
        }
        if constexpr (REM > 0) {
            for (uint32_t e = tid; e < ROWS * REM; e += nthreads) {
                const uint32_t row = e / REM, pz = 64u + e % REM;
                const uint32_t px = row / (uint32_t)PY, py = row - px * (uint32_t)PY;
                const int gx = lg_med3(o[0] - LOX + (int)px, 0, n[0] - 1), gy = lg_med3(o[1] - LO + (int)py, 0, n[1] - 1);
                const int gz = lg_med3(o[2] - LO + (int)pz, 0, n[2] - 1);
                tile[row * (uint32_t)LD + pz] = plane[((uint32_t)gx * (uint32_t)n[1] + (uint32_t)gy) * (uint32_t)n[2] + (uint32_t)gz];
            }
        }
    }
    // the cell of tile voxel (lx, ly, lz), 0 <= l < T; neighbours at (dx * PY + dy) * LD + dz from it
    static __device__ __forceinline__ uint32_t cell(uint32_t lx, uint32_t ly, uint32_t lz) {
        return ((lx + LOX) * PY + (ly + LO)) * LD + lz + LO;
    }
};

}  // namespace lago
