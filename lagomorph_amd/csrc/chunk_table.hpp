// The chunked-table frame of the integer-table operators (mi.hip: the joint histogram; labels.hip: the overlap counts),
// written once.  Grid rows x chunks: a workgroup walks its chunk of a row as a scalar head up to the first vector
// boundary, vectors, and a scalar tail, and adds into `rep` replicas of an integer table in dynamic LDS; it sums them
// and writes its partial table with plain stores to the slab (rows, chunks, size), whose chunks table_reduce_kernel
// sums.  Every slab entry is written: no memset, no global atomic, the same bits for any chunking and replica count.
// The first part is plain C++17 (tests/native/chunk_table_emul.cpp builds it with a host compiler), the rest needs HIP.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include "common.hpp"   // (kBlock, launch and fail_* for the second part)
#endif

namespace lago {

constexpr int64_t kSlabBytes = 8ll << 20;     // the partial tables of all rows stay below this (or one table a row)
constexpr size_t kTableLdsBytes = 64 * 1024;  // what the replicas of one workgroup may take

struct RowChunks { uint32_t nvox, chunks, chunk; };   // elements of one row, workgroups per row, elements per workgroup

// How many chunks a row is worth: one per chunk_min elements, as long as the slab of all rows stays below slab_bytes
constexpr int64_t chunks_wanted(int64_t table_bytes, int64_t rows, int64_t nvox, int64_t chunk_min, int64_t slab_bytes) {
    const int64_t by_size = (nvox + chunk_min - 1) / chunk_min;
    const int64_t cap = slab_bytes / table_bytes / (rows > 1 ? rows : 1);
    const int64_t c = by_size < cap ? by_size : cap;
    return c < 1 ? 1 : c;
}
// ... and what a lago_*_scratch_* query answers (1 for arguments the entry point rejects)
inline int scratch_chunks(bool table_ok, int64_t table_bytes, int64_t rows, int64_t nvox, int64_t chunk_min) {
    if (!table_ok || rows < 0 || nvox < 0 || nvox > (1ll << 30)) return 1;
    return (int)chunks_wanted(table_bytes, rows, nvox, chunk_min, kSlabBytes);
}
// The split for at most `want` chunks of at least `least` elements: the chunk is a multiple of four and no chunk is
// empty (an empty row is one chunk of nothing)
constexpr RowChunks split_row(int64_t nvox, int64_t want, int64_t least) {
    int64_t c = (nvox + least - 1) / least;
    c = c < want ? c : want;
    c = c < 1 ? 1 : c;
    const int64_t per = ((nvox + c - 1) / c + 3) / 4 * 4;
    return {(uint32_t)nvox, per ? (uint32_t)((nvox + per - 1) / per) : 1u, (uint32_t)per};
}

// n elements as scalars [0, head), nvec vectors of VW elements from head, and scalars [tail, n).  `mis`: the
// misalignment of every pointer involved against a vector, in elements; `same` false (they differ): no vector is formed
struct WalkSplit { uint32_t head, nvec, tail; };
template <uint32_t VW>
constexpr WalkSplit walk_split(uint32_t n, bool same, uint32_t mis) {
    const uint32_t up = (VW - mis) % VW;
    const uint32_t head = same ? (up < n ? up : n) : n;
    const uint32_t nvec = (n - head) / VW;
    return {head, nvec, head + nvec * VW};
}

#if defined(__HIPCC__)
struct ChunkOfRow { uint32_t row, c0, n; };   // this workgroup's elements [c0, c0 + n) of row `row` (all uniform)
__device__ __forceinline__ ChunkOfRow chunk_of_block(const RowChunks &p) {
    const uint32_t row = blockIdx.x / p.chunks, c0 = (blockIdx.x - row * p.chunks) * p.chunk;
    return {row, c0, c0 < p.nvox ? min(p.chunk, p.nvox - c0) : 0u};
}
template <uint32_t VW, typename T>
__device__ __forceinline__ uint32_t misalign(const T *p) {   // in elements, against a vector of VW
    return (uint32_t)(((uintptr_t)p / sizeof(T)) % VW);
}

// The walk of n elements, a lane at a time: scalar(i) and vector(i) are given c0 + the index within the chunk, the
// index within the row.
template <uint32_t VW, typename FS, typename FV>
__device__ __forceinline__ void chunk_walk(uint32_t c0, uint32_t n, bool same, uint32_t mis, FS &&scalar, FV &&vector) {
    const WalkSplit w = walk_split<VW>(n, same, mis);
    for (uint32_t i = threadIdx.x; i < w.head; i += kBlock) scalar(c0 + i);
    for (uint32_t v = threadIdx.x; v < w.nvec; v += kBlock) vector(c0 + w.head + v * VW);
    for (uint32_t i = w.tail + threadIdx.x; i < n; i += kBlock) scalar(c0 + i);
}
// ... and for callbacks that ballot: all loops have uniform bounds and no lane leaves one early.  scalar(i, valid) and
// vector(first, i, valid) are given indices within the chunk (the vector's as the uniform start of the vectors and
// the lane's offset from it, to be added to the pointer in that order); without `valid` the element is not to be touched.
template <uint32_t VW, typename FS, typename FV>
__device__ __forceinline__ void chunk_walk_uniform(uint32_t n, bool same, uint32_t mis, FS &&scalar, FV &&vector) {
    const WalkSplit w = walk_split<VW>(n, same, mis);
    const auto scalars = [&](uint32_t from, uint32_t to) {
        for (uint32_t base = from; base < to; base += kBlock) scalar(base + threadIdx.x, base + threadIdx.x < to);
    };
    scalars(0, w.head);
    for (uint32_t base = 0; base < w.nvec; base += kBlock)
        vector(w.head, (base + threadIdx.x) * VW, base + threadIdx.x < w.nvec);
    scalars(w.tail, n);
}
// `rep` replicas of a table of `size` counters in LDS (I: int or uint32_t, as the caller indexes): zeroed before the walk
template <typename C, typename I>
__device__ __forceinline__ void tables_zero(C *tab, I size, int rep) {
    for (I e = threadIdx.x; e < (I)rep * size; e += kBlock) tab[e] = 0;
    __syncthreads();
}
// ... and after it summed into this workgroup's partial table of the slab
template <typename S, typename C, typename I>
__device__ __forceinline__ void tables_store(S *slab, const C *tab, I size, int rep) {
    __syncthreads();
    S *out = slab + (size_t)blockIdx.x * size;
    for (I e = threadIdx.x; e < size; e += kBlock) {
        C sum = tab[e];
        for (int r = 1; r < rep; ++r) sum += tab[(I)r * size + e];
        out[e] = (S)sum;
    }
}

// One workgroup per 64 entries of one row's table (the last group of a row is ragged where `size` is no multiple of
// 64): lane (part, e) sums the chunks part, part + 4, ... of its entry with eight loads in flight, the four parts meet
// in LDS and finish(index in (rows, size), sum) writes the result.  An integer sum: the order does not show.
template <typename S, typename F>
__global__ __launch_bounds__(kBlock) void table_reduce_kernel(const S *__restrict__ slab, uint32_t chunks, uint32_t size,
                                                              uint32_t groups, F finish) {
    __shared__ long long part[4][64];
    const uint32_t row = blockIdx.x / groups, e = (blockIdx.x - row * groups) * 64 + (threadIdx.x & 63u);   // row: uniform
    const uint32_t p = threadIdx.x >> 6;
    long long sum = 0;
    if (e < size) {
        const S *s = slab + (size_t)row * chunks * size + e;
#pragma unroll 8
        for (uint32_t c = p; c < chunks; c += 4) sum += (long long)s[(size_t)c * size];
    }
    part[p][threadIdx.x & 63u] = sum;
    __syncthreads();
    if (p == 0 && e < size) {
        const uint32_t t = threadIdx.x;
        finish((size_t)row * size + e, part[0][t] + part[1][t] + part[2][t] + part[3][t]);
    }
}

// ---- host side.  What an entry point `what` does about chunking between its own checks and the launch of its walk
// (grid rows x rc.chunks): the split for a scratch of scratch_chunks tables a row, both grids below 2^31 blocks, the
// slab's bytes for its overlap check.  kLaunchNow or the code of fail_invalid.
template <typename S>
inline int plan_tables(RowChunks &rc, size_t &slab_bytes, const char *what, uint32_t size, int64_t rows, int64_t nvox,
                       int64_t chunk_min, int64_t scratch_chunks) {
    if (scratch_chunks < 1) return fail_invalid("%s: scratch must hold at least one table per row", what);
    const int64_t want = chunks_wanted((int64_t)size * sizeof(S), rows, nvox, chunk_min, kSlabBytes);
    rc = split_row(nvox, want < scratch_chunks ? want : scratch_chunks, chunk_min);
    const uint64_t nb = (uint64_t)rows * rc.chunks, nr = (uint64_t)rows * ((size + 63) / 64);   // blocks: walk, reducer
    if (nb >= (1ull << 31) || nr >= (1ull << 31)) return fail_invalid("%s: bad extent", what);
    slab_bytes = (size_t)nb * size * sizeof(S);
    return kLaunchNow;
}
// ... and after that launch (`e`): the reducer
template <typename S, typename F>
inline int reduce_tables(const char *what, hipError_t e, hipStream_t s, const RowChunks &rc, int64_t rows, uint32_t size,
                         const S *slab, F finish) {
    if (e != hipSuccess) return fail_hip(e, what);
    const uint32_t groups = (size + 63) / 64;
    e = launch(table_reduce_kernel<S, F>, dim3((uint32_t)rows * groups), dim3(kBlock), 0, s, slab, rc.chunks, size, groups, finish);
    return launched(e, s, what);
}
#endif

}  // namespace lago
