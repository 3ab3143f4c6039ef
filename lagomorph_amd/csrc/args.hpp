// The argument frame of the entry points (included from common.hpp): what a volume's extents, a call's pointers and
// its outputs' byte ranges must satisfy before the first device call, written once.  The first part needs nothing but
// the C++17 standard library, the return codes of include/lagomorph_hip.h and a declaration of fail_invalid
// (tests/native/args_emul.cpp compiles it with a plain host compiler and stubs fail_invalid).  Nothing here touches the
// launch-direction counter (common.hpp: next_direction).
#pragma once

#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <initializer_list>

#include "../../include/lagomorph_hip.h"

namespace lago {

int fail_invalid(const char *fmt, ...);

constexpr int kLaunchNow = 1;   // what a check returns, next to LAGO_OK (the call is done) and the error codes (< 0)

// a b c for factors >= 0 without forming a product that overflows: false when it does not fit int64_t
inline bool volume_product(int64_t a, int64_t b, int64_t c, int64_t &nv) {
    nv = 0;
    return a == 0 || b == 0 || c == 0 || (!__builtin_mul_overflow(a, b, &nv) && !__builtin_mul_overflow(nv, c, &nv));
}
// a 2D problem (nx, ny) = (H, W) is the volume (1, H, W): the same flattened layout (its nz is ignored)
inline void as_volume(int dim, int64_t &nx, int64_t &ny, int64_t &nz) {
    if (dim == 2) nz = ny, ny = nx, nx = 1;
}

// The most voxels one channel plane may have, and how the rejection reads.  32-bit byte offsets into a plane: of float64
// for everything that goes on to make_geom (nvox * 8 < 2^32), of `elem`-byte elements (elem divides 2^32) for the points
struct PlaneLimit { int64_t max_nvox; const char *text; };
constexpr PlaneLimit kPlane29 = {(1ll << 29) - 1, "a channel plane of 2^29 elements or more"};
constexpr PlaneLimit plane_bytes32(size_t elem) { return {(1ll << 32) / (int64_t)elem - 1, "a channel plane of 2^32 bytes or more"}; }
constexpr PlaneLimit kPlane30 = {1ll << 30, "more than 2^30 voxels in a row"};    // 32-bit voxel counts with headroom
constexpr PlaneLimit kPlaneAny = {INT64_MAX, "a volume of 2^63 voxels or more"};  // the caller bounds the extents itself

// A checked volume: the extents as laid out in memory, each in 0..INT_MAX, nvox = nx ny nz within the limit (0: empty)
struct Volume { int64_t nx, ny, nz, nvox; };

inline int check_dim(const char *what, int dim) {
    if (dim == 2 || dim == 3) return LAGO_OK;
    return fail_invalid("%s: Only two- and three-dimensional fields are supported (dim %d)", what, dim);
}
// In this order: dim, the 2D remap, a negative extent or count (`counts`: nn, nc, rows, np, ..., which take part in
// nothing else), an extent of 2^31 or more, the plane limit.  LAGO_OK or the code of fail_invalid.
inline int check_volume(Volume &v, const char *what, int dim, int64_t nx, int64_t ny, int64_t nz, PlaneLimit limit,
                        std::initializer_list<int64_t> counts = {}) {
    if (const int rc = check_dim(what, dim)) return rc;
    as_volume(dim, nx, ny, nz);
    bool negative = nx < 0 || ny < 0 || nz < 0;
    for (const int64_t c : counts) negative = negative || c < 0;
    if (negative) return fail_invalid("%s: negative extent", what);
    if (nx > INT_MAX || ny > INT_MAX || nz > INT_MAX) return fail_invalid("%s: an extent of 2^31 or more", what);
    int64_t nv;
    if (!volume_product(nx, ny, nz, nv) || nv > limit.max_nvox) return fail_invalid("%s: %s", what, limit.text);
    v = {nx, ny, nz, nv};
    return LAGO_OK;
}
// The extent rules of make_geom(g, dim, nn, nx, ny, nz) (common.hpp), which the older entry points report as one
// "bad extent": nn >= 0, every extent >= 1 after the 2D remap, fewer than 2^29 voxels
inline bool geom_volume(Volume &v, int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz) {
    as_volume(dim, nx, ny, nz);
    int64_t nv;
    if (nn < 0 || nx < 1 || ny < 1 || nz < 1 || !volume_product(nx, ny, nz, nv) || nv > kPlane29.max_nvox) return false;
    v = {nx, ny, nz, nv};
    return true;
}

inline bool overlaps(const void *a, size_t na, const void *b, size_t nb) {   // [a, a + na) and [b, b + nb) bytes
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + nb && q < p + na;
}
inline bool overlaps(const void *a, const void *b, size_t bytes) { return overlaps(a, bytes, b, bytes); }

// A byte range a call reads or writes.  One with a null pointer or no bytes (an optional argument that is absent or
// not wanted) takes no part in any_overlap: whether an output overlaps an input, or two outputs overlap each other.
struct Span { const void *p; size_t bytes; };
inline bool any_overlap(std::initializer_list<Span> outs, std::initializer_list<Span> ins) {
    const auto hit = [](const Span &a, const Span &b) { return a.p && b.p && a.bytes && b.bytes && overlaps(a.p, a.bytes, b.p, b.bytes); };
    for (const Span *o = outs.begin(); o != outs.end(); ++o) {
        for (const Span &i : ins)
            if (hit(*o, i)) return true;
        for (const Span *o2 = o + 1; o2 != outs.end(); ++o2)
            if (hit(*o, *o2)) return true;
    }
    return false;
}

// The arguments of a gather: out (nn, nc, npos) sampled from a field (nn or 1, nc, nplane) of `elem`-byte elements
// at positions (nn, dim, npos) of `pelem`-byte elements; of its adjoint, grad_out has the shape of out.
struct GatherBytes {
    size_t out, field, pos;
    GatherBytes(size_t elem, size_t pelem, int dim, int64_t nn, int64_t nc, int64_t npos, int64_t nplane, int bc)
        : out((size_t)nn * nc * npos * elem), field((size_t)(bc ? 1 : nn) * nc * nplane * elem), pos((size_t)nn * dim * npos * pelem) {}
};
inline int check_gather(const char *what, const void *out, const void *field, const void *pos, const GatherBytes &b) {
    if (!out || !field || !pos) return fail_invalid("%s: null pointer", what);
    if (any_overlap({{out, b.out}}, {{field, b.field}, {pos, b.pos}})) return fail_invalid("%s: out must not overlap an input", what);
    return kLaunchNow;
}

}  // namespace lago

#if defined(__HIPCC__)
namespace lago {

int fail_hip(hipError_t e, const char *what);

// The adjoint of a gather up to its launch: d_field (the scatter target, zeroed here on the stream) and d_pos, each
// computed when its need_* flag is set.  An empty problem zeroes the gradients that have elements: nothing adds
// anything, a d_field that has cells is all zeros, a d_pos has no element or only empty sums.
inline int check_gather_backward(const char *what, void *d_field, void *d_pos, const void *go, const void *field,
                                 const void *pos, const GatherBytes &b, bool need_f, bool need_p, bool empty, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (empty) {
        if (need_f && d_field && b.field) e = hipMemsetAsync(d_field, 0, b.field, s);
        if (e == hipSuccess && need_p && d_pos && b.pos) e = hipMemsetAsync(d_pos, 0, b.pos, s);
        return e != hipSuccess ? fail_hip(e, what) : LAGO_OK;
    }
    if (!need_f && !need_p) return LAGO_OK;
    if ((need_f && !d_field) || (need_p && (!d_pos || !field)) || !go || !pos) return fail_invalid("%s: null pointer", what);
    // (a gradient that is not wanted is ignored)
    if (any_overlap({{need_f ? d_field : nullptr, b.field}, {need_p ? d_pos : nullptr, b.pos}}, {{go, b.out}, {pos, b.pos}, {field, b.field}}))
        return fail_invalid("%s: a gradient must not overlap an input or the other gradient", what);
    if (need_f && (e = hipMemsetAsync(d_field, 0, b.field, s)) != hipSuccess) return fail_hip(e, what);
    return kLaunchNow;
}

}  // namespace lago
#endif
