// Host-side dispatch and launch helpers (included from common.hpp).
//
// Dispatch: a kernel family is a template over a few flags / small integers that are only known at run time.  The
// helpers below turn each runtime value into a std::integral_constant and hand it to a generic lambda, which names the
// kernel's template arguments in the kernel's own order:
//
//     with_flags([&](auto NEED_U, auto UNIT, auto BC) { ... kernel<NT, NEED_U(), UNIT(), BC()> ... }, need_u, unit, bc);
//
// An arm that must not be instantiated is guarded with `if constexpr` inside the lambda.  This part needs nothing but
// the C++17 standard library (tests/native/launch_dispatch_emul.cpp compiles it with a plain host compiler).
#pragma once

#include <type_traits>
#include <utility>

namespace lago {

// f(std::bool_constant<flag>...), one per runtime flag, in the order given
template <typename F>
inline decltype(auto) with_flags(F &&f) { return f(); }
template <typename F, typename... Rest>
inline decltype(auto) with_flags(F &&f, bool first, Rest... rest) {
    auto bind = [&](auto FIRST) -> decltype(auto) {
        return with_flags([&](auto... REST) -> decltype(auto) { return f(FIRST, REST...); }, rest...);
    };
    return first ? bind(std::true_type{}) : bind(std::false_type{});
}

// f(std::integral_constant<int, V>) for the V of the list that equals v; false (f not called) when none does
template <int... Vs, typename F>
inline bool with_int(int v, F &&f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// f(std::integral_constant<int, 3>) for dim == 3, <int, 2> otherwise (the entry points have rejected every other dim)
template <typename F>
inline decltype(auto) with_dim(int dim, F &&f) {
    return dim == 3 ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 2>{});
}

}  // namespace lago

#if defined(__HIPCC__)
namespace lago {

// What a `*_launch` helper of one kernel family returns (next to LAGO_OK and the error codes, which are <= 0) when the
// shape is not its own: the entry point then goes on to the next kernel of its ladder.
constexpr int kNotTaken = 1;

// Launch with `smem` bytes of dynamic LDS.  More than 64 KB has to be allowed per kernel first; a failure to do so is
// returned (the caller reports it: fail_hip(e, "<entry point>")).  A failure of the launch itself is left to
// finish_launch, as for every other launch.
template <typename... P, typename... A>
inline hipError_t launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t smem, hipStream_t stream, A &&...args) {
    if (smem > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, grid, block, smem, stream, std::forward<A>(args)...);
    return hipSuccess;
}

// How an entry point ends after its last launch(): the failure launch() returned, else what finish_launch finds.
inline int launched(hipError_t e, hipStream_t s, const char *what) { return e != hipSuccess ? fail_hip(e, what) : finish_launch(s, what); }

// Grid of the slab-unrolled 3D gather kernels (U voxels per lane, kBlock lanes): false when the volume is too flat or
// too small for them, or the grid too large; otherwise nbx_u blocks per batch item, nb in all.
inline bool slab_grid(const Geom &g, int64_t nn, int U, uint32_t &nbx_u, uint32_t &nb) {
    if (!(g.nz >= 2 && kBlock / g.nz + 1 < g.ny && g.nvox >= 4u * U * kBlock)) return false;
    nbx_u = (g.nvox + U * kBlock - 1) / (U * kBlock);
    const uint64_t n = (uint64_t)nbx_u * (uint64_t)nn;
    if (n >= (1ull << 31)) return false;
    nb = (uint32_t)n;
    return true;
}

}  // namespace lago
#endif
