// Host check of the dispatch helpers of lagomorph_amd/csrc/launch.hpp (tests/test_launch_dispatch_host.py).
// Plain C++17, no HIP: the helpers turn runtime flags / integers into compile-time constants for a generic lambda; a
// swapped pair would select the wrong kernel instantiation without any diagnostic, so every combination is walked and
// the constants received are compared with the values passed, position by position.
#include <cstdio>
#include <vector>

#include "../../lagomorph_amd/csrc/launch.hpp"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        ++g_checks;                                                  \
        if (!(cond)) {                                               \
            ++g_fail;                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
        }                                                            \
    } while (0)

// with_flags with N flags, for every one of the 2^N runtime combinations; `wrap` runs the dispatch inside an outer one
template <typename Wrap>
static void walk_flags(Wrap wrap) {
    using lago::with_flags;
    for (int m = 0; m < 16; ++m) {
        const bool a = m & 1, b = m & 2, c = m & 4, d = m & 8;
        wrap([&](int outer) {
            int calls = 0;
            std::vector<bool> got;
            with_flags([&](auto A) { ++calls; got = {A()}; }, a);
            CHECK(calls == 1 && got == std::vector<bool>({a}));
            calls = 0;
            with_flags([&](auto A, auto B) { ++calls; got = {A(), B()}; }, a, b);
            CHECK(calls == 1 && got == std::vector<bool>({a, b}));
            calls = 0;
            with_flags([&](auto A, auto B, auto C) { ++calls; got = {A(), B(), C()}; }, a, b, c);
            CHECK(calls == 1 && got == std::vector<bool>({a, b, c}));
            calls = 0;
            with_flags([&](auto A, auto B, auto C, auto D) {
                ++calls;
                // the values are usable as template arguments
                got = {std::bool_constant<A()>::value, std::bool_constant<B()>::value, std::bool_constant<C()>::value,
                       std::bool_constant<D()>::value};
            }, a, b, c, d);
            CHECK(calls == 1 && got == std::vector<bool>({a, b, c, d}));
            // the result of f is passed on
            CHECK(with_flags([&](auto A, auto B) { return (A() ? 2 : 0) + (B() ? 1 : 0) + 10 * outer; }, a, b) ==
                  (a ? 2 : 0) + (b ? 1 : 0) + 10 * outer);
        });
    }
}

int main() {
    using lago::with_dim;
    using lago::with_int;
    walk_flags([](auto body) { body(0); });
    // nested inside with_dim
    for (int dim = 2; dim <= 3; ++dim) {
        int outer_calls = 0;
        walk_flags([&](auto body) {
            int calls = 0;
            with_dim(dim, [&](auto DIM) {
                ++calls;
                ++outer_calls;
                CHECK((std::integral_constant<int, DIM()>::value) == dim);
                body(DIM());
            });
            CHECK(calls == 1);
        });
        CHECK(outer_calls == 16);
    }
    // nested inside with_int, for every value of its list and for values outside it
    for (int nt : {256, 512, 1024}) {
        walk_flags([&](auto body) {
            int calls = 0;
            const bool hit = with_int<256, 512, 1024>(nt, [&](auto NT) {
                ++calls;
                CHECK((std::integral_constant<int, NT()>::value) == nt);
                body(NT());
            });
            CHECK(hit && calls == 1);
        });
    }
    for (int v : {0, 1, 255, 257, 511, 768, 1023, 1025, 2048, -256}) {
        int calls = 0;
        CHECK((!with_int<256, 512, 1024>(v, [&](auto) { ++calls; })));
        CHECK(calls == 0);
    }
    for (int k = -1; k <= 6; ++k) {   // the 1..4 lists of lincomb and the Ad_star row tile
        int calls = 0, got = -100;
        const bool hit = with_int<1, 2, 3, 4>(k, [&](auto K) { ++calls; got = K(); });
        CHECK(hit == (k >= 1 && k <= 4));
        CHECK(calls == (hit ? 1 : 0) && (!hit || got == k));
    }
    {   // a value that is listed twice still gives one call
        int calls = 0;
        CHECK((with_int<4, 4>(4, [&](auto) { ++calls; })));
        CHECK(calls == 1);
    }
    printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
