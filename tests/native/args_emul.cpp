// Host check of lagomorph_amd/csrc/args.hpp (tests/test_args_host.py): the checked volume, the old make_geom extent
// rules and the disjointness rule against references that cannot overflow (unsigned __int128, sets of byte addresses).
// Plain C++17, no HIP: fail_invalid is stubbed and records the message.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../../lagomorph_amd/csrc/args.hpp"

static char g_msg[512];
static int g_fail_calls = 0;
int lago::fail_invalid(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    ++g_fail_calls;
    return LAGO_ERR_INVALID;
}

static long long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        ++g_checks;                                        \
        if (!(cond)) {                                     \
            if (++g_failed <= 20) {                        \
                fprintf(stderr, "FAILED %s: ", #cond);     \
                fprintf(stderr, __VA_ARGS__);              \
                fprintf(stderr, "\n");                     \
            }                                              \
        }                                                  \
    } while (0)

typedef unsigned __int128 u128;
using namespace lago;

enum Verdict { V_OK, V_DIM, V_NEGATIVE, V_EXTENT, V_PLANE };
static const char *const kWord[] = {"", "dimensional", "negative", "an extent of 2^31 or more", nullptr /* the limit's text */};

static const int64_t kExt[] = {-1, 0, 1, 2, 3, 1023, 1024, 23170, 23171, 1ll << 16, (1ll << 29) - 1, 1ll << 29, (1ll << 31) - 1, 1ll << 31,
                               (1ll << 32) - 1, 1ll << 32, (1ll << 32) + 1, 1ll << 40, 1ll << 62, INT64_MAX};
static const int kNumExt = sizeof(kExt) / sizeof(kExt[0]);

static void test_volume() {
    const PlaneLimit limits[] = {kPlane29, plane_bytes32(4), plane_bytes32(8), kPlane30};
    const int64_t limit_nvox[] = {(1ll << 29) - 1, (1ll << 30) - 1, (1ll << 29) - 1, 1ll << 30};   // < 2^29 elements, < 2^32 bytes, <= 2^30 voxels
    const int dims[] = {-3, 0, 1, 2, 3, 4};
    for (int li = 0; li < 4; ++li) {
        CHECK(limits[li].max_nvox == limit_nvox[li], "limit %d", li);
        for (const int dim : dims)
            for (int a = 0; a < kNumExt; ++a)
                for (int b = 0; b < kNumExt; ++b)
                    for (int c = 0; c < kNumExt; ++c) {
                        const int64_t nx = kExt[a], ny = kExt[b], nz = kExt[c];
                        // the reference
                        Verdict want = V_OK;
                        int64_t x = nx, y = ny, z = nz;
                        u128 nv = 0;
                        if (dim != 2 && dim != 3) want = V_DIM;
                        else {
                            if (dim == 2) z = ny, y = nx, x = 1;
                            if (x < 0 || y < 0 || z < 0) want = V_NEGATIVE;
                            else if (x > INT_MAX || y > INT_MAX || z > INT_MAX) want = V_EXTENT;
                            else if ((nv = (u128)x * (u128)y * (u128)z) > (u128)limit_nvox[li]) want = V_PLANE;   // < 2^93
                        }
                        Volume v = {-7, -7, -7, -7};
                        g_msg[0] = 0;
                        const int calls = g_fail_calls;
                        const int rc = check_volume(v, "t", dim, nx, ny, nz, limits[li], {1, 0});
                        if (want == V_OK) {
                            CHECK(rc == LAGO_OK && g_fail_calls == calls, "dim %d (%lld, %lld, %lld) limit %d: rejected: %s", dim,
                                  (long long)nx, (long long)ny, (long long)nz, li, g_msg);
                            CHECK(v.nx == x && v.ny == y && v.nz == z && (u128)v.nvox == nv, "dim %d (%lld, %lld, %lld): volume", dim,
                                  (long long)nx, (long long)ny, (long long)nz);
                        } else {
                            const char *word = want == V_PLANE ? limits[li].text : kWord[want];
                            CHECK(rc == LAGO_ERR_INVALID && g_fail_calls == calls + 1 && strstr(g_msg, word),
                                  "dim %d (%lld, %lld, %lld) limit %d: want '%s', got %d '%s'", dim, (long long)nx, (long long)ny,
                                  (long long)nz, li, word, rc, g_msg);
                            CHECK(v.nvox == -7, "a rejected call must leave the volume alone");
                        }
                    }
    }
    // the further counts: only their sign matters
    Volume v;
    CHECK(check_volume(v, "t", 3, 4, 4, 4, kPlane29, {0, 0, 0}) == LAGO_OK, "zero counts");
    CHECK(check_volume(v, "t", 3, 4, 4, 4, kPlane29, {INT64_MAX}) == LAGO_OK, "a count takes part in nothing but the sign check");
    CHECK(check_volume(v, "t", 3, 4, 4, 4, kPlane29, {5, -1}) == LAGO_ERR_INVALID && strstr(g_msg, "negative"), "negative count");
    CHECK(check_volume(v, "t", 2, 4, 4, -9, kPlane29, {-1, 0}) == LAGO_ERR_INVALID && strstr(g_msg, "negative"), "negative count, 2D");
    CHECK(check_volume(v, "t", 5, 4, 4, 4, kPlane29, {-1}) == LAGO_ERR_INVALID && strstr(g_msg, "dimensional"), "dim wins over a count");
    CHECK(check_volume(v, "t", 2, 4, 5, -9, kPlane29) == LAGO_OK && v.nx == 1 && v.ny == 4 && v.nz == 5 && v.nvox == 20, "2D ignores nz");
    // the triples whose int64_t product wraps to a small value
    CHECK(check_volume(v, "t", 3, (1ll << 32) + 1, (1ll << 32) - 1, 1, kPlane29) == LAGO_ERR_INVALID, "wrapping triple");
    CHECK(check_volume(v, "t", 3, 1ll << 32, 1ll << 32, 1, kPlane30) == LAGO_ERR_INVALID, "wrapping triple");
}

// make_geom(g, dim, nn, nx, ny, nz): valid iff nn >= 0, every extent >= 1 after the 2D remap, product < 2^29
static void test_geom_volume() {
    const int64_t nns[] = {-1, 0, 1, 7};
    for (const int dim : {2, 3})
        for (const int64_t nn : nns)
            for (int a = 0; a < kNumExt; ++a)
                for (int b = 0; b < kNumExt; ++b)
                    for (int c = 0; c < kNumExt; ++c) {
                        int64_t x = kExt[a], y = kExt[b], z = kExt[c];
                        if (dim == 2) z = y, y = x, x = 1;
                        bool want = nn >= 0 && x >= 1 && y >= 1 && z >= 1 && x < (1ll << 29) && y < (1ll << 29) && z < (1ll << 29);
                        const u128 nv = want ? (u128)x * (u128)y * (u128)z : 0;   // < 2^87
                        want = want && nv < ((u128)1 << 29);
                        Volume v = {-7, -7, -7, -7};
                        const bool got = geom_volume(v, dim, nn, kExt[a], kExt[b], kExt[c]);
                        CHECK(got == want, "geom_volume dim %d nn %lld (%lld, %lld, %lld): %d", dim, (long long)nn, (long long)kExt[a],
                              (long long)kExt[b], (long long)kExt[c], (int)got);
                        if (got && want) CHECK(v.nx == x && v.ny == y && v.nz == z && (u128)v.nvox == nv, "geom_volume: volume");
                    }
    Volume v;
    // products that wrap in int64_t (2^64 - 1 -> -1, 2^64 -> 0, 2^63 -> negative, 2^66 -> 0): accepted before, now rejected
    CHECK(!geom_volume(v, 3, 1, (1ll << 32) + 1, (1ll << 32) - 1, 1), "wrapping triple");
    CHECK(!geom_volume(v, 3, 1, 1ll << 32, 1ll << 32, 1), "wrapping triple");
    CHECK(!geom_volume(v, 3, 1, 1ll << 62, 2, 1), "wrapping triple");
    CHECK(!geom_volume(v, 3, 1, 1ll << 62, 4, 4), "wrapping triple");
    CHECK(!geom_volume(v, 2, 1, 1ll << 40, 1ll << 24, 1), "wrapping pair, 2D");
    // as before: 2^28 voxels pass, exactly 2^29 do not, 2^29 - 2^19 do
    CHECK(geom_volume(v, 3, 1, 1, 1 << 14, 1 << 14) && v.nvox == (1ll << 28), "(1, 2^14, 2^14)");
    CHECK(!geom_volume(v, 3, 1, 1, 1 << 15, 1 << 14), "(1, 2^15, 2^14): 2^29 voxels");
    CHECK(!geom_volume(v, 3, 1, 1 << 9, 1 << 10, 1 << 10), "(2^9, 2^10, 2^10): 2^29 voxels");
    CHECK(geom_volume(v, 3, 1, 1 << 9, 1 << 10, (1 << 10) - 1) && v.nvox == (1ll << 29) - (1ll << 19), "(2^9, 2^10, 2^10 - 1)");
    int64_t nv;
    CHECK(volume_product(INT64_MAX, 1, 1, nv) && nv == INT64_MAX, "volume_product: the largest value");
    CHECK(!volume_product(INT64_MAX, 2, 1, nv) && !volume_product(1ll << 21, 1ll << 21, 1ll << 21, nv), "volume_product: 2^63 and more");
    CHECK(volume_product(INT64_MAX, INT64_MAX, 0, nv) && nv == 0, "volume_product: an empty volume");
}

// two outputs and two inputs over addresses 0..12 (0: null) and sizes 0..4, against the sets of bytes they cover
static void test_any_overlap() {
    const auto bytes_of = [](unsigned p, unsigned n) { return p == 0 || n == 0 ? 0u : ((1u << n) - 1u) << p; };
    const auto span = [](unsigned p, unsigned n) { return Span{(const void *)(uintptr_t)p, (size_t)n}; };
    long long rejected = 0;
    for (unsigned p0 = 0; p0 <= 12; ++p0) for (unsigned n0 = 0; n0 <= 4; ++n0)
    for (unsigned p1 = 0; p1 <= 12; ++p1) for (unsigned n1 = 0; n1 <= 4; ++n1) {
        const unsigned o0 = bytes_of(p0, n0), o1 = bytes_of(p1, n1);
        for (unsigned p2 = 0; p2 <= 12; ++p2) for (unsigned n2 = 0; n2 <= 4; ++n2)
        for (unsigned p3 = 0; p3 <= 12; ++p3) for (unsigned n3 = 0; n3 <= 4; ++n3) {
            const unsigned i0 = bytes_of(p2, n2), i1 = bytes_of(p3, n3);
            const bool want = ((o0 | o1) & (i0 | i1)) != 0 || (o0 & o1) != 0;
            const bool got = any_overlap({span(p0, n0), span(p1, n1)}, {span(p2, n2), span(p3, n3)});
            rejected += got;
            CHECK(got == want, "outs (%u+%u) (%u+%u) ins (%u+%u) (%u+%u): %d", p0, n0, p1, n1, p2, n2, p3, n3, (int)got);
        }
    }
    CHECK(rejected > 0, "no combination overlapped");
    // a null or empty span never causes a rejection, wherever it points and whatever its size
    const Span full = {(const void *)(uintptr_t)16, 1u << 20};
    for (const Span &quiet : {Span{nullptr, 1u << 20}, Span{(const void *)(uintptr_t)64, 0}, Span{nullptr, 0}}) {
        CHECK(!any_overlap({quiet}, {full}) && !any_overlap({full}, {quiet}) && !any_overlap({full, quiet}, {}) &&
                  !any_overlap({quiet, quiet}, {quiet}), "a span that takes no part");
    }
    CHECK(any_overlap({full, full}, {}) && any_overlap({full}, {full}) && !any_overlap({}, {full, full}), "inputs may overlap each other");
}

// the forward gather's pointers: out against the field (one item when broadcast) and the positions
static void test_check_gather() {
    const char *base = (const char *)(uintptr_t)0x100000;
    const GatherBytes b(4, 8, 3, 2, 5, 7, 11, 0), bc(4, 8, 3, 2, 5, 7, 11, 1);
    CHECK(b.out == 2 * 5 * 7 * 4 && b.field == 2 * 5 * 11 * 4 && b.pos == 2 * 3 * 7 * 8 && bc.field == 5 * 11 * 4 && bc.out == b.out, "GatherBytes");
    CHECK(check_gather("t", base, base + b.out, base + b.out + b.field, b) == kLaunchNow, "adjacent ranges");
    CHECK(check_gather("t", base + 1, base + b.out, base - b.pos, b) == LAGO_ERR_INVALID && strstr(g_msg, "overlap"), "out into the field");
    CHECK(check_gather("t", base + b.pos - 1, base + (1 << 20), base, b) == LAGO_ERR_INVALID && strstr(g_msg, "overlap"), "positions into out");
    CHECK(check_gather("t", base, base - bc.field, base + b.out, bc) == kLaunchNow, "a broadcast field is one item long");
    CHECK(check_gather("t", base, base - bc.field, base + b.out, b) == LAGO_ERR_INVALID, "... a field per item is not");
    for (int q = 0; q < 3; ++q)
        CHECK(check_gather("t", q == 0 ? nullptr : base, q == 1 ? nullptr : base + (1 << 20), q == 2 ? nullptr : base + (2 << 20), b) ==
                      LAGO_ERR_INVALID && strstr(g_msg, "null"), "null pointer %d", q);
}

int main() {
    test_volume();
    test_geom_volume();
    test_any_overlap();
    test_check_gather();
    printf("%lld checks, %lld failed\n", g_checks, g_failed);
    return g_failed != 0;
}
