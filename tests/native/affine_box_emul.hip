// Host walk of the box splat's candidate / ownership logic (lagomorph_amd/csrc/affine_box.hpp, the functions
// affine_splat_box_kernel itself calls): for a matrix, a translation and a grid, every source voxel is given its
// position and its owner box by the header's own code, and the owner's candidate range must contain it -- a source
// outside is one the kernel would drop from d_I.  Built and run by tests/test_affine_box_cover.py; needs no GPU.
//
//   affine_box_emul CASES      CASES: one case per line,  name f32|f64 nx ny nz  a0 .. a8  t0 t1 t2
//
// One line per case on stdout:
//   name regular sources uncovered misowned needed shipped i j k
// regular: affine_item_regular's decision (0: nothing else is computed, the general kernel has the item);
// uncovered: sources outside their owner's candidate range; misowned: sources whose owner box (found by division)
// does not answer affine_box_owns with yes -- the partition is broken if there is one; needed: the largest distance,
// in source voxels on one axis, by which a source lies outside its owner's preimage box BEFORE slack and floor / ceil
// (<= 0: no source needed any slack); shipped: affine_box_slack for the grid; i j k: the source that needed most.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../lagomorph_amd/csrc/affine_box.hpp"

using namespace lago;

struct Case {
    std::string name;
    bool f64;
    int n[3];
    double A[9], T[3];
};

struct BoxRange {
    int s0[3], s1[3];
    double mn[3], mx[3];
};

template <typename R>
static std::string run_case(const Case &c) {
    R An[9], Tn[3];
    for (int q = 0; q < 9; ++q) An[q] = (R)c.A[q];
    for (int q = 0; q < 3; ++q) Tn[q] = (R)c.T[q];
    const int nx = c.n[0], ny = c.n[1], nz = c.n[2];
    char buf[512];
    double Ai[9];
    if (!affine_item_regular<R>(An, Ai)) {
        snprintf(buf, sizeof buf, "%s 0 0 0 0 0 0 0 0 0", c.name.c_str());
        return buf;
    }
    // the box grid of affine_splat_boxes (affine.hip)
    const int B[3] = {nx < 8 ? nx : 8, ny < 8 ? ny : 8, nz < 48 ? nz : 48};
    const int nb[3] = {(nx + B[0] - 1) / B[0], (ny + B[1] - 1) / B[1], (nz + B[2] - 1) / B[2]};
    const int ext[3] = {nx, ny, nz};
    const R ox = half_extent<R>(nx), oy = half_extent<R>(ny), oz = half_extent<R>(nz);
    const double od[3] = {(double)ox, (double)oy, (double)oz};
    const double Td[3] = {(double)Tn[0], (double)Tn[1], (double)Tn[2]};
    const double slack = affine_box_slack(nx, ny, nz);
    std::vector<BoxRange> boxes((size_t)nb[0] * nb[1] * nb[2]);
    for (int bx = 0; bx < nb[0]; ++bx)
        for (int by = 0; by < nb[1]; ++by)
            for (int bz = 0; bz < nb[2]; ++bz) {
                BoxRange &r = boxes[((size_t)bx * nb[1] + by) * nb[2] + bz];
                const int org[3] = {bx * B[0], by * B[1], bz * B[2]};
                const int len[3] = {std::min(B[0], nx - org[0]), std::min(B[1], ny - org[1]), std::min(B[2], nz - org[2])};
                double lo[3], hi[3];
                affine_box_interval<R>(An, Td, od, ext, org, len, lo, hi);
                affine_box_preimage(Ai, Td, od, lo, hi, r.mn, r.mx);
                affine_box_candidates(r.mn, r.mx, slack, ext, r.s0, r.s1);
            }
    long long sources = 0, uncovered = 0, misowned = 0;
    double needed = -1e300;
    int worst[3] = {0, 0, 0};
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            for (int k = 0; k < nz; ++k) {
                const R fi = (R)i - ox, fj = (R)j - oy, fk = (R)k - oz;
                R hx, hy, hz;
                affine_box_position<R>(An, Tn, fi, fj, fk, ox, oy, oz, hx, hy, hz);
                const int own[3] = {clamp1(lg_floor(hx), nx) / B[0], clamp1(lg_floor(hy), ny) / B[1], clamp1(lg_floor(hz), nz) / B[2]};
                const BoxRange &r = boxes[((size_t)own[0] * nb[1] + own[1]) * nb[2] + own[2]];
                const int org[3] = {own[0] * B[0], own[1] * B[1], own[2] * B[2]};
                int fx, fy, fz;
                uint32_t lx, ly, lz;
                if (!affine_box_owns<R>(hx, hy, hz, nx, ny, nz, org[0], org[1], org[2], std::min(B[0], nx - org[0]),
                                        std::min(B[1], ny - org[1]), std::min(B[2], nz - org[2]), fx, fy, fz, lx, ly, lz))
                    ++misowned;
                const int s[3] = {i, j, k};
                bool in = true;
                for (int d = 0; d < 3; ++d) {
                    in = in && s[d] >= r.s0[d] && s[d] <= r.s1[d];
                    const double out = std::max(r.mn[d] - (double)s[d], (double)s[d] - r.mx[d]);
                    if (out > needed) {
                        needed = out;
                        worst[0] = i; worst[1] = j; worst[2] = k;
                    }
                }
                ++sources;
                if (!in) ++uncovered;
            }
    snprintf(buf, sizeof buf, "%s 1 %lld %lld %lld %.6e %.6e %d %d %d", c.name.c_str(), sources, uncovered, misowned, needed,
             slack, worst[0], worst[1], worst[2]);
    return buf;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    std::vector<Case> cases;
    char name[256], ty[16];
    for (;;) {
        Case c;
        if (fscanf(f, "%255s %15s %d %d %d", name, ty, &c.n[0], &c.n[1], &c.n[2]) != 5) break;
        char tok[64];
        for (int q = 0; q < 12; ++q) {
            if (fscanf(f, "%63s", tok) != 1) {
                fprintf(stderr, "case %s: short line\n", name);
                return 2;
            }
            (q < 9 ? c.A[q] : c.T[q - 9]) = strtod(tok, nullptr);   // (nan, inf, hex floats included)
        }
        c.name = name;
        c.f64 = !strcmp(ty, "f64");
        if (c.n[0] < 1 || c.n[1] < 1 || c.n[2] < 1 || (long long)c.n[0] * c.n[1] * c.n[2] > (1ll << 28)) {
            fprintf(stderr, "case %s: bad extents\n", name);
            return 2;
        }
        cases.push_back(c);
    }
    fclose(f);
    std::vector<std::string> out(cases.size());
    std::atomic<size_t> next{0};
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 8 ? 8 : nt);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&] {
            for (size_t q; (q = next.fetch_add(1)) < cases.size();)
                out[q] = cases[q].f64 ? run_case<double>(cases[q]) : run_case<float>(cases[q]);
        });
    for (auto &t : pool) t.join();
    for (auto &s : out) puts(s.c_str());
    return 0;
}
