// Host emulation of warp_labels: every voxel of every case of a file through the functions of
// lagomorph_amd/csrc/label_vote.hpp (the header labels.hip's kernels call), built by a plain host compiler with
// -ffp-contract=off as the library is.  tests/test_labels_host.py compares the output with tests/labels_ref.py exactly,
// and runs a second build of this program with -fsanitize=address,undefined.
//
//   label_emul <in> <out>
//   in : cases until the end of the file, each
//        int32 dim (2 | 3), prec (4 | 8), N, NL (1: one label map for every item | N), n[3] (n[2] unused in 2D), double dt,
//        int32 L[NL * nvox], R u[N * dim * nvox]
//   out: per case  int32 nearest[N * nvox], int32 vote[N * nvox], int32 lo[N * nvox * dim], int32 hi[N * nvox * dim],
//        double t[N * nvox * dim]   (the axes of a voxel together)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../lagomorph_amd/csrc/label_vote.hpp"

template <typename T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <typename T>
static bool wr(FILE *f, const T *p, size_t n) { return fwrite(p, sizeof(T), n, f) == n; }

template <typename R>
static int run(FILE *in, FILE *out, int dim, int N, int NL, const int32_t (&n)[3], double dt) {
    const size_t nvox = (size_t)n[0] * n[1] * (dim == 3 ? n[2] : 1);
    std::vector<int32_t> L((size_t)NL * nvox);
    std::vector<R> u((size_t)N * dim * nvox);
    if (!rd(in, L.data(), L.size()) || !rd(in, u.data(), u.size())) return 4;
    std::vector<int32_t> nearest((size_t)N * nvox), vote((size_t)N * nvox), lo((size_t)N * nvox * dim), hi(lo.size());
    std::vector<double> t(lo.size());
    for (int b = 0; b < N; ++b) {
        const int32_t *Lb = L.data() + (NL == 1 ? 0 : (size_t)b * nvox);
        for (size_t s = 0; s < nvox; ++s) {
            int idx[3];
            size_t r = s;
            for (int a = dim - 1; a >= 0; --a) {
                idx[a] = (int)(r % (size_t)n[a]);
                r /= (size_t)n[a];
            }
            lago::LvAxis ax[3];
            for (int a = 0; a < dim; ++a) {
                ax[a] = lago::lv_axis<R>(lago::lv_sample_pos<R>(idx[a], dt, u[((size_t)b * dim + a) * nvox + s]), n[a]);
                if (ax[a].lo < 0 || ax[a].lo >= n[a] || ax[a].hi < 0 || ax[a].hi >= n[a]) return 5;   // (L is indexed with them)
                const size_t e = ((size_t)b * nvox + s) * dim + a;
                lo[e] = ax[a].lo;
                hi[e] = ax[a].hi;
                t[e] = ax[a].t;
            }
            const auto at = [&](int x, int y, int z) { return Lb[dim == 3 ? ((size_t)x * n[1] + y) * n[2] + z : (size_t)x * n[1] + y]; };
            const size_t o = (size_t)b * nvox + s;
            if (dim == 3) {
                int32_t c[8];
                double w[8];
                for (int q = 0; q < 8; ++q)
                    c[q] = at((q & 4) ? ax[0].hi : ax[0].lo, (q & 2) ? ax[1].hi : ax[1].lo, (q & 1) ? ax[2].hi : ax[2].lo);
                lago::lv_weights(ax[0].t, ax[1].t, ax[2].t, w);
                vote[o] = lago::lv_vote<8>(c, w);
                nearest[o] = at(ax[0].nearest(), ax[1].nearest(), ax[2].nearest());
            } else {
                int32_t c[4];
                double w[4];
                for (int q = 0; q < 4; ++q) c[q] = at((q & 2) ? ax[0].hi : ax[0].lo, (q & 1) ? ax[1].hi : ax[1].lo, 0);
                lago::lv_weights(ax[0].t, ax[1].t, w);
                vote[o] = lago::lv_vote<4>(c, w);
                nearest[o] = at(ax[0].nearest(), ax[1].nearest(), 0);
            }
        }
    }
    return wr(out, nearest.data(), nearest.size()) && wr(out, vote.data(), vote.size()) && wr(out, lo.data(), lo.size()) &&
                   wr(out, hi.data(), hi.size()) && wr(out, t.data(), t.size())
               ? 0
               : 6;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    int32_t h[7];
    int rc = 0;
    while (rc == 0 && rd(in, h, 7)) {
        double dt;
        const int32_t n[3] = {h[4], h[5], h[6]};
        if (!rd(in, &dt, 1) || (h[0] != 2 && h[0] != 3) || (h[1] != 4 && h[1] != 8) || h[2] < 1 || (h[3] != 1 && h[3] != h[2]) ||
            n[0] < 1 || n[1] < 1 || (h[0] == 3 && n[2] < 1))
            rc = 4;
        else
            rc = h[1] == 4 ? run<float>(in, out, h[0], h[2], h[3], n, dt) : run<double>(in, out, h[0], h[2], h[3], n, dt);
    }
    fclose(in);
    return fclose(out) == 0 ? rc : 6;
}
