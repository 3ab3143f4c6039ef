// lagomorph_amd/csrc/bspline_weights.hpp on the CPU: every position of every case through bs_axis and bs_dweights, built
// with a plain host compiler (tests/test_bspline_host.py compares with tests/bspline_ref.py, bit for bit).
//
//   bspline_emul <cases> <results>
//
// cases:   per case  int32 itemsize (4 | 8), int32 n, int32 count; then count positions of that size
// results: per case  count x (4 int32 k, int32 f, int32 clamped | nan << 1), then count x (t, 4 w, 4 dw) of that size
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../lagomorph_amd/csrc/bspline_weights.hpp"

template <typename R>
static bool run_case(FILE *in, FILE *out, int n, int count) {
    std::vector<R> x(count);
    if (count && fread(x.data(), sizeof(R), count, in) != (size_t)count) return false;
    std::vector<int32_t> ints((size_t)count * 6);
    std::vector<R> reals((size_t)count * 9);
    for (int p = 0; p < count; ++p) {
        lago::BsAxis<R> A;
        lago::bs_axis(x[p], n, A);
        R dw[4];
        lago::bs_dweights(A, dw);
        for (int q = 0; q < 4; ++q) {
            if (A.k[q] < 0 || A.k[q] > n - 1) {
                fprintf(stderr, "tap %d of position %d outside [0, %d]\n", A.k[q], p, n - 1);
                return false;
            }
            ints[(size_t)p * 6 + q] = A.k[q];
            reals[(size_t)p * 9 + 1 + q] = A.w[q];
            reals[(size_t)p * 9 + 5 + q] = dw[q];
        }
        ints[(size_t)p * 6 + 4] = A.f;
        ints[(size_t)p * 6 + 5] = (A.clamped ? 1 : 0) | (A.nan ? 2 : 0);
        reals[(size_t)p * 9] = A.t;
    }
    return fwrite(ints.data(), sizeof(int32_t), ints.size(), out) == ints.size() &&
           fwrite(reals.data(), sizeof(R), reals.size(), out) == reals.size();
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t head[3];
    while (fread(head, sizeof(int32_t), 3, in) == 3) {
        const bool ok = head[0] == 4 ? run_case<float>(in, out, head[1], head[2])
                                     : head[0] == 8 ? run_case<double>(in, out, head[1], head[2]) : false;
        if (!ok) return 1;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
