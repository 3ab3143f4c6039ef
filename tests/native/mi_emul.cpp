// Host emulation of the Parzen joint histogram and its backward: every voxel of a case through the functions of
// lagomorph_amd/csrc/mi_window.hpp (the header mi.hip's kernels call), built by a plain host compiler with
// -ffp-contract=off as the library is.  tests/test_mi_host.py compares the output with tests/mi_ref.py bit for bit.
//
//   mi_emul <in> <out>
//   in : int32 B, int32 n, double loI, hiI, loJ, hiJ, double I[n], double J[n], double G[B * B]
//   out: int64 H[B * B] (sequential sum of the fixed-point products), int32 kI[n], int32 kJ[n],
//        double dwI[4 n], double dwJ[4 n], double dI[n], double dJ[n]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../lagomorph_amd/csrc/mi_window.hpp"

template <typename T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <typename T>
static bool wr(FILE *f, const T *p, size_t n) { return fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t B = 0, n = 0;
    double r[4];
    if (!rd(f, &B, 1) || !rd(f, &n, 1) || !rd(f, r, 4) || B < 4 || B > 64 || n < 0) return 4;
    std::vector<double> I(n), J(n), G((size_t)B * B);
    if (!rd(f, I.data(), n) || !rd(f, J.data(), n) || !rd(f, G.data(), G.size())) return 4;
    fclose(f);
    const lago::MiAxis aI = lago::mi_axis(r[0], r[1], B), aJ = lago::mi_axis(r[2], r[3], B);
    std::vector<long long> H((size_t)B * B, 0);
    std::vector<int32_t> kI(n), kJ(n);
    std::vector<double> dwI(4 * (size_t)n), dwJ(4 * (size_t)n), dI(n), dJ(n);
    for (int x = 0; x < n; ++x) {
        double tI, tJ, wI[4], wJ[4], dI4[4], dJ4[4], g[4][4];
        kI[x] = lago::mi_locate(I[x], aI, B, tI);
        kJ[x] = lago::mi_locate(J[x], aJ, B, tJ);
        if (kI[x] < 0 || kI[x] > B - 4 || kJ[x] < 0 || kJ[x] > B - 4) return 5;   // (the table below is indexed with them)
        lago::mi_weights(tI, wI);
        lago::mi_weights(tJ, wJ);
        lago::mi_derivs(I[x], tI, aI, dI4);
        lago::mi_derivs(J[x], tJ, aJ, dJ4);
        for (int a = 0; a < 4; ++a) {
            dwI[4 * (size_t)x + a] = dI4[a];
            dwJ[4 * (size_t)x + a] = dJ4[a];
            for (int b = 0; b < 4; ++b) {
                const size_t e = (size_t)(kI[x] + a) * B + (kJ[x] + b);
                H[e] += lago::mi_fixed(wI[a], wJ[b]);
                g[a][b] = G[e];
            }
        }
        dI[x] = lago::mi_grad_sum<false>(dI4, wJ, g) / (double)n;
        dJ[x] = lago::mi_grad_sum<true>(dJ4, wI, g) / (double)n;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 3;
    const bool ok = wr(f, H.data(), H.size()) && wr(f, kI.data(), n) && wr(f, kJ.data(), n) && wr(f, dwI.data(), dwI.size()) &&
                    wr(f, dwJ.data(), dwJ.size()) && wr(f, dI.data(), n) && wr(f, dJ.data(), n);
    return fclose(f) == 0 && ok ? 0 : 6;
}
