// Host emulation of distance_transform: every line of every case through lagomorph_amd/csrc/edt_line.hpp, in float32
// and in the kernels' pass order (last axis first).  tests/test_edt_host.py writes the cases, compares the results with
// tests/edt_ref.py, and runs this program once more built with -fsanitize=address,undefined.
//
//   edt_emul cases.bin out.bin
//   case  : int32 dim, N, nx, ny, nz (dim 2: nx = 1), where, label; float32 sx, sy, sz; int32 L[N nx ny nz]
//   result: int32 feature[N nx ny nz] (0 / 1); float32 squared distance[N nx ny nz]
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../lagomorph_amd/csrc/edt_line.hpp"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t h[7];
    while (fread(h, sizeof(int32_t), 7, in) == 7) {
        const int dim = h[0], N = h[1], nx = h[2], ny = h[3], nz = h[4], where = h[5];
        const int32_t label = h[6];
        float s[3];
        if (fread(s, sizeof(float), 3, in) != 3) return 3;
        if ((dim != 2 && dim != 3) || N < 1 || nx < 1 || ny < 1 || nz < 1 || nx > lago::EDT_MAX_EXTENT || ny > lago::EDT_MAX_EXTENT ||
            nz > lago::EDT_MAX_EXTENT)
            return 3;
        const size_t nvox = (size_t)nx * ny * nz;
        std::vector<int32_t> L(N * nvox), feat(N * nvox);
        std::vector<float> g(N * nvox), line(lago::EDT_MAX_EXTENT);
        if (fread(L.data(), sizeof(int32_t), L.size(), in) != L.size()) return 3;
        for (int n = 0; n < N; ++n) {
            const int32_t *Lv = L.data() + n * nvox;
            float *gv = g.data() + n * nvox;
            // the first pass forms g from L as it loads a line ...
            for (int x = 0; x < nx; ++x)
                for (int y = 0; y < ny; ++y)
                    for (int z = 0; z < nz; ++z) {
                        const bool f = lago::edt_feature(Lv, where, label, dim, x, y, z, nx, ny, nz);
                        feat[n * nvox + ((size_t)x * ny + y) * nz + z] = f;
                        gv[((size_t)x * ny + y) * nz + z] = lago::edt_g0(f);
                    }
            // ... and every pass works on a copy of its line (the kernels' LDS tile) and writes in place
            std::vector<float> tmp(lago::EDT_MAX_EXTENT);
            const auto run = [&](float *at, int len, int64_t stride, float sp) {
                for (int j = 0; j < len; ++j) line[j] = at[j * stride];
                lago::edt_line(tmp.data(), line.data(), len, sp);
                for (int j = 0; j < len; ++j) at[j * stride] = tmp[j];
            };
            for (int x = 0; x < nx; ++x)
                for (int y = 0; y < ny; ++y) run(gv + ((size_t)x * ny + y) * nz, nz, 1, s[2]);
            for (int x = 0; x < nx; ++x)
                for (int z = 0; z < nz; ++z) run(gv + (size_t)x * ny * nz + z, ny, nz, s[1]);
            if (dim == 3)
                for (int y = 0; y < ny; ++y)
                    for (int z = 0; z < nz; ++z) run(gv + (size_t)y * nz + z, nx, (int64_t)ny * nz, s[0]);
        }
        if (fwrite(feat.data(), sizeof(int32_t), feat.size(), out) != feat.size()) return 4;
        if (fwrite(g.data(), sizeof(float), g.size(), out) != g.size()) return 4;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
