// lagomorph_amd/csrc/energy_stencil.hpp on the CPU: the energy density and the operator value of every voxel of the
// planes it is given, in both precisions, built with a plain host compiler (tests/test_energy_host.py compares with
// tests/energy_ref.py: float32 bit for bit with the restatement, float64 against the definition).
//
//   energy_emul <cases> <results>
//
// cases:   int32 count; per case: int32 kind, dim, nx, ny, nz (dim 2: nx = 1), elem (4 or 8); 3 float64 spacings of
//          the axes (x, y, z); nx ny nz elements of `elem` bytes
// results: per case: nx ny nz densities, then nx ny nz operator values, `elem` bytes each
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../lagomorph_amd/csrc/energy_stencil.hpp"

static int clampi(int v, int n) { return v < 0 ? 0 : v > n - 1 ? n - 1 : v; }

template <typename R, int DIM>
static bool run(FILE *in, FILE *out, int kind, const int (&n)[3], const double *h) {
    const size_t nv = (size_t)n[0] * n[1] * n[2];
    std::vector<R> u(nv), dens(nv), op(nv);
    if (fread(u.data(), sizeof(R), nv, in) != nv) return false;
    const lago::EnergyWeights<R> w = lago::energy_weights<R>(kind, h);
    for (int x = 0; x < n[0]; ++x)
        for (int y = 0; y < n[1]; ++y)
            for (int z = 0; z < n[2]; ++z) {
                auto at = [&](int dx, int dy, int dz) {
                    return u[((size_t)clampi(x + dx, n[0]) * n[1] + clampi(y + dy, n[1])) * n[2] + clampi(z + dz, n[2])];
                };
                const lago::EnergyMask<R> q[3] = {lago::energy_mask<R>(x, n[0]), lago::energy_mask<R>(y, n[1]), lago::energy_mask<R>(z, n[2])};
                const size_t i = ((size_t)x * n[1] + y) * n[2] + z;
                if (kind == lago::kEnergyBending) {
                    dens[i] = lago::energy_bending_density<R, DIM>(w, q, at);
                    op[i] = lago::energy_bending_apply<R, DIM>(w, q, at);
                } else {
                    dens[i] = lago::energy_diffusion_density<R, DIM>(w, at);
                    op[i] = lago::energy_diffusion_apply<R, DIM>(w, at);
                }
            }
    return fwrite(dens.data(), sizeof(R), nv, out) == nv && fwrite(op.data(), sizeof(R), nv, out) == nv;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t count;
    if (fread(&count, sizeof count, 1, in) != 1) return 1;
    for (int32_t c = 0; c < count; ++c) {
        int32_t head[6];
        double h[3];
        if (fread(head, sizeof(int32_t), 6, in) != 6 || fread(h, sizeof(double), 3, in) != 3) return 1;
        const int kind = head[0], dim = head[1], elem = head[5];
        const int n[3] = {head[2], head[3], head[4]};
        if ((kind != 0 && kind != 1) || (dim != 2 && dim != 3) || (elem != 4 && elem != 8) || n[0] < 1 || n[1] < 1 || n[2] < 1 ||
            (dim == 2 && n[0] != 1))
            return 1;
        const bool ok = elem == 4 ? (dim == 3 ? run<float, 3>(in, out, kind, n, h) : run<float, 2>(in, out, kind, n, h))
                                  : (dim == 3 ? run<double, 3>(in, out, kind, n, h) : run<double, 2>(in, out, kind, n, h));
        if (!ok) return 1;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
