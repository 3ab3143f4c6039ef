// lagomorph_amd/csrc/ffd_weights.hpp on the CPU: ffd_axis for every (r, s), s = 1 .. 32, 0 <= r < s, in both
// precisions, and the control-extent formula, built with a plain host compiler (tests/test_ffd_host.py compares with
// tests/ffd_ref.py, bit for bit).
//
//   ffd_emul <results>
//
// results: for s = 1 .. 32, r = 0 .. s - 1:  5 float32 (t, 4 w);  then the same sweep as 5 float64;
//          then for s = 1 .. 32, n = 1 .. 200:  int64 ffd_ctrl_extent(n, s)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../lagomorph_amd/csrc/ffd_weights.hpp"

template <typename R>
static bool sweep(FILE *out) {
    std::vector<R> v;
    for (int s = 1; s <= lago::kFfdMaxSpacing; ++s)
        for (int r = 0; r < s; ++r) {
            const lago::FfdAxis<R> A = lago::ffd_axis<R>(r, s);
            v.push_back(A.t);
            for (int q = 0; q < 4; ++q) v.push_back(A.w[q]);
        }
    return fwrite(v.data(), sizeof(R), v.size(), out) == v.size();
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *out = fopen(argv[1], "wb");
    if (!out) return 2;
    if (!sweep<float>(out) || !sweep<double>(out)) return 1;
    std::vector<int64_t> m;
    for (int s = 1; s <= lago::kFfdMaxSpacing; ++s)
        for (int n = 1; n <= 200; ++n) m.push_back(lago::ffd_ctrl_extent(n, s));
    if (fwrite(m.data(), sizeof(int64_t), m.size(), out) != m.size()) return 1;
    return fclose(out) == 0 ? 0 : 1;
}
