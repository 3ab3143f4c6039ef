// Host emulation of the pyramid kernels' arithmetic: lagomorph_amd/csrc/pyramid_weights.hpp, the header the kernels
// call, run by a plain host compiler (tests/test_pyramid_host.py).
//
//   pyramid_emul entries OUT          for n = 1 .. 40: R[j][x] (m x n doubles, row-major), then E[x][j] (n x m doubles)
//   pyramid_emul IN OUT               IN: int32 count, then per case int32 op (0 reduce, 1 reduce_adjoint, 2 expand,
//                                     3 expand_adjoint), int32 n[3] (the FINE extents as laid out in memory; 2D: n[0] = 1),
//                                     int32 elem (4 or 8), double scale, the input plane in that precision.
//                                     OUT: the output planes, one after the other.
//
// One plane is contracted axis by axis in the header's order (kPyrDownOrder, kPyrUpOrder), every tap through
// pyr_down_weight / pyr_up_weight and pyr_dot; a tap outside the axis reads the clamped cell (down) or 0 (up), as the
// kernels' staged tiles hold them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../lagomorph_amd/csrc/pyramid_weights.hpp"

using namespace lago;

template <typename R, typename W, bool UP>
static std::vector<R> contract(const std::vector<R> &in, int (&ext)[3], int axis, int n) {
    const int m = (int)pyr_coarse_extent(n), nin = UP ? m : n, nout = UP ? n : m;
    int oe[3] = {ext[0], ext[1], ext[2]};
    oe[axis] = nout;
    std::vector<R> out((size_t)oe[0] * oe[1] * oe[2]);
    const size_t stride = axis == 0 ? (size_t)ext[1] * ext[2] : axis == 1 ? (size_t)ext[2] : 1;
    int i[3];
    for (i[0] = 0; i[0] < oe[0]; ++i[0])
        for (i[1] = 0; i[1] < oe[1]; ++i[1])
            for (i[2] = 0; i[2] < oe[2]; ++i[2]) {
                const int o = i[axis];
                int b[3] = {i[0], i[1], i[2]};
                b[axis] = 0;
                const R *line = in.data() + ((size_t)b[0] * ext[1] + b[1]) * ext[2] + b[2];
                R w[kPyrDownTaps];
                R acc;
                if (UP) {
                    for (int t = 0; t < kPyrUpTaps; ++t) w[t] = pyr_up_weight<R, W>(o, t, n);
                    const int first = pyr_up_first(o);
                    acc = pyr_dot<kPyrUpTaps>(w, [&](int t) { return first + t >= 0 && first + t < nin ? line[(size_t)(first + t) * stride] : (R)0; });
                } else {
                    for (int k = 0; k < kPyrDownTaps; ++k) w[k] = pyr_down_weight<R, W>(o, k, n);
                    const int first = pyr_down_first(o);
                    acc = pyr_dot<kPyrDownTaps>(w, [&](int k) { return line[(size_t)pyr_clamp(first + k, nin) * stride]; });
                }
                out[((size_t)i[0] * oe[1] + i[1]) * oe[2] + i[2]] = acc;
            }
    ext[axis] = nout;
    return out;
}

template <typename R, typename W, bool UP>
static std::vector<R> apply(std::vector<R> v, const int (&n)[3], double scale) {
    int ext[3];
    for (int a = 0; a < 3; ++a) ext[a] = UP ? (int)pyr_coarse_extent(n[a]) : n[a];
    for (int s = 0; s < 3; ++s) {
        const int axis = UP ? kPyrUpOrder[s] : kPyrDownOrder[s];
        v = contract<R, W, UP>(v, ext, axis, n[axis]);
    }
    for (R &x : v) x = pyr_scale(x, scale);
    return v;
}

template <typename R>
static bool run_case(FILE *in, FILE *out, int op, const int (&n)[3], double scale) {
    const bool up = op == 1 || op == 2;
    size_t count = 1;
    for (int a = 0; a < 3; ++a) count *= (size_t)(up ? (int)pyr_coarse_extent(n[a]) : n[a]);
    std::vector<R> v(count);
    if (fread(v.data(), sizeof(R), count, in) != count) return false;
    std::vector<R> r = op == 0   ? apply<R, PyrReduce, false>(v, n, scale)
                       : op == 1 ? apply<R, PyrReduce, true>(v, n, scale)
                       : op == 2 ? apply<R, PyrExpand, true>(v, n, scale)
                                 : apply<R, PyrExpand, false>(v, n, scale);
    return fwrite(r.data(), sizeof(R), r.size(), out) == r.size();
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    if (!strcmp(argv[1], "entries")) {
        FILE *out = fopen(argv[2], "wb");
        if (!out) return 3;
        for (int n = 1; n <= 40; ++n) {
            const int m = (int)pyr_coarse_extent(n);
            std::vector<double> e;
            for (int j = 0; j < m; ++j)
                for (int x = 0; x < n; ++x) e.push_back(PyrReduce::at<double>(j, x, n));
            for (int x = 0; x < n; ++x)
                for (int j = 0; j < m; ++j) e.push_back(PyrExpand::at<double>(j, x, n));
            // the float32 entries are the same numbers, and nothing lies outside the tap ranges
            for (int j = 0; j < m; ++j)
                for (int x = 0; x < n; ++x) {
                    if ((double)PyrReduce::at<float>(j, x, n) != PyrReduce::at<double>(j, x, n)) return 4;
                    if ((double)PyrExpand::at<float>(j, x, n) != PyrExpand::at<double>(j, x, n)) return 4;
                    const bool down = x >= pyr_down_first(j) && x < pyr_down_first(j) + kPyrDownTaps;
                    const bool upr = j >= pyr_up_first(x) && j < pyr_up_first(x) + kPyrUpTaps;
                    if ((!down || !upr) && (PyrReduce::at<double>(j, x, n) != 0 || PyrExpand::at<double>(j, x, n) != 0)) return 5;
                }
            if (fwrite(e.data(), sizeof(double), e.size(), out) != e.size()) return 3;
        }
        return fclose(out) ? 3 : 0;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    int32_t count;
    if (fread(&count, 4, 1, in) != 1) return 3;
    for (int32_t c = 0; c < count; ++c) {
        int32_t head[5];
        double scale;
        if (fread(head, 4, 5, in) != 5 || fread(&scale, 8, 1, in) != 1) return 3;
        const int n[3] = {head[1], head[2], head[3]};
        const bool ok = head[4] == 4 ? run_case<float>(in, out, head[0], n, scale) : run_case<double>(in, out, head[0], n, scale);
        if (!ok) return 3;
    }
    fclose(in);
    return fclose(out) ? 3 : 0;
}
