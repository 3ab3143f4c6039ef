// Fluid metric operator in the Fourier domain -- gfx950 HIP kernel.
//
// Replaces cuda/metric.cu of the reference (fluid_kernel_2d :162-218,
// fluid_kernel_3d :220-306, Cholesky helpers :20-130, OperatorMultiply
// :132-160).  Per frequency bin the symmetric matrix l (lambda on the diagonal,
// beta*sin*sin off it) is squared to L = l*l and either applied (flat) or
// inverted through its Cholesky factor (sharp), on the real and imaginary part
// of every vector component, in place on the interleaved-complex rFFT buffer.
//
// One lane per complex bin of the flattened (kx, ky, kz) index (kz fastest, 8 or
// 16 contiguous bytes per lane), batch loop inside the lane so the factor is
// computed once per bin exactly as the reference does.  Pure streaming: every
// byte of Fm is read once and written once.
#include "fluid.hpp"

namespace lago {

template <typename R, int DIM, bool INV>
__global__ __launch_bounds__(kBlock) void fluid_kernel(Cplx<R> *__restrict__ Fm, FluidOp<R> o, int nn, Geom g, R scale) {
    const Vox v = locate(g);
    if (!v.valid) return;
    const size_t nv = g.nvox;  // complex bins per component
    Cplx<R> *F = Fm + v.s;
    if (DIM == 3) {
        FluidBin3<R, INV> op;
        op.setup(o, v.i, v.j, v.k);
        for (int n = 0; n < nn; ++n, F += 3 * nv) {
            Cplx<R> a = F[0], b = F[nv], c = F[2 * nv];
            op.apply(a, b, c, scale);
            F[0] = a;
            F[nv] = b;
            F[2 * nv] = c;
        }
    } else {
        FluidBin2<R, INV> op;
        op.setup(o, v.j, v.k);
        for (int n = 0; n < nn; ++n, F += 2 * nv) {
            Cplx<R> a = F[0], b = F[nv];
            op.apply(a, b, scale);
            F[0] = a;
            F[nv] = b;
        }
    }
}

template <typename R>
int fluid_operator_impl(R *Fm, int inverse, const FluidOp<R> &op, int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz,
                        hipStream_t s, double scale) {
    if (dim != 2 && dim != 3) return fail_invalid("Only two- and three-dimensional fluid metric is supported");
    Geom g;
    if (nn < 0 || nn >= (1ll << 31) || !make_geom(g, dim, 1, nx, ny, nz))
        return fail_invalid("fluid_operator: bad extent");
    if (g.nblocks == 0 || nn == 0) return LAGO_OK;
    if (!Fm || !op.cosX || !op.sinX || !op.cosY || !op.sinY || (dim == 3 && (!op.cosZ || !op.sinZ)))
        return fail_invalid("fluid_operator: null pointer");
    if (((uintptr_t)Fm) % (2 * sizeof(R))) return fail_invalid("fluid_operator: Fmv must be aligned to a complex element");
    Cplx<R> *F = reinterpret_cast<Cplx<R> *>(Fm);
    with_dim(dim, [&](auto DIM) {
        with_flags([&](auto INV) {
            hipLaunchKernelGGL((fluid_kernel<R, DIM(), INV()>), dim3(g.nblocks), dim3(kBlock), 0, s, F, op, (int)nn, g,
                               (R)scale);
        }, inverse != 0);
    });
    return finish_launch(s, "fluid_operator");
}

template int fluid_operator_impl<float>(float *, int, const FluidOp<float> &, int, int64_t, int64_t, int64_t, int64_t,
                                        hipStream_t, double);
template int fluid_operator_impl<double>(double *, int, const FluidOp<double> &, int, int64_t, int64_t, int64_t, int64_t,
                                         hipStream_t, double);

}  // namespace lago

extern "C" {
#define LAGO_DEFINE(REAL, SUF)                                                                                    \
    int lago_fluid_operator##SUF(REAL *Fm, int inverse, const REAL *cosX, const REAL *sinX, const REAL *cosY,     \
                                 const REAL *sinY, const REAL *cosZ, const REAL *sinZ, double alpha, double beta, \
                                 double gamma, int dim, int64_t nn, int64_t nx, int64_t ny, int64_t nz,           \
                                 void *stream) {                                                                  \
        const lago::FluidOp<REAL> op{cosX, sinX, cosY, sinY, cosZ, sinZ, alpha, beta, gamma};                     \
        return lago::fluid_operator_impl<REAL>(Fm, inverse, op, dim, nn, nx, ny, nz, (hipStream_t)stream, 1.0);   \
    }
LAGO_DEFINE(float, _f32)
LAGO_DEFINE(double, _f64)
#undef LAGO_DEFINE
}
