// Sums of products of stationary SDE kernels -> packed SSM parameters (mfgm_kernel_ssm.h), one set of parameters for the whole grid
// or one per region between change points (mfgm_piecewise_ssm.h).
#include "mfgm_internal.h"
#include "mfgm_kernel_ssm.h"
#include "mfgm_piecewise_ssm.h"

using namespace mfgm;

namespace {
int factor_dim(int kind) {
    switch (kind) {
        case MFGM_FACTOR_MATERN12: case MFGM_FACTOR_CONSTANT: return 1;
        case MFGM_FACTOR_MATERN32: case MFGM_FACTOR_HARMONIC: return 2;
        case MFGM_FACTOR_MATERN52: return 3;
        default: return 0;
    }
}

template <int D>
int kernel_ssm_impl(const Plan& P, const KernelTermsDev& kt, const double* dts, double* A, double* off, double* chol, int* info,
                    hipStream_t st) {
    const LevelDesc& lv = P.lv[0];
    hipLaunchKernelGGL((k_kernel_ssm<D>), dim3(lv.Lpad / 64), dim3(64), 0, st, lv, kt, dts, A, off, chol, info);
    MFGM_CHECK_LAUNCH();
    return 0;
}

template <int D>
int piecewise_ssm_impl(const Plan& P, const KernelTermsDev& kt, const PiecewiseDev& pw, const double* tps, double* A, double* off,
                       double* chol, int* info, hipStream_t st) {
    const LevelDesc& lv = P.lv[0];
    hipLaunchKernelGGL((k_piecewise_ssm<D>), dim3(lv.Lpad / 64), dim3(64), 0, st, lv, kt, pw, tps, A, off, chol, info);
    MFGM_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// The caller's terms -> the kernels' form (1 x 1 factors behind the others; src[c][slot] = the caller's factor in that slot), with
// every structural check of the entry points that take mfgm_kernel_terms (declared in mfgm_internal.h).  0, or 1 for a structure the
// kernels do not take.
int mfgm::device_terms(const Plan& P, const mfgm_kernel_terms& in, KernelTermsDev& kt, int (*src)[3]) {
    if (P.wide || P.d > 8) return 1;
    int dim = 0;
    if (device_terms(in, kt, src, dim)) return 1;
    return dim != P.d;
}

// The same without a plan: the state dimension is the terms' own (d: out).
int mfgm::device_terms(const mfgm_kernel_terms& in, KernelTermsDev& kt, int (*src)[3], int& d) {
    if (in.nterm < 1 || in.nterm > 8) return 1;
    memset(&kt, 0, sizeof(kt));
    kt.nterm = in.nterm;
    int dim = 0;
    for (int c = 0; c < in.nterm; ++c) {
        const int nf = in.nfactor[c];
        if (nf < 1 || nf > 3 || in.offset[c] != dim) return 1;
        int n = 1;
        for (int f = 0; f < nf; ++f) {
            const int fd = factor_dim(in.kind[c][f]);
            if (fd == 0) return 1;
            n *= fd;
        }
        if (dim + n > 8) return 1;
        // 1 x 1 factors commute through the Kronecker product: move them behind the others, keeping the others' order
        int slot = 0, shape = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int f = 0; f < nf; ++f) {
                const int fd = factor_dim(in.kind[c][f]);
                if ((fd > 1) != (pass == 0)) continue;
                kt.kind[c][slot] = in.kind[c][f];
                kt.rate[c][slot] = in.rate[c][f];
                kt.var[c][slot] = in.var[c][f];
                src[c][slot] = f;
                if (fd > 1) shape = shape * 10 + fd;
                ++slot;
            }
        switch (shape) {
            case 0: kt.shape[c] = KT_SHAPE_1; break;
            case 2: kt.shape[c] = KT_SHAPE_2; break;
            case 3: kt.shape[c] = KT_SHAPE_3; break;
            case 22: kt.shape[c] = KT_SHAPE_22; break;
            case 23: kt.shape[c] = KT_SHAPE_23; break;
            case 32: kt.shape[c] = KT_SHAPE_32; break;
            case 222: kt.shape[c] = KT_SHAPE_222; break;
            default: return 1;
        }
        kt.offset[c] = dim;
        dim += n;
    }
    for (int i = 0; i < dim; ++i) kt.mean[i] = in.mean[i];
    kt.jitter = in.jitter;
    d = dim;
    return 0;
}

extern "C" int mfgm_packed_kernel_ssm(const mfgm_plan* plan, const mfgm_kernel_terms* terms, const double* time_deltas, double* A,
                                      double* off, double* chol, int* info, void* stream) {
    if (!plan || !terms || !A || !off || !chol || !info) return 1;
    const Plan& P = plan->p;
    if (P.T > 1 && !time_deltas) return 1;
    KernelTermsDev kt;
    int src[8][3] = {};
    if (device_terms(P, *terms, kt, src)) return 1;
    hipStream_t st = (hipStream_t)stream;
    MFGM_DISPATCH_D(P.d, (kernel_ssm_impl<DD>(P, kt, time_deltas, A, off, chol, info, st)));
}

extern "C" int mfgm_packed_piecewise_ssm(const mfgm_plan* plan, const mfgm_piecewise_terms* terms, const double* time_points, double* A,
                                         double* off, double* chol, int* info, void* stream) {
    if (!plan || !terms || !time_points || !A || !off || !chol || !info) return 1;
    const Plan& P = plan->p;
    const mfgm_piecewise_terms& in = *terms;
    if (in.nregion < 1 || !in.rate || !in.var || !in.mean) return 1;
    if (in.nregion > 1 && !in.change_points) return 1;
    KernelTermsDev kt;
    PiecewiseDev pw;
    memset(&pw, 0, sizeof(pw));
    if (device_terms(P, in.base, kt, pw.src)) return 1;
    pw.nregion = in.nregion;
    pw.cp = in.change_points;
    pw.rate = in.rate;
    pw.var = in.var;
    pw.mean = in.mean;
    hipStream_t st = (hipStream_t)stream;
    MFGM_DISPATCH_D(P.d, (piecewise_ssm_impl<DD>(P, kt, pw, time_points, A, off, chol, info, st)));
}
