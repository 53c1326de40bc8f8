// Scalar non-Gaussian likelihoods of the CVI models (mfgm_lik.h): one launch over the observations.
#include "mfgm_internal.h"
#include "mfgm_lik.h"

using namespace mfgm;

extern "C" {

int mfgm_scalar_lik(int kind, size_t n, const double* fmu, const double* fvar, const double* y, double param, double* ve, double* g1,
                    double* g2, void* stream) {
    if (kind != MFGM_LIK_BERNOULLI && kind != MFGM_LIK_POISSON) return 1;
    if (kind == MFGM_LIK_BERNOULLI && !(param >= 0.0 && param < 0.5)) return 1;
    if (kind == MFGM_LIK_POISSON && !(param > 0.0)) return 1;
    if (n == 0) return 0;
    if (!fmu || !fvar || !y) return 1;
    const size_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffu) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (kind == MFGM_LIK_BERNOULLI)
        hipLaunchKernelGGL(k_scalar_lik<MFGM_LIK_BERNOULLI>, dim3((unsigned)blocks), dim3(256), 0, st, n, fmu, fvar, y, param, ve, g1, g2);
    else
        hipLaunchKernelGGL(k_scalar_lik<MFGM_LIK_POISSON>, dim3((unsigned)blocks), dim3(256), 0, st, n, fmu, fvar, y, param, ve, g1, g2);
    MFGM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
