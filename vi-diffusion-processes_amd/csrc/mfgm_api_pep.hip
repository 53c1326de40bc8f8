// Power Expectation Propagation site updates and tilted moments (mfgm_pep.h): one launch over the selected points.
#include "mfgm_internal.h"
#include "mfgm_pep.h"

using namespace mfgm;

namespace {

bool pep_param_ok(int kind, double param, double alpha) {
    if (!(alpha > 0.0 && alpha <= 1.0)) return false;
    if (kind == MFGM_LIK_BERNOULLI) return param >= 0.0 && param < 0.5;
    if (kind == MFGM_LIK_POISSON || kind == MFGM_LIK_GAUSSIAN) return param > 0.0 && param < INFINITY;
    return false;
}

template <int KIND>
void launch_sites(size_t blocks, hipStream_t st, size_t n, size_t k, const int64_t* idx, const double* fmu, const double* fvar,
                  const double* y, double param, double alpha, double lr, double* nat1, double* nat2, double* lnorm, double* e_out,
                  int* skipped) {
    hipLaunchKernelGGL(k_pep_sites<KIND>, dim3((unsigned)blocks), dim3(256), 0, st, n, k, idx, fmu, fvar, y, param, alpha, lr, nat1, nat2,
                       lnorm, e_out, skipped);
}

template <int KIND>
void launch_tilted(size_t blocks, hipStream_t st, size_t n, const double* mc, const double* vc, const double* y, double param,
                   double alpha, double* lz, double* d1, double* d2) {
    hipLaunchKernelGGL(k_pep_tilted<KIND>, dim3((unsigned)blocks), dim3(256), 0, st, n, mc, vc, y, param, alpha, lz, d1, d2);
}

}  // namespace

extern "C" {

int mfgm_pep_sites(int kind, size_t n, const double* fmu, const double* fvar, const double* y, double param, double alpha, double lr,
                   const int64_t* idx, size_t k, double* nat1, double* nat2, double* lnorm, double* e_out, int* skipped, void* stream) {
    if (!pep_param_ok(kind, param, alpha)) return 1;
    if (!(lr >= 0.0 && lr <= 1.0)) return 1;
    const size_t count = idx ? k : n;
    if (count == 0) return 0;
    if (!fmu || !fvar || !y || !nat1 || !nat2) return 1;
    const size_t blocks = (count + 255) / 256;
    if (blocks > 0x7fffffffu) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (kind == MFGM_LIK_BERNOULLI)
        launch_sites<MFGM_LIK_BERNOULLI>(blocks, st, n, count, idx, fmu, fvar, y, param, alpha, lr, nat1, nat2, lnorm, e_out, skipped);
    else if (kind == MFGM_LIK_POISSON)
        launch_sites<MFGM_LIK_POISSON>(blocks, st, n, count, idx, fmu, fvar, y, param, alpha, lr, nat1, nat2, lnorm, e_out, skipped);
    else
        launch_sites<MFGM_LIK_GAUSSIAN>(blocks, st, n, count, idx, fmu, fvar, y, param, alpha, lr, nat1, nat2, lnorm, e_out, skipped);
    MFGM_CHECK_LAUNCH();
    return 0;
}

int mfgm_pep_tilted(int kind, size_t n, const double* mc, const double* vc, const double* y, double param, double alpha, double* lz,
                    double* d1, double* d2, void* stream) {
    if (!pep_param_ok(kind, param, alpha)) return 1;
    if (n == 0) return 0;
    if (!mc || !vc || !y) return 1;
    const size_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffu) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (kind == MFGM_LIK_BERNOULLI)
        launch_tilted<MFGM_LIK_BERNOULLI>(blocks, st, n, mc, vc, y, param, alpha, lz, d1, d2);
    else if (kind == MFGM_LIK_POISSON)
        launch_tilted<MFGM_LIK_POISSON>(blocks, st, n, mc, vc, y, param, alpha, lz, d1, d2);
    else
        launch_tilted<MFGM_LIK_GAUSSIAN>(blocks, st, n, mc, vc, y, param, alpha, lz, d1, d2);
    MFGM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
