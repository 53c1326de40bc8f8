// C-ABI entry points of the sparse Power EP site update (mfgm_spep.h): one launch over the intervals.
#include "mfgm_internal.h"
#include "mfgm_spep.h"

using namespace mfgm;

namespace {

bool spep_param_ok(int kind, double param, double alpha, double lr) {
    if (!(alpha > 0.0 && alpha <= 1.0) || !(lr >= 0.0 && lr <= 1.0)) return false;
    if (kind == MFGM_LIK_BERNOULLI) return param >= 0.0 && param < 0.5;
    if (kind == MFGM_LIK_POISSON || kind == MFGM_LIK_GAUSSIAN) return param > 0.0 && param < INFINITY;
    return false;
}

template <int KIND>
int launch_spep(const SparseArgs& sa, int packed, const double* y, double param, double alpha, double lr, const double* mu, const double* Sig,
                const double* Sub, double* nat1, double* nat2, double* lnorm, double* e_out, int* skipped, hipStream_t st) {
    const int n = 2 * sa.d, ni = sa.m_hi - sa.m_lo;
#define SPEP(NP_)                                                                                                                    \
    hipLaunchKernelGGL((k_spep_sites<KIND, NP_>), dim3((ni + 64 / NP_ - 1) / (64 / NP_)), dim3(64),                                   \
                       sizeof(double) * (64 / NP_) * spep_lds_doubles(n), st, sa, packed, y, param, alpha, lr, mu, Sig, Sub, nat1, nat2, \
                       lnorm, e_out, skipped)
    if (n <= 2) SPEP(2); else if (n <= 4) SPEP(4); else if (n <= 8) SPEP(8); else if (n <= 16) SPEP(16);
    else if (n <= 32) SPEP(32); else SPEP(64);
#undef SPEP
    MFGM_CHECK_LAUNCH();
    return 0;
}

int spep_sites(const mfgm_sparse_data* s, int packed, int kind, const double* y, double param, double alpha, double lr, const double* mu,
               const double* Sig, const double* Sub, double* nat1, double* nat2, double* lnorm, double* e_out, int* skipped, void* stream) {
    if (!spep_param_ok(kind, param, alpha, lr)) return 1;
    if (!(s && s->M >= 1 && s->d >= 1 && s->d <= 32 && s->N >= 0 && s->seg && (s->N == 0 || (s->w && s->c && y)))) return 1;
    if (s->m_hi > 0 && !(s->m_lo >= 0 && s->m_lo < s->m_hi && s->m_hi <= s->M + 1)) return 1;
    if (!mu || !Sig || !Sub || !nat1 || !nat2 || !s->prior_mean || !s->prior_cov) return 1;
    SparseArgs a;
    a.M = s->M; a.d = s->d; a.N = s->N; a.seg = s->seg;
    a.m_lo = (s->m_hi > 0) ? s->m_lo : 0;
    a.m_hi = (s->m_hi > 0) ? s->m_hi : s->M + 1;
    a.w = s->w; a.c = s->c; a.prior_mean = s->prior_mean; a.prior_cov = s->prior_cov;
    hipStream_t st = (hipStream_t)stream;
    if (kind == MFGM_LIK_BERNOULLI)
        return launch_spep<MFGM_LIK_BERNOULLI>(a, packed, y, param, alpha, lr, mu, Sig, Sub, nat1, nat2, lnorm, e_out, skipped, st);
    if (kind == MFGM_LIK_POISSON)
        return launch_spep<MFGM_LIK_POISSON>(a, packed, y, param, alpha, lr, mu, Sig, Sub, nat1, nat2, lnorm, e_out, skipped, st);
    return launch_spep<MFGM_LIK_GAUSSIAN>(a, packed, y, param, alpha, lr, mu, Sig, Sub, nat1, nat2, lnorm, e_out, skipped, st);
}

}  // namespace

extern "C" {

int mfgm_sparse_pep_sites(const mfgm_sparse_data* data, int kind, const double* y, double param, double alpha, double lr, const double* mu,
                          const double* Sig, const double* Sub, double* nat1, double* nat2, double* lnorm, double* e_out, int* skipped,
                          void* stream) {
    return spep_sites(data, 0, kind, y, param, alpha, lr, mu, Sig, Sub, nat1, nat2, lnorm, e_out, skipped, stream);
}

int mfgm_sparse_pep_sites_q(const mfgm_sparse_data* data, int kind, const double* y, double param, double alpha, double lr,
                            const double* mu, const double* Sig, const double* Sub, double* nat1, double* nat2q, double* lnorm,
                            double* e_out, int* skipped, void* stream) {
    return spep_sites(data, 1, kind, y, param, alpha, lr, mu, Sig, Sub, nat1, nat2q, lnorm, e_out, skipped, stream);
}

}  // extern "C"
