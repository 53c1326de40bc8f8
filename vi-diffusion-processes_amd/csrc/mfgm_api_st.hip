// C-ABI entry points of the spatio-temporal sparse CVI local kernels (mfgm_st.h).
#include "mfgm_internal.h"
#include "mfgm_st.h"
#include "mfgm_sweeps.h"

using namespace mfgm;

namespace {
// D = Ms dt in 9 .. 32 (the factors are bounded first, so the product cannot overflow), every array the description names present
bool st_ok(const mfgm_st_data* s) {
    if (!s || s->M < 1 || s->N < 0 || s->Ms < 1 || s->Ms > 32 || s->dt < 1 || s->dt > 32) return false;
    const int d = s->Ms * s->dt;
    if (d < 9 || d > 32) return false;
    return s->seg && (s->N == 0 || (s->a && s->h && s->c));
}
StArgs st_args(const mfgm_st_data* s) {
    StArgs a;
    a.M = s->M; a.Ms = s->Ms; a.dt = s->dt; a.d = s->Ms * s->dt; a.N = s->N;
    a.seg = s->seg; a.a = s->a; a.h = s->h; a.c = s->c; a.prior_mean = s->prior_mean; a.prior_cov = s->prior_cov;
    return a;
}
}  // namespace

extern "C" {

int mfgm_st_predict_kl(const mfgm_st_data* data, const double* mu, const double* Sig, const double* Sub, double* fmu, double* fvar,
                       const mfgm_plan* plan, const double* Pd, const double* Ps, double aD, double aS, const double* mup, double* trace,
                       double* maha, void* ws, void* stream) {
    if (!st_ok(data) || !mu || !Sig || !Sub || !fmu || !fvar || !data->prior_mean || !data->prior_cov) return 1;
    const StArgs sa = st_args(data);
    SparseKl kl;
    memset(&kl, 0, sizeof(kl));
    const bool want_kl = plan && trace && maha;
    if (want_kl) {
        if (!Pd || !Ps || !mup || !ws) return 1;
        const Plan& P = plan->p;
        if (!P.wide || P.B != 1 || P.T != data->M || P.d != sa.d) return 1;
        kl = SparseKl{Pd, Ps, mup, aD, aS, (double*)ws + P.off_part[0]};
    } else if (data->N == 0) {
        return 0;
    }
    const size_t shmem = sizeof(double) * ((size_t)kStChunk * (2 * sa.d + 1) + 4 * sa.d);
#define ST_PREDICT(NJ_, PAIR_)                                                                                                      \
    hipLaunchKernelGGL((k_st_predict<NJ_, PAIR_>), dim3(sa.M + 1), dim3(64), shmem, (hipStream_t)stream, sa, mu, Sig, Sub, fmu, fvar, kl)
    if (sa.d % 2 == 0) {
        // even d: blocks and their rows are 16-byte aligned, a lane holds pairs of entries
        const int nj = (sa.d * sa.d / 2 + 63) / 64;
        if (nj <= 2) ST_PREDICT(2, true); else if (nj <= 4) ST_PREDICT(4, true); else ST_PREDICT(8, true);
    } else {
        const int nj = (sa.d * sa.d + 63) / 64;
        if (nj <= 2) ST_PREDICT(2, false); else if (nj <= 4) ST_PREDICT(4, false); else if (nj <= 8) ST_PREDICT(8, false);
        else ST_PREDICT(16, false);
    }
#undef ST_PREDICT
    MFGM_CHECK_LAUNCH();
    if (!want_kl) return 0;
    const Plan& P = plan->p;
    return launch_sum_partials(kl.part, sa.M + 1, sa.M + 1, 1, trace, maha, (double*)ws + P.off_part2, (hipStream_t)stream);
}

int mfgm_st_site_update_q(const mfgm_st_data* data, const double* g1, const double* g2, double lr, double* nat1, double* nat2q,
                          void* stream) {
    if (!st_ok(data) || !nat1 || !nat2q || (data->N > 0 && (!g1 || !g2))) return 1;
    const StArgs sa = st_args(data);
    const int d = sa.d, QS = d * (d + 1) + d * d;
    const size_t shmem = sizeof(double) * kSitesQChunk * (2 * d + 2);
    const int per_wg = kSitesQG * kSitesQRounds;
    const dim3 grid((sa.M + 1 + per_wg - 1) / per_wg);
    const int ne = (QS + 255) / 256;
#define ST_SITESQ(NE_) hipLaunchKernelGGL((k_st_sites_q<NE_>), grid, dim3(256), shmem, (hipStream_t)stream, sa, g1, g2, lr, nat1, nat2q)
    if (ne <= 1) ST_SITESQ(1); else if (ne <= 2) ST_SITESQ(2); else if (ne <= 3) ST_SITESQ(3); else if (ne <= 4) ST_SITESQ(4);
    else if (ne <= 6) ST_SITESQ(6); else if (ne <= 8) ST_SITESQ(8); else if (ne <= 9) ST_SITESQ(9); else return 1;
#undef ST_SITESQ
    MFGM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
