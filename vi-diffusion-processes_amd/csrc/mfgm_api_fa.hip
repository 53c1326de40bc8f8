// C-ABI entry points of the factor-analysis sparse CVI local kernels (mfgm_fa.h).
#include <cmath>

#include "mfgm_fa.h"
#include "mfgm_internal.h"

using namespace mfgm;

namespace {
// L in 1 .. 8, P in 1 .. 64, every dl >= 1, D = sum dl in 2 .. 32 (each dl is bounded first, so the sum cannot overflow), w_stride 0 or
// P L; the arrays over data points that both passes read present when there is a data point
bool fa_ok(const mfgm_fa_data* s) {
    if (!s || s->M < 1 || s->N < 0 || s->L < 1 || s->L > kFaMaxL || s->P < 1 || s->P > kFaMaxP) return false;
    int D = 0;
    for (int l = 0; l < s->L; ++l) {
        if (s->dl[l] < 1 || s->dl[l] > 32) return false;
        D += s->dl[l];
    }
    if (D < 2 || D > 32) return false;
    if (s->w_stride != 0 && s->w_stride != (long long)s->P * s->L) return false;
    return s->seg && (s->N == 0 || (s->h && s->c));
}
FaArgs fa_args(const mfgm_fa_data* s) {
    FaArgs a;
    memset(&a, 0, sizeof(a));
    a.M = s->M; a.L = s->L; a.P = s->P; a.N = s->N;
    int D = 0;
    for (int l = 0; l < s->L; ++l) {
        a.dl[l] = s->dl[l];
        a.off[l] = D;
        D += s->dl[l];
    }
    a.D = D;
    a.seg = s->seg; a.h = s->h; a.c = s->c; a.w = s->w; a.w_stride = s->w_stride;
    a.prior_mean = s->prior_mean; a.prior_cov = s->prior_cov;
    return a;
}
// 0: a bad kind or parameter; 1: every kind 0 (prediction only); 2: every output has a likelihood (the ranges of mfgm_scalar_lik /
// mfgm_pep_sites)
int lik_mode(const mfgm_fa_data* s, const mfgm_fa_lik* lik) {
    if (!lik) return 0;
    int none = 0;
    for (int p = 0; p < s->P; ++p) {
        const double prm = lik->param[p];
        switch (lik->kind[p]) {
            case 0: ++none; break;
            case MFGM_LIK_BERNOULLI:
                if (!(prm >= 0.0 && prm < 0.5)) return 0;
                break;
            case MFGM_LIK_POISSON: case MFGM_LIK_GAUSSIAN:
                if (!(prm > 0.0 && prm < HUGE_VAL)) return 0;
                break;
            default: return 0;
        }
    }
    if (none == s->P) return 1;
    return none == 0 ? 2 : 0;
}

template <bool PACKED>
int launch_sites(const mfgm_fa_data* data, const double* gam1, const double* gam2, double lr, double* nat1, double* nat2, void* stream) {
    if (!fa_ok(data) || !nat1 || !nat2 || !(lr >= 0.0 && lr <= 1.0) || (data->N > 0 && (!gam1 || !gam2))) return 1;
    const FaArgs a = fa_args(data);
    const int D = a.D, QS = PACKED ? D * (D + 1) + D * D : 4 * D * D;
    const size_t shmem = sizeof(double) * kFaSitesChunk * (2 * D + a.L + a.L * (a.L + 1) / 2) + sizeof(int) * 2 * D;
    const int ne = (QS + 255) / 256;
#define FA_SITES(NE_) hipLaunchKernelGGL((k_fa_sites<NE_, PACKED>), dim3(a.M + 1), dim3(256), shmem, (hipStream_t)stream, a, gam1, gam2, lr, nat1, nat2)
    if (ne <= 1) FA_SITES(1); else if (ne <= 2) FA_SITES(2); else if (ne <= 4) FA_SITES(4); else if (ne <= 6) FA_SITES(6);
    else if (ne <= 9) FA_SITES(9); else if (ne <= 12) FA_SITES(12); else if (ne <= 16) FA_SITES(16); else return 1;
#undef FA_SITES
    MFGM_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" {

int mfgm_fa_predict_lik(const mfgm_fa_data* data, const mfgm_fa_lik* lik, const double* y, const double* mu, const double* Sig,
                        const double* Sub, double* fmu, double* fvar, double* lmu, double* lcov, double* ve_part, double* dm, double* dv,
                        double* gam1, double* gam2, void* stream) {
    if (!fa_ok(data)) return 1;
    const int mode = lik_mode(data, lik);
    if (mode == 0) return 1;
    const bool has_lik = mode == 2;
    if (!has_lik && (y || ve_part || dm || dv || gam1 || gam2)) return 1;
    if (data->N > 0 && (!mu || !Sig || !Sub || !data->w || !data->prior_mean || !data->prior_cov || (has_lik && !y))) return 1;
    if (data->N == 0) return 0;
    const FaArgs a = fa_args(data);
    FaLik lk;
    memset(&lk, 0, sizeof(lk));
    for (int p = 0; p < a.P; ++p) {
        lk.kind[p] = lik->kind[p];
        lk.param[p] = lik->param[p];
    }
    const bool wconst = a.w_stride == 0;
    const int DD = a.D * a.D, NB = DD | 1;
    // intervals per wavefront: about 64 data points' worth of them, as many as ~40 KB of LDS hold, at most kFaMaxGroup, at least 1
    const size_t fixed = sizeof(double) * ((size_t)kFaChunk * (2 * a.D + 1) + kFaChunk + NB + a.D + (wconst ? a.P * a.L : 0)) + sizeof(int);
    const size_t per_g = sizeof(double) * ((size_t)2 * NB + a.D) + sizeof(int);
    const long long want = ((long long)kFaChunk * (a.M + 1) + a.N - 1) / a.N;
    const long long fit = fixed < 40960 ? (long long)((40960 - fixed) / per_g) : 0;
    const int G = (int)std::max(1LL, std::min({want, fit, (long long)kFaMaxGroup}));
    const size_t shmem = fixed + (size_t)G * per_g;
    if (shmem > 65536) return 1;
    const dim3 grid((a.M + 1 + G - 1) / G);
#define FA_PREDICT(LMAX_, LIK_, WC_)                                                                                                 \
    hipLaunchKernelGGL((k_fa_predict_lik<LMAX_, LIK_, WC_>), grid, dim3(64), shmem, (hipStream_t)stream, a, lk, G, y, mu, Sig, Sub, fmu, \
                       fvar, lmu, lcov, ve_part, dm, dv, gam1, gam2)
#define FA_PREDICT_L(LMAX_)                                                            \
    do {                                                                               \
        if (has_lik) { if (wconst) FA_PREDICT(LMAX_, true, true); else FA_PREDICT(LMAX_, true, false); }   \
        else { if (wconst) FA_PREDICT(LMAX_, false, true); else FA_PREDICT(LMAX_, false, false); }         \
    } while (0)
    if (a.L <= 4) FA_PREDICT_L(4); else FA_PREDICT_L(8);
#undef FA_PREDICT_L
#undef FA_PREDICT
    MFGM_CHECK_LAUNCH();
    return 0;
}

int mfgm_fa_site_update(const mfgm_fa_data* data, const double* gam1, const double* gam2, double lr, double* nat1, double* nat2,
                        void* stream) {
    return launch_sites<false>(data, gam1, gam2, lr, nat1, nat2, stream);
}

int mfgm_fa_site_update_q(const mfgm_fa_data* data, const double* gam1, const double* gam2, double lr, double* nat1, double* nat2q,
                          void* stream) {
    return launch_sites<true>(data, gam1, gam2, lr, nat1, nat2q, stream);
}

}  // extern "C"
