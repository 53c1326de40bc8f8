// C-ABI entry points of the multi-latent sparse CVI local kernels (mfgm_ml.h).
#include "mfgm_internal.h"
#include "mfgm_ml.h"

using namespace mfgm;

namespace {
// L in 1 .. 8, every dl >= 1, D = sum dl in 2 .. 32 (each dl is bounded first, so the sum cannot overflow); the arrays over data
// points present when there is a data point
bool ml_ok(const mfgm_ml_data* s) {
    if (!s || s->M < 1 || s->N < 0 || s->L < 1 || s->L > kMlMaxL) return false;
    int D = 0;
    for (int l = 0; l < s->L; ++l) {
        if (s->dl[l] < 1 || s->dl[l] > 32) return false;
        D += s->dl[l];
    }
    if (D < 2 || D > 32) return false;
    return s->seg && (s->N == 0 || (s->h && s->c));
}
MlArgs ml_args(const mfgm_ml_data* s) {
    MlArgs a;
    memset(&a, 0, sizeof(a));
    a.M = s->M; a.L = s->L; a.N = s->N;
    int D = 0;
    for (int l = 0; l < s->L; ++l) {
        a.dl[l] = s->dl[l];
        a.off[l] = D;
        D += s->dl[l];
    }
    a.D = D;
    a.seg = s->seg; a.h = s->h; a.c = s->c; a.prior_mean = s->prior_mean; a.prior_cov = s->prior_cov;
    return a;
}
bool lik_ok(const mfgm_ml_data* s, const mfgm_ml_lik* lik) {
    if (!lik) return false;
    switch (lik->kind) {
        case MFGM_ML_NONE: return true;
        case MFGM_ML_MULTISTAGE:
            return s->L == 3 && lik->param[0] >= 0.0 && lik->param[0] < 0.5 && lik->param[1] > 0.0 && lik->param[1] < HUGE_VAL;
        case MFGM_ML_HETGAUSS: return s->L == 2;
        default: return false;
    }
}

template <bool PACKED>
int launch_sites(const mfgm_ml_data* data, const double* g1, const double* g2, double lr, double* nat1, double* nat2, void* stream) {
    if (!ml_ok(data) || !nat1 || !nat2 || !(lr >= 0.0 && lr <= 1.0) || (data->N > 0 && (!g1 || !g2))) return 1;
    const MlArgs a = ml_args(data);
    const int D = a.D, QS = PACKED ? D * (D + 1) + D * D : 4 * D * D;
    const size_t shmem = sizeof(double) * kMlSitesChunk * (2 * D + 2 * a.L) + sizeof(int) * 2 * D;
    const int ne = (QS + 255) / 256;
#define ML_SITES(NE_) hipLaunchKernelGGL((k_ml_sites<NE_, PACKED>), dim3(a.M + 1), dim3(256), shmem, (hipStream_t)stream, a, g1, g2, lr, nat1, nat2)
    if (ne <= 1) ML_SITES(1); else if (ne <= 2) ML_SITES(2); else if (ne <= 4) ML_SITES(4); else if (ne <= 6) ML_SITES(6);
    else if (ne <= 9) ML_SITES(9); else if (ne <= 12) ML_SITES(12); else if (ne <= 16) ML_SITES(16); else return 1;
#undef ML_SITES
    MFGM_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" {

int mfgm_ml_predict_lik(const mfgm_ml_data* data, const mfgm_ml_lik* lik, const double* y, const double* mu, const double* Sig,
                        const double* Sub, double* fmu, double* fvar, double* ve_part, double* g1, double* g2, void* stream) {
    if (!ml_ok(data) || !lik_ok(data, lik)) return 1;
    if (lik->kind == MFGM_ML_NONE && (y || ve_part || g1 || g2)) return 1;
    if (data->N > 0 && (!mu || !Sig || !Sub || !data->prior_mean || !data->prior_cov || (lik->kind != MFGM_ML_NONE && !y))) return 1;
    if (lik->kind == MFGM_ML_NONE && data->N == 0) return 0;
    const MlArgs a = ml_args(data);
    const MlLik lk{lik->kind, lik->param[0], lik->param[1]};
    int nblk = 0;
    for (int l = 0; l < a.L; ++l) nblk += a.dl[l] * a.dl[l];
    // intervals per wavefront: about 64 data points' worth of them, as many as ~40 KB of LDS hold, at most kMlMaxGroup, at least 1
    const size_t fixed = sizeof(double) * ((size_t)kMlChunk * (2 * a.D + 1) + kMlChunk + nblk + a.D) + sizeof(int);
    const size_t per_g = sizeof(double) * ((size_t)2 * nblk + a.D) + sizeof(int);
    const long long want = ((long long)kMlChunk * (a.M + 1) + std::max(a.N, 1) - 1) / std::max(a.N, 1);
    long long fit = fixed < 40960 ? (long long)((40960 - fixed) / per_g) : 0;
    const int G = (int)std::max(1LL, std::min({want, fit, (long long)kMlMaxGroup}));
    const size_t shmem = fixed + (size_t)G * per_g;
    if (shmem > 65536) return 1;
    const dim3 grid((a.M + 1 + G - 1) / G);
#define ML_PREDICT(KIND_)                                                                                                          \
    hipLaunchKernelGGL((k_ml_predict_lik<KIND_>), grid, dim3(64), shmem, (hipStream_t)stream, a, lk, G, y, mu, Sig, Sub, fmu, fvar, \
                       ve_part, g1, g2)
    if (lik->kind == MFGM_ML_NONE) ML_PREDICT(0); else if (lik->kind == MFGM_ML_MULTISTAGE) ML_PREDICT(1); else ML_PREDICT(2);
#undef ML_PREDICT
    MFGM_CHECK_LAUNCH();
    return 0;
}

int mfgm_ml_site_update(const mfgm_ml_data* data, const double* g1, const double* g2, double lr, double* nat1, double* nat2, void* stream) {
    return launch_sites<false>(data, g1, g2, lr, nat1, nat2, stream);
}

int mfgm_ml_site_update_q(const mfgm_ml_data* data, const double* g1, const double* g2, double lr, double* nat1, double* nat2q,
                          void* stream) {
    return launch_sites<true>(data, g1, g2, lr, nat1, nat2q, stream);
}

}  // extern "C"
