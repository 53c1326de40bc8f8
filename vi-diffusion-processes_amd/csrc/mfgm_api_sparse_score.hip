// Kernel score of the sparse-CVI bound through the conditionals of the data points (mfgm_sparse_score.h).
#include "mfgm_internal.h"
#include "mfgm_sparse_score.h"

using namespace mfgm;

namespace {
template <int NMAX>
int cond_score_impl(const CondScoreArgs& a, const KernelTermsDev& kt, const ScoreDest& sd, double* score, hipStream_t st) {
    hipLaunchKernelGGL((k_sparse_cond_score<NMAX>), dim3(a.nblk), dim3(64), 0, st, a, kt);
    MFGM_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_score_sum, dim3(1, 6 * kt.nterm), dim3(256), 0, st, (const double*)a.part, a.nblk, a.nblk, sd, score);
    MFGM_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" size_t mfgm_sparse_cond_score_workspace_doubles(int N) {
    return (size_t)kScorePlanes * (size_t)std::max(1, ceil_div(std::max(N, 1), 64));
}

extern "C" int mfgm_sparse_cond_score(const mfgm_sparse_data* data, const mfgm_kernel_terms* terms, const double* gap_lo,
                                      const double* gap_hi, const double* a, const double* b, const double* mu, const double* Sig,
                                      const double* Sub, double* score, void* ws, int* info, void* stream) {
    if (!data || !terms || !mu || !Sig || !Sub || !score || !ws || !info) return 1;
    if (data->M < 1 || data->d < 1 || data->d > 8 || data->N < 0 || data->m_hi > 0 || !data->seg || !data->prior_mean || !data->prior_cov)
        return 1;
    if (data->N > 0 && (!data->w || !data->c || !gap_lo || !gap_hi || !a || !b)) return 1;
    // device_terms reads the plan's block size alone
    Plan P{};
    P.d = data->d;
    P.wide = 0;
    KernelTermsDev kt;
    int src[8][3] = {};
    if (device_terms(P, *terms, kt, src)) return 1;
    ScoreDest sd;
    for (int q = 0; q < kScorePlanes; ++q) sd.dst[q] = -1;
    for (int c = 0; c < kt.nterm; ++c)
        for (int f = 0; f < 3; ++f) {
            if (kt.kind[c][f] == 0) continue;
            for (int j = 0; j < 2; ++j) sd.dst[6 * c + 2 * f + j] = 6 * c + 2 * src[c][f] + j;
        }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(score, 0, (size_t)kScorePlanes * sizeof(double), st) != hipSuccess) return 3;
    if (data->N == 0) return 0;
    CondScoreArgs ca;
    ca.sp.M = data->M; ca.sp.d = data->d; ca.sp.N = data->N; ca.sp.m_lo = 0; ca.sp.m_hi = data->M + 1;
    ca.sp.seg = data->seg; ca.sp.w = data->w; ca.sp.c = data->c; ca.sp.prior_mean = data->prior_mean; ca.sp.prior_cov = data->prior_cov;
    ca.gap_lo = gap_lo; ca.gap_hi = gap_hi; ca.a = a; ca.b = b; ca.mu = mu; ca.Sig = Sig; ca.Sub = Sub;
    ca.part = (double*)ws;
    ca.info = info;
    ca.jitter = kt.jitter;
    ca.nblk = ceil_div(data->N, 64);
    // the instantiation follows the largest term block, as k_kernel_score's
    static const int block_of[7] = {1, 2, 3, 4, 6, 6, 8};      // KT_SHAPE_1, _2, _3, _22, _23, _32, _222
    int nmax = 1;
    for (int c = 0; c < kt.nterm; ++c) nmax = std::max(nmax, block_of[kt.shape[c]]);
    switch (nmax) {
        case 1: return cond_score_impl<1>(ca, kt, sd, score, st);
        case 2: return cond_score_impl<2>(ca, kt, sd, score, st);
        case 3: return cond_score_impl<3>(ca, kt, sd, score, st);
        case 4: return cond_score_impl<4>(ca, kt, sd, score, st);
        case 6: return cond_score_impl<6>(ca, kt, sd, score, st);
        default: return cond_score_impl<8>(ca, kt, sd, score, st);
    }
}
