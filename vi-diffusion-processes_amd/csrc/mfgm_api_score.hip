// Log-likelihood score of the kernel terms from the posterior pairwise moments (mfgm_score.h).
#include "mfgm_internal.h"
#include "mfgm_score.h"

using namespace mfgm;

namespace {
template <int NMAX>
int kernel_score_impl(const Plan& P, const ScoreArgs& a, const KernelTermsDev& kt, const ScoreDest& sd, double* score, hipStream_t st) {
    const LevelDesc& lv = P.lv[0];
    if (hipMemsetAsync(score, 0, (size_t)P.B * kScorePlanes * sizeof(double), st) != hipSuccess) return 3;
    hipLaunchKernelGGL((k_kernel_score<NMAX>), dim3(lv.Lpad / 64), dim3(64), 0, st, a, kt);
    MFGM_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_score_sum, dim3(P.B, 6 * kt.nterm), dim3(256), 0, st, (const double*)a.part, lv.P, lv.Lpad, sd, score);
    MFGM_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" int mfgm_packed_kernel_score(const mfgm_plan* plan, const mfgm_kernel_terms* terms, const double* time_deltas,
                                        const double* x, const double* Sig, const double* Sub, double* score, void* ws, int* info,
                                        void* stream) {
    if (!plan || !terms || !x || !Sig || !score || !ws || !info) return 1;
    const Plan& P = plan->p;
    if (P.T > 1 && (!time_deltas || !Sub)) return 1;
    KernelTermsDev kt;
    int src[8][3] = {};
    if (device_terms(P, *terms, kt, src)) return 1;
    ScoreDest sd;
    for (int q = 0; q < kScorePlanes; ++q) sd.dst[q] = -1;
    bool allexact = (kt.jitter == 0.0);
    for (int c = 0; c < kt.nterm; ++c)
        for (int f = 0; f < 3; ++f) {
            if (kt.kind[c][f] == 0) continue;
            allexact = allexact && (kt.kind[c][f] == MFGM_FACTOR_CONSTANT || kt.kind[c][f] == MFGM_FACTOR_HARMONIC);
            for (int j = 0; j < 2; ++j) sd.dst[6 * c + 2 * f + j] = 6 * c + 2 * src[c][f] + j;
        }
    ScoreArgs a;
    a.lv = P.lv[0];
    a.dts = time_deltas;
    a.x = x;
    a.Sig = Sig;
    a.Sub = Sub;
    a.part = (double*)ws + P.off_part[0];
    a.info = info;
    a.jitter = kt.jitter;
    a.allexact = allexact ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    a.d = P.d;
    // the instantiation follows the largest term block, not the plan's d
    static const int block_of[7] = {1, 2, 3, 4, 6, 6, 8};      // KT_SHAPE_1, _2, _3, _22, _23, _32, _222
    int nmax = 1;
    for (int c = 0; c < kt.nterm; ++c) nmax = std::max(nmax, block_of[kt.shape[c]]);
    switch (nmax) {
        case 1: return kernel_score_impl<1>(P, a, kt, sd, score, st);
        case 2: return kernel_score_impl<2>(P, a, kt, sd, score, st);
        case 3: return kernel_score_impl<3>(P, a, kt, sd, score, st);
        case 4: return kernel_score_impl<4>(P, a, kt, sd, score, st);
        case 6: return kernel_score_impl<6>(P, a, kt, sd, score, st);
        default: return kernel_score_impl<8>(P, a, kt, sd, score, st);
    }
}
