// Kernel score of the panel's sparse-CVI bound through the conditionals of its data points (mfgm_panel_score.h).
#include "mfgm_internal.h"
#include "mfgm_panel_score.h"

using namespace mfgm;

namespace {
size_t panel_score_blocks(int B, int N) { return ((size_t)std::max(B, 0) * (size_t)std::max(N, 0) + 63) / 64; }

template <int NMAX>
int panel_score_impl(const PanelScoreArgs& a, const LevelDesc& lv, const KernelTermsDev& kt, const ScoreDest& sd, double* score,
                     hipStream_t st) {
    hipLaunchKernelGGL((k_panel_cond_score<NMAX>), dim3(a.nblk), dim3(64), 0, st, a, lv, kt);
    MFGM_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_score_sum, dim3(1, 6 * kt.nterm), dim3(256), 0, st, (const double*)a.part, a.nblk, a.nblk, sd, score);
    MFGM_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" size_t mfgm_panel_cond_score_workspace_doubles(int B, int N) {
    return (size_t)kScorePlanes * std::max<size_t>(1, panel_score_blocks(B, N));
}

extern "C" int mfgm_panel_cond_score(const mfgm_plan* plan, const mfgm_panel_data* data, const mfgm_kernel_terms* terms,
                                     const double* gap_lo, const double* gap_hi, const double* a, const double* b, const double* x,
                                     const double* Sig, const double* Sub, double* score, void* ws, int* info, void* stream) {
    if (!plan || !data || !terms || !score) return 1;
    if (data->B < 1 || data->M < 1 || data->N < 0 || data->d < 1 || data->d > 8) return 1;
    const Plan& P = plan->p;
    if (P.wide || P.B != data->B || P.T != data->M || P.d != data->d) return 1;
    const size_t nblk = panel_score_blocks(data->B, data->N);
    if (nblk > 0x7fffffffu) return 1;
    if (nblk > 0 && (!data->idx || !data->w || !data->prior_mean || !data->prior_cov || !gap_lo || !gap_hi || !a || !b || !x || !Sig ||
                     (data->M > 1 && !Sub) || !ws || !info))
        return 1;
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
    if (nblk == 0) return 0;
    PanelScoreArgs pa;
    pa.sp.B = data->B; pa.sp.M = data->M; pa.sp.d = data->d; pa.sp.N = data->N;
    pa.sp.idx = data->idx; pa.sp.seg = data->seg; pa.sp.w = data->w; pa.sp.c = data->c;
    pa.sp.prior_mean = data->prior_mean; pa.sp.prior_cov = data->prior_cov;
    pa.gap_lo = gap_lo; pa.gap_hi = gap_hi; pa.a = a; pa.b = b; pa.x = x; pa.Sig = Sig; pa.Sub = Sub;
    pa.part = (double*)ws;
    pa.info = info;
    pa.jitter = kt.jitter;
    pa.nblk = (int)nblk;
    // the instantiation follows the largest term block, as k_sparse_cond_score's
    static const int block_of[7] = {1, 2, 3, 4, 6, 6, 8};      // KT_SHAPE_1, _2, _3, _22, _23, _32, _222
    int nmax = 1;
    for (int c = 0; c < kt.nterm; ++c) nmax = std::max(nmax, block_of[kt.shape[c]]);
    const LevelDesc& lv = P.lv[0];
    switch (nmax) {
        case 1: return panel_score_impl<1>(pa, lv, kt, sd, score, st);
        case 2: return panel_score_impl<2>(pa, lv, kt, sd, score, st);
        case 3: return panel_score_impl<3>(pa, lv, kt, sd, score, st);
        case 4: return panel_score_impl<4>(pa, lv, kt, sd, score, st);
        case 6: return panel_score_impl<6>(pa, lv, kt, sd, score, st);
        default: return panel_score_impl<8>(pa, lv, kt, sd, score, st);
    }
}
