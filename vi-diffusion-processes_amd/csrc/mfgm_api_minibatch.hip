// Mini-batch sparse CVI: the data pass of one unsorted batch and the CSR offsets of the sorted batch (mfgm_minibatch.h).
#include <climits>
#include <cmath>

#include "mfgm_internal.h"
#include "mfgm_minibatch.h"

using namespace mfgm;

namespace {
template <int NMAX>
int batch_impl(const BatchArgs& a, const KernelTermsDev& kt, unsigned blocks, double* ve_sum, hipStream_t st) {
    hipLaunchKernelGGL((k_sparse_batch<NMAX>), dim3(blocks), dim3(64), 0, st, a, kt);
    MFGM_CHECK_LAUNCH();
    if (ve_sum) {
        // the wavefronts' sums in index order: plane 0 of k_score_sum, one chain
        ScoreDest sd;
        for (int q = 0; q < kScorePlanes; ++q) sd.dst[q] = -1;
        sd.dst[0] = 0;
        hipLaunchKernelGGL(k_score_sum, dim3(1, 1), dim3(256), 0, st, (const double*)a.part, (int)blocks, (int)blocks, sd, ve_sum);
        MFGM_CHECK_LAUNCH();
    }
    return 0;
}

long long batch_blocks(long n) { return ((long long)n + 63) / 64; }
}  // namespace

extern "C" size_t mfgm_sparse_batch_workspace_doubles(long n) {
    return (size_t)std::max(1LL, batch_blocks(std::max(n, 0L)));
}

extern "C" int mfgm_sparse_batch_predict_lik(const mfgm_kernel_terms* terms, int M, const double* z, long n, const double* t,
                                             const double* shift, int kind, double param, double scale, const double* y,
                                             const double* prior_mean, const double* prior_cov, const double* mu, const double* Sig,
                                             const double* Sub, int* idx, double* w, double* c, double* fmu, double* fvar, double* ve,
                                             double* g1, double* g2, double* ve_sum, void* ws, int* info, void* stream) {
    if (!terms || !z || !prior_mean || !prior_cov || !mu || !Sig || !Sub || !info) return 1;
    if (M < 1 || n < 0 || batch_blocks(n) > INT_MAX) return 1;
    if (n > 0 && !t) return 1;
    switch (kind) {
        case 0:
            if (y || ve || g1 || g2 || ve_sum) return 1;
            break;
        case MFGM_LIK_BERNOULLI:
            if (!(param >= 0.0 && param < 0.5)) return 1;
            break;
        case MFGM_LIK_POISSON: case MFGM_LIK_GAUSSIAN:
            if (!(param > 0.0 && param < HUGE_VAL)) return 1;
            break;
        default: return 1;
    }
    if (!(scale > 0.0 && scale < HUGE_VAL)) return 1;
    if (kind != 0 && n > 0 && !y) return 1;
    if (ve_sum && !ws) return 1;
    KernelTermsDev kt;
    int src[8][3] = {};
    int d = 0;
    if (device_terms(*terms, kt, src, d)) return 1;      // d > 8 included
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (ve_sum && hipMemsetAsync(ve_sum, 0, sizeof(double), st) != hipSuccess) return 3;
        return 0;
    }
    BatchArgs a;
    a.M = M; a.d = d; a.n = n;
    a.z = z; a.t = t; a.shift = shift; a.y = y; a.prior_mean = prior_mean; a.prior_cov = prior_cov; a.mu = mu; a.Sig = Sig; a.Sub = Sub;
    a.idx = idx; a.w = w; a.c = c; a.fmu = fmu; a.fvar = fvar; a.ve = ve; a.g1 = g1; a.g2 = g2;
    a.part = ve_sum ? (double*)ws : nullptr;
    a.info = info;
    a.kind = kind; a.param = param; a.scale = scale; a.jitter = kt.jitter;
    const unsigned blocks = (unsigned)batch_blocks(n);
    // the instantiation follows the largest term block, as k_sparse_cond_score's
    static const int block_of[7] = {1, 2, 3, 4, 6, 6, 8};      // KT_SHAPE_1, _2, _3, _22, _23, _32, _222
    int nmax = 1;
    for (int q = 0; q < kt.nterm; ++q) nmax = std::max(nmax, block_of[kt.shape[q]]);
    switch (nmax) {
        case 1: return batch_impl<1>(a, kt, blocks, ve_sum, st);
        case 2: return batch_impl<2>(a, kt, blocks, ve_sum, st);
        case 3: return batch_impl<3>(a, kt, blocks, ve_sum, st);
        case 4: return batch_impl<4>(a, kt, blocks, ve_sum, st);
        case 6: return batch_impl<6>(a, kt, blocks, ve_sum, st);
        default: return batch_impl<8>(a, kt, blocks, ve_sum, st);
    }
}

extern "C" int mfgm_sparse_batch_seg(int M, const double* z, long n, const double* t_sorted, int* seg, void* stream) {
    if (!z || !seg || M < 1 || n < 0 || n > INT_MAX) return 1;
    if (n > 0 && !t_sorted) return 1;
    hipLaunchKernelGGL(k_batch_seg, dim3((unsigned)((M + 2 + 63) / 64)), dim3(64), 0, (hipStream_t)stream, M, z, (int)n, t_sorted, seg);
    MFGM_CHECK_LAUNCH();
    return 0;
}
