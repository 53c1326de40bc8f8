// Impulse and step mean functions of a driven kernel SDE: the coefficient scan and the evaluation at query points (mfgm_mean.h).
#include "mfgm_internal.h"
#include "mfgm_mean.h"

#include <climits>

using namespace mfgm;

namespace {
// The segment length of the scan: the caller's, or the smallest s with s * s >= K (the serial parts of the scan are the seg steps of a
// segment lane and the K / seg steps of the walk over the segment ends; their sum is smallest there).  A rule in K alone.
int action_seg(int K, int seg_len) {
    if (seg_len > 0) return seg_len;
    int s = 1;
    while ((long long)s * s < K) ++s;
    return s;
}

int action_segments(int K, int seg) { return (int)(((long long)K + seg - 1) / seg); }

template <int D>
int action_coefficients_impl(const KernelTermsDev& kt, int B, int K, int seg, const double* times, const double* rhs, double* coef,
                             double* ends, hipStream_t st) {
    const int S = action_segments(K, seg);
    const long long l0 = (long long)B * S;
    hipLaunchKernelGGL((k_action_local<D>), dim3((unsigned)((l0 + 63) / 64)), dim3(64), 0, st, kt, B, K, seg, S, times, rhs, coef, ends);
    MFGM_CHECK_LAUNCH();
    if (S == 1) return 0;
    hipLaunchKernelGGL((k_action_ends<D>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, kt, B, K, seg, S, times, ends);
    MFGM_CHECK_LAUNCH();
    const long long l2 = (long long)B * (K - seg);
    hipLaunchKernelGGL((k_action_apply<D>), dim3((unsigned)((l2 + 63) / 64)), dim3(64), 0, st, kt, B, K, seg, S, times,
                       (const double*)ends, coef);
    MFGM_CHECK_LAUNCH();
    return 0;
}

template <int D>
int action_mean_impl(const KernelTermsDev& kt, const ActionMeanArgs& a, hipStream_t st) {
    const long long lanes = (long long)a.B * a.N;
    hipLaunchKernelGGL((k_action_mean<D>), dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, kt, a);
    MFGM_CHECK_LAUNCH();
    return 0;
}

// terms -> the kernels' form and the state dimension; mean and jitter play no part
int action_terms(const mfgm_kernel_terms* terms, KernelTermsDev& kt, int& d) {
    if (!terms) return 1;
    int src[8][3] = {};
    if (device_terms(*terms, kt, src, d)) return 1;
    for (int i = 0; i < 8; ++i) kt.mean[i] = 0.0;
    kt.jitter = 0.0;
    return 0;
}
}  // namespace

extern "C" size_t mfgm_action_workspace_doubles(int B, int K, int d, int seg_len) {
    if (B < 1 || K < 1 || d < 1 || d > 8 || seg_len < 0) return 0;
    return (size_t)B * action_segments(K, action_seg(K, seg_len)) * d;
}

extern "C" int mfgm_action_coefficients(const mfgm_kernel_terms* terms, int B, int K, int seg_len, const double* action_times,
                                        const double* rhs, double* coef, void* ws, void* stream) {
    if (!terms || !action_times || !rhs || !coef || !ws) return 1;
    if (B < 1 || K < 1 || seg_len < 0) return 1;
    KernelTermsDev kt;
    int d = 0;
    if (action_terms(terms, kt, d)) return 1;
    const int seg = action_seg(K, seg_len);
    if (((long long)B * K + 63) / 64 > INT_MAX) return 1;
    hipStream_t st = (hipStream_t)stream;
    MFGM_DISPATCH_D(d, (action_coefficients_impl<DD>(kt, B, K, seg, action_times, rhs, coef, (double*)ws, st)));
}

extern "C" int mfgm_action_mean(const mfgm_kernel_terms* terms, int B, int K, long N, const double* action_times, const double* coef,
                                const double* shift, const double* time_points, const double* emission, double* state_mean,
                                double* f_mean, void* stream) {
    if (!terms || !action_times || !coef) return 1;
    if (B < 1 || K < 1 || N < 0) return 1;
    if (N > 0 && !time_points) return 1;
    if (f_mean && !emission) return 1;
    KernelTermsDev kt;
    int d = 0;
    if (action_terms(terms, kt, d)) return 1;
    if (((long long)B * N + 63) / 64 > INT_MAX) return 1;
    if (N == 0 || (!state_mean && !f_mean)) return 0;
    ActionMeanArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B;
    a.K = K;
    a.N = N;
    a.times = action_times;
    a.coef = coef;
    a.shift = shift;
    a.tps = time_points;
    a.state_mean = state_mean;
    a.f_mean = f_mean;
    if (emission)
        for (int i = 0; i < d; ++i) a.emission[i] = emission[i];
    hipStream_t st = (hipStream_t)stream;
    MFGM_DISPATCH_D(d, (action_mean_impl<DD>(kt, a, st)));
}
