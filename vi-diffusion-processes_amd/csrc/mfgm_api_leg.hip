// Latent exponentially generated kernels -> SSM parameters: the packed prior of a time grid and (A, Q) of arbitrary gaps
// (mfgm_leg_ssm.h).
#include <cmath>

#include "mfgm_internal.h"
#include "mfgm_leg_ssm.h"

using namespace mfgm;

namespace {
template <int D>
int leg_ssm_impl(const Plan& P, const LegDev& lg, const double* dts, double* A, double* off, double* chol, int* info, hipStream_t st) {
    const LevelDesc& lv = P.lv[0];
    hipLaunchKernelGGL((k_leg_ssm<D>), dim3(lv.Lpad / 64), dim3(64), 0, st, lv, lg, dts, A, off, chol, info);
    MFGM_CHECK_LAUNCH();
    return 0;
}

template <int D>
int leg_transitions_impl(const LegDev& lg, long n, const double* dts, double* A, double* Q, hipStream_t st) {
    hipLaunchKernelGGL((k_leg_transitions<D>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, lg, n, dts, A, Q);
    MFGM_CHECK_LAUNCH();
    return 0;
}

// the caller's spec -> the kernels' argument; 0, or 1 for a spec the kernels do not take
int device_spec(const mfgm_leg_spec* in, LegDev& lg) {
    if (!in || in->d < 1 || in->d > 8) return 1;
    const int d = in->d;
    memset(&lg, 0, sizeof(lg));
    for (int e = 0; e < d * d; ++e) lg.F[e] = in->F[e];
    for (int i = 0; i < d; ++i) lg.mean[i] = in->mean[i];
    lg.jitter = in->jitter;
    for (int j = 0; j < d; ++j) {
        double c = 0.0;
        for (int i = 0; i < d; ++i) c += std::fabs(in->F[i * d + j]);
        lg.norm1 = std::max(lg.norm1, c);
    }
    return 0;
}
}  // namespace

extern "C" int mfgm_packed_leg_ssm(const mfgm_plan* plan, const mfgm_leg_spec* spec, const double* time_deltas, double* A,
                                   double* off, double* chol, int* info, void* stream) {
    if (!plan || !A || !off || !chol || !info) return 1;
    LegDev lg;
    if (device_spec(spec, lg)) return 1;
    const Plan& P = plan->p;
    if (P.wide || P.d != spec->d) return 1;
    if (P.T > 1 && !time_deltas) return 1;
    hipStream_t st = (hipStream_t)stream;
    MFGM_DISPATCH_D(P.d, (leg_ssm_impl<DD>(P, lg, time_deltas, A, off, chol, info, st)));
}

extern "C" int mfgm_leg_transitions(const mfgm_leg_spec* spec, long n, const double* time_deltas, double* A, double* Q,
                                    void* stream) {
    LegDev lg;
    if (device_spec(spec, lg) || n < 0 || n > 64L * 0x7fffffffL) return 1;
    if (n == 0) return 0;
    if (!time_deltas || !A || !Q) return 1;
    hipStream_t st = (hipStream_t)stream;
    MFGM_DISPATCH_D(spec->d, (leg_transitions_impl<DD>(lg, n, time_deltas, A, Q, st)));
}
