// Seeded draws x = L^{-T} (y + eps) from a form-0 factorisation (mfgm_sample.h), lane-per-segment plans (d <= 8).
#include "mfgm_internal.h"
#include "mfgm_sample.h"

using namespace mfgm;

namespace {
// MFGM_SAMPLE_PACKED=1: the replay writes every sample in the packed VEC layout (coalesced stores) and mfgm_unpack re-lays it out,
// instead of storing the natural [S, B, T, d] rows straight from the lanes (the default; DESIGN.md section 10 has the A/B)
bool packed_out() {
    static const bool env = [] { const char* e = getenv("MFGM_SAMPLE_PACKED"); return e && atoi(e) != 0; }();
    return env;
}

template <int D>
int launch_sample(const mfgm_plan* plan, SmpArgs a, hipStream_t st) {
    constexpr int K = sample_k(D);
    const LevelDesc& lv = a.lv;
    const int groups = ceil_div(a.S, K);
    if (groups > 65535) return 1;
    const dim3 grid(lv.Lpad / 64, groups);
    hipLaunchKernelGGL((k_sample_seg<D, K, true>), grid, dim3(64), 0, st, a);
    MFGM_CHECK_LAUNCH();
    for (int n0 = 0; n0 < a.S; n0 += 65535) {      // one wavefront per (chain, sample); grid.y is capped at 65535
        SmpArgs c = a;
        c.c = a.c + (size_t)n0 * D * lv.Lpad;
        c.xin = a.xin + (size_t)n0 * D * lv.Lpad;
        hipLaunchKernelGGL((k_sample_scan<D>), dim3(a.B, std::min(65535, a.S - n0)), dim3(64), 0, st, c);
        MFGM_CHECK_LAUNCH();
    }
    if (!a.xpk) {
        hipLaunchKernelGGL((k_sample_seg<D, K, false, false>), grid, dim3(64), 0, st, a);
        MFGM_CHECK_LAUNCH();
        return 0;
    }
    double* natural = a.x;
    a.x = a.xin + (size_t)a.S * D * lv.Lpad;       // packed samples after xin in the scratch
    hipLaunchKernelGGL((k_sample_seg<D, K, false, true>), grid, dim3(64), 0, st, a);
    MFGM_CHECK_LAUNCH();
    for (int n = 0; n < a.S; ++n) {
        const int rc = mfgm_unpack(plan, MFGM_VEC, a.x + (size_t)n * a.xpk, natural + (size_t)n * a.B * a.T * D, a.T, st);
        if (rc) return rc;
    }
    return 0;
}
}  // namespace

extern "C" {

size_t mfgm_packed_sample_scratch_doubles(const mfgm_plan* plan, int n_samples) {
    if (!plan || plan->p.wide || n_samples < 0) return 0;
    const Plan& P = plan->p;
    const LevelDesc& lv = P.lv[0];
    const size_t d = P.d, S = n_samples;
    size_t n = (d * d + 2 * S * d) * lv.Lpad;
    if (packed_out()) n += S * level_elems(P, lv, MFGM_VEC);
    return n;
}

int mfgm_packed_sample(const mfgm_plan* plan, const double* L, const double* G, const double* y, int n_samples,
                       unsigned long long seed, unsigned int stream_tag, double* x, double* scratch, void* stream) {
    if (!plan || plan->p.wide || n_samples < 0) return 1;
    const Plan& P = plan->p;
    if ((unsigned long long)P.B * (unsigned long long)P.T >= (1ull << 32)) return 1;
    if (n_samples == 0) return 0;
    if (!L || !G || !y || !x || !scratch) return 1;
    SmpArgs a{};
    a.lv = P.lv[0];
    a.B = P.B;
    a.T = P.T;
    a.S = n_samples;
    a.seed = seed;
    a.tag = stream_tag;
    a.L = L;
    a.G = G;
    a.y = y;
    a.Phi = scratch;
    a.c = a.Phi + (size_t)P.d * P.d * a.lv.Lpad;
    a.xin = a.c + (size_t)n_samples * P.d * a.lv.Lpad;
    a.x = x;
    a.xpk = packed_out() ? level_elems(P, a.lv, MFGM_VEC) : 0;
    MFGM_DISPATCH_D(P.d, (launch_sample<DD>(plan, a, (hipStream_t)stream)));
}

}  // extern "C"
