// Simulation of the SDE priors (mfgm_sim.h): the counter-based normal stream and Euler-Maruyama (markovflow/sde/sde_utils.py:36-96).
#include "mfgm_internal.h"
#include "mfgm_sim.h"

using namespace mfgm;

namespace {
bool sim_ok(const mfgm_quad_drift* q) {
    if (!q || q->d < 1 || q->d > kSimD) return false;
    if (q->kind == 10) return q->d == 2;
    if (q->kind == 11) return q->nh >= 1 && 3 * q->nh + 1 <= MFGM_QUAD_NTHETA;
    return q->kind >= 12 && q->kind <= 15;
}

// rows staged per lane before a flush (MFGM_EM_STAGE, clamped to kSimStageW doubles per path); default 0: per-lane row stores.  The
// kernel is issue-bound (about 370 instructions per step and pair of normals), at under a tenth of the bytes-written bound,
// and staging 8 .. 64 rows measured 10 - 13 % slower on 65 536 paths x 1 001 steps (tools/em_rate.py --stage-ab)
int stage_rows(int d) {
    static const int env = [] { const char* e = getenv("MFGM_EM_STAGE"); return e ? std::max(0, atoi(e)) : 0; }();
    return std::min(env, kSimStageW / d);
}

template <int D, int KIND>
int launch_em(const mfgm_quad_drift& q, const sim_chol& lc, int B, int N, const double* x0, const double* tg, unsigned long long seed,
              double* X, hipStream_t st) {
    const int S = stage_rows(D);
    const size_t lds = S ? (size_t)kSimLanes * ((S * D) | 1) * sizeof(double) : 0;
    hipLaunchKernelGGL((k_euler_maruyama<D, KIND>), dim3((B + kSimLanes - 1) / kSimLanes), dim3(kSimLanes), lds, st, q, lc, B, N, x0, tg,
                       seed, S, X);
    MFGM_CHECK_LAUNCH();
    return 0;
}

template <int D>
int em_kind(const mfgm_quad_drift& q, const sim_chol& lc, int B, int N, const double* x0, const double* tg, unsigned long long seed,
            double* X, hipStream_t st) {
    switch (q.kind) {
        case 10:
            if constexpr (D == 2) return launch_em<2, 10>(q, lc, B, N, x0, tg, seed, X, st);
            return 1;
        case 11: return launch_em<D, 11>(q, lc, B, N, x0, tg, seed, X, st);
        case 12: return launch_em<D, 12>(q, lc, B, N, x0, tg, seed, X, st);
        case 13: return launch_em<D, 13>(q, lc, B, N, x0, tg, seed, X, st);
        case 14: return launch_em<D, 14>(q, lc, B, N, x0, tg, seed, X, st);
        case 15: return launch_em<D, 15>(q, lc, B, N, x0, tg, seed, X, st);
        default: return 1;
    }
}
}  // namespace

extern "C" {

int mfgm_normal_fill(unsigned long long seed, unsigned int s, int P, int K, int d, double* out, void* stream) {
    if (P < 0 || K < 0 || d < 1 || (!out && P > 0 && K > 0)) return 1;
    const size_t total = (size_t)P * K * ((d + 1) / 2);
    if (total == 0) return 0;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(k_normal_fill, dim3(blocks), dim3(256), 0, (hipStream_t)stream, seed, s, P, K, d, out);
    MFGM_CHECK_LAUNCH();
    return 0;
}

int mfgm_euler_maruyama(const mfgm_quad_drift* drift, int B, int N, const double* x0, const double* time_grid, const double* L,
                        unsigned long long seed, double* X, void* stream) {
    if (!sim_ok(drift) || B < 1 || N < 1 || !x0 || !time_grid || !L || !X) return 1;
    const int d = drift->d;
    sim_chol lc{};
    for (int r = 0; r < d; ++r)
        for (int j = 0; j <= r; ++j) lc.L[r * (r + 1) / 2 + j] = L[r * d + j];
    MFGM_DISPATCH_D(d, (em_kind<DD>(*drift, lc, B, N, x0, time_grid, seed, X, (hipStream_t)stream)));
}

}  // extern "C"
