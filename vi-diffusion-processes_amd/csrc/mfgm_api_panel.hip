// C-ABI entry points of the panel sparse CVI local kernels (mfgm_panel.h).
#include <cmath>

#include "mfgm_internal.h"
#include "mfgm_panel.h"

using namespace mfgm;

namespace {
bool panel_ok(const mfgm_panel_data* s) {
    return s && s->B >= 1 && s->M >= 1 && s->N >= 0 && s->d >= 1 && s->d <= 8;
}
PanelArgs panel_args(const mfgm_panel_data* s) {
    PanelArgs a;
    a.B = s->B; a.M = s->M; a.d = s->d; a.N = s->N;
    a.idx = s->idx; a.seg = s->seg; a.w = s->w; a.c = s->c; a.prior_mean = s->prior_mean; a.prior_cov = s->prior_cov;
    return a;
}
bool narrow_plan(const mfgm_plan* plan) { return plan && !plan->p.wide && plan->p.d >= 1 && plan->p.d <= 8; }
// the ranges of mfgm_scalar_lik / mfgm_pep_sites
bool lik_ok(int kind, double param) {
    switch (kind) {
        case 0: return true;
        case MFGM_LIK_BERNOULLI: return param >= 0.0 && param < 0.5;
        case MFGM_LIK_POISSON: case MFGM_LIK_GAUSSIAN: return param > 0.0 && param < HUGE_VAL;
        default: return false;
    }
}

template <int D>
int launch_theta(const Plan& P, const double* nat1, const double* nat2, const double* plin, const double* pdiag, const double* psub,
                 double* lin, double* diag, double* sub, hipStream_t st) {
    const LevelDesc& lv = P.lv[0];
    const long long blocks = (long long)(lv.Lpad / 64) * lv.R;
    if (blocks > 0x7fffffffLL) return 1;
    hipLaunchKernelGGL(k_panel_theta<D>, dim3((unsigned)blocks), dim3(256), 0, st, lv, P.T, nat1, nat2, plin, pdiag, psub, lin, diag, sub);
    MFGM_CHECK_LAUNCH();
    return 0;
}

template <int D>
int launch_predict(const PanelArgs& a, const LevelDesc& lv, int kind, double param, const double* y, const double* x, const double* Sig,
                   const double* Sub, double* fmu, double* fvar, double* ve, double* g1, double* g2, double* ve_series, hipStream_t st) {
    // one workgroup per series: as many wavefronts as the row has points for, at most four
    const dim3 grid(a.B), block(a.N <= 64 ? 64 : (a.N <= 128 ? 128 : 256));
#define PANEL_PREDICT(KIND_) \
    hipLaunchKernelGGL((k_panel_predict<D, KIND_>), grid, block, 0, st, a, lv, param, y, x, Sig, Sub, fmu, fvar, ve, g1, g2, ve_series)
    if (kind == 0) PANEL_PREDICT(0);
    else if (kind == MFGM_LIK_BERNOULLI) PANEL_PREDICT(1);
    else if (kind == MFGM_LIK_POISSON) PANEL_PREDICT(2);
    else PANEL_PREDICT(kPanelGaussian);
#undef PANEL_PREDICT
    MFGM_CHECK_LAUNCH();
    return 0;
}

template <int D>
int launch_sites(const PanelArgs& a, const double* g1, const double* g2, double lr, double* nat1, double* nat2, hipStream_t st) {
    const size_t blocks = ((size_t)a.B * (a.M + 1) * 2 * D + 255) / 256;
    if (blocks > 0x7fffffffu) return 1;
    hipLaunchKernelGGL(k_panel_sites<D>, dim3((unsigned)blocks), dim3(256), 0, st, a, g1, g2, lr, nat1, nat2);
    MFGM_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" {

int mfgm_panel_theta(const mfgm_plan* plan, const double* nat1, const double* nat2, const double* plin, const double* pdiag,
                     const double* psub, double* lin, double* diag, double* sub, void* stream) {
    if (!narrow_plan(plan) || !nat1 || !nat2 || !pdiag || !psub || !lin || !diag || !sub) return 1;
    const Plan& P = plan->p;
    MFGM_DISPATCH_D(P.d, launch_theta<DD>(P, nat1, nat2, plin, pdiag, psub, lin, diag, sub, (hipStream_t)stream));
}

int mfgm_panel_predict_lik(const mfgm_plan* plan, const mfgm_panel_data* data, int kind, double param, const double* y, const double* x,
                           const double* Sig, const double* Sub, double* fmu, double* fvar, double* ve, double* g1, double* g2,
                           double* ve_series, void* stream) {
    if (!panel_ok(data) || !narrow_plan(plan) || !lik_ok(kind, param)) return 1;
    const Plan& P = plan->p;
    if (P.B != data->B || P.T != data->M || P.d != data->d) return 1;
    if (kind == 0 && (y || ve || g1 || g2 || ve_series)) return 1;
    if (data->N > 0 && (!data->idx || !data->w || !data->c || !data->prior_mean || !data->prior_cov || !x || !Sig || (data->M > 1 && !Sub) ||
                        (kind != 0 && !y)))
        return 1;
    if (data->N == 0 && !ve_series) return 0;          // nothing to write (an empty row sums to 0 in ve_series)
    const PanelArgs a = panel_args(data);
    MFGM_DISPATCH_D(a.d, launch_predict<DD>(a, P.lv[0], kind, param, y, x, Sig, Sub, fmu, fvar, ve, g1, g2, ve_series, (hipStream_t)stream));
}

int mfgm_panel_site_update(const mfgm_panel_data* data, const double* g1, const double* g2, double lr, double* nat1, double* nat2,
                           void* stream) {
    if (!panel_ok(data) || !nat1 || !nat2 || !(lr >= 0.0 && lr <= 1.0)) return 1;
    if (data->N > 0 && (!data->seg || !data->w || !g1 || !g2)) return 1;
    const PanelArgs a = panel_args(data);
    MFGM_DISPATCH_D(a.d, launch_sites<DD>(a, g1, g2, lr, nat1, nat2, (hipStream_t)stream));
}

}  // extern "C"
