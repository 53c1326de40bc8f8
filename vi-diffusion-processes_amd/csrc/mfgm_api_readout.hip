// Linear-readout likelihoods of the diffusion models (mfgm_readout.h): the data-site update and the observation-node variational
// expectations, one launch each.
#include "mfgm_internal.h"
#include "mfgm_readout.h"

using namespace mfgm;

static_assert(sizeof(mfgm_readout) == sizeof(mfgm::Readout), "public and internal readout structs must match");

namespace {

// 0 when the descriptor fits the plan and every factor is a known kind with its parameter in range
int readout_check(const mfgm_plan* plan, const mfgm_readout* readout, Readout& rd) {
    if (!plan || !readout) return 1;
    const Plan& P = plan->p;
    if (P.wide || P.d > 8 || (size_t)P.B * P.T >= (1ull << 32)) return 1;
    memcpy(&rd, readout, sizeof(rd));
    if (rd.o < 1 || rd.o > 8 || rd.d != P.d) return 1;
    for (int j = 0; j < rd.o; ++j) {
        const double p = rd.param[j];
        if (rd.kind[j] == MFGM_LIK_BERNOULLI) {
            if (!(p >= 0.0 && p < 0.5)) return 1;
        } else if (rd.kind[j] == MFGM_LIK_POISSON || rd.kind[j] == MFGM_LIK_GAUSSIAN) {
            if (!(p > 0.0 && p < INFINITY)) return 1;
        } else {
            return 1;
        }
    }
    return 0;
}

template <int D>
int site_update_impl(const Plan& P, const Readout& rd, const double* mu, const double* Sig, int gathered, const long long* node_ids,
                     int n, const double* y, double* theta_lin, double* theta_diag, double* sites_vec, double* sites_sym, double lr,
                     hipStream_t st) {
    hipLaunchKernelGGL((k_readout_site_update<D>), dim3((n + 255) / 256), dim3(256), 0, st, P.lv[0], P.T, rd, mu, Sig, gathered,
                       node_ids, n, y, theta_lin, theta_diag, sites_vec, sites_sym, lr);
    MFGM_CHECK_LAUNCH();
    return 0;
}

template <int D>
int obs_ve_impl(const Plan& P, const Readout& rd, const double* mu, const double* Sig, const long long* node_ids, int n_per,
                const double* y, double* out_mu, double* out_cov, double* ve, hipStream_t st) {
    hipLaunchKernelGGL((k_readout_obs_ve<D>), dim3((n_per + 255) / 256, P.B), dim3(256), 0, st, P.lv[0], P.T, rd, mu, Sig, node_ids,
                       n_per, y, out_mu, out_cov, ve);
    MFGM_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

int mfgm_readout_site_update(const mfgm_plan* plan, const mfgm_readout* readout, const double* mu, const double* Sig, int gathered,
                             const long long* node_ids, int n, const double* y, double* theta_lin, double* theta_diag,
                             double* sites_vec, double* sites_sym, double lr, void* stream) {
    Readout rd;
    if (readout_check(plan, readout, rd)) return 1;
    if (!(lr >= 0.0 && lr <= 1.0) || n < 0 || (gathered != 0 && gathered != 1)) return 1;
    if (n == 0) return 0;
    if (!mu || !Sig || !node_ids || !y || !theta_lin || !theta_diag || !sites_vec || !sites_sym) return 1;
    const Plan& P = plan->p;
    hipStream_t st = (hipStream_t)stream;
    MFGM_DISPATCH_D(P.d, (site_update_impl<DD>(P, rd, mu, Sig, gathered, node_ids, n, y, theta_lin, theta_diag, sites_vec, sites_sym,
                                               lr, st)));
}

int mfgm_readout_obs_ve(const mfgm_plan* plan, const mfgm_readout* readout, const double* mu, const double* Sig,
                        const long long* node_ids, int n_per, const double* y, double* out_mu, double* out_cov, double* ve,
                        void* stream) {
    Readout rd;
    if (readout_check(plan, readout, rd)) return 1;
    if (n_per < 0) return 1;
    if (n_per == 0) return 0;
    if (!mu || !Sig || !node_ids || !y || !ve) return 1;
    const Plan& P = plan->p;
    hipStream_t st = (hipStream_t)stream;
    MFGM_DISPATCH_D(P.d, (obs_ve_impl<DD>(P, rd, mu, Sig, node_ids, n_per, y, out_mu, out_cov, ve, st)));
}

}  // extern "C"
