// Power Expectation Propagation site update of the sites-on-f GP models (include/mfgm.h, mfgm_pep_sites / mfgm_pep_tilted; the update
// of markovflow/models/pep.py:179-215 with the power alpha applied to the likelihood and the energy terms taken at the cavity).
//
// Per point, from the posterior f-marginal (mu, v) and the site (eta1, eta2, l):
//   cavity (the rank-one state-space cavity projected onto f):  lc = 1/v + 2 alpha eta2,  vc = 1/lc,  mc = vc (mu/v - alpha eta1)
//   tilted normaliser  log Z = log int p(y|f)^alpha N(f; mc, vc) df  and its first two derivatives d1, d2 with respect to mc:
//     Gaussian (variance s^2): closed form;  Bernoulli-probit at alpha = 1: closed form log p_j(s mc / sqrt(1 + vc));
//     Bernoulli at alpha != 1 and Poisson: the 20-point Gauss-Hermite rule in log space (the derivatives of the rule)
//   update (gradient_correction, pep.py:250-261):  L2 = 1/2 / (vc + 1/d2),  L1 = 2 L2 (d1/d2 - mc),
//     e = log Z + n(mc, vc) - n(mu, v),  n(m, v) = 1/2 (log v + m^2 / v)
//     site <- (1 - lr) site + lr ((1 - alpha) site + (L1, L2, e))
//
// One lane per selected point, as k_scalar_lik: coalesced loads and stores when the index list is absent, no LDS, no atomics but the
// rare skip counter.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/mfgm.h"
#include "mfgm_gh.h"
#include "mfgm_lik.h"
#include "mfgm_math.h"

namespace mfgm {

constexpr double kPepLog2Pi = 1.83787706640934548356;

// log l(X) and its first two derivatives of one likelihood kind at X (Bernoulli: s = +1 for y == 1 else -1, jitter j; Poisson: bin b)
template <int KIND>
MFGM_DEV void pep_loglik(double X, double y, double param, double& l, double& dl, double& d2l) {
    if (KIND == MFGM_LIK_BERNOULLI) {
        const double sgn = (y == 1.0) ? 1.0 : -1.0;
        const double c = 1.0 - 2.0 * param;
        const double p = param + c * (0.5 * erfc(-sgn * X * kLikInvSqrt2));
        l = log(p);
        dl = sgn * c * (kLikInvSqrt2Pi * exp(-0.5 * X * X)) / p;
        d2l = -X * dl - dl * dl;
    } else {
        const double m = param * exp(X);
        l = y * (log(param) + X) - m - lgamma(y + 1.0);
        dl = y - m;
        d2l = -m;
    }
}

// log Z and (d1, d2) = derivatives of log Z with respect to mc, at the cavity N(mc, vc)
template <int KIND>
MFGM_DEV void pep_tilted(double mc, double vc, double y, double param, double alpha, double& lz, double& d1, double& d2) {
    if (KIND == MFGM_LIK_GAUSSIAN) {
        const double S = param / alpha + vc;
        const double r = y - mc;
        lz = 0.5 * (1.0 - alpha) * (kPepLog2Pi + log(param)) - 0.5 * log(alpha) - 0.5 * (kPepLog2Pi + log(S)) - 0.5 * r * r / S;
        d1 = r / S;
        d2 = -1.0 / S;
        return;
    }
    if (KIND == MFGM_LIK_BERNOULLI && alpha == 1.0) {
        // int p_j(s f) N(f; mc, vc) df = p_j(s mc / sqrt(1 + vc)) exactly (gpflow's Bernoulli.predict_log_density)
        const double sgn = (y == 1.0) ? 1.0 : -1.0;
        const double c = 1.0 - 2.0 * param;
        const double q = 1.0 / sqrt(1.0 + vc);
        const double z = sgn * mc * q;
        const double p = param + c * (0.5 * erfc(-z * kLikInvSqrt2));
        const double g = c * (kLikInvSqrt2Pi * exp(-0.5 * z * z)) / p;     // d log p / dz
        lz = log(p);
        d1 = sgn * q * g;
        d2 = (-z * g - g * g) * (q * q);
        return;
    }
    // log-space rule: a_k = log W_k + alpha l(X_k), pi = softmax(a), log Z = logsumexp(a); running maximum M of alpha l(X_k) with
    // rescaling, so that no weight table in log form is needed (the node that sets M contributes W_k >= 1e-13: no underflow)
    const double sc = sqrt(2.0 * vc);
    double M = -INFINITY, S = 0.0, P1 = 0.0, P2 = 0.0;
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        double xi, w;
        gh_node(20, k, xi, w);
        double l, dl, d2l;
        pep_loglik<KIND>(mc + sc * xi, y, param, l, dl, d2l);
        const double a = alpha * l, g1 = alpha * dl, g2 = alpha * d2l + g1 * g1;
        if (a > M) {
            const double r = exp(M - a);     // exp(-inf) = 0 at the first node
            S *= r;
            P1 *= r;
            P2 *= r;
            M = a;
        }
        const double e = w * exp(a - M);
        S += e;
        P1 += e * g1;
        P2 += e * g2;
    }
    lz = M + log(S);
    d1 = P1 / S;
    d2 = P2 / S - d1 * d1;
}

// [k] selected points (idx[j], or j when idx is null); out-of-range indices are ignored
template <int KIND>
__global__ __launch_bounds__(256) void k_pep_sites(size_t n, size_t k, const int64_t* __restrict__ idx, const double* __restrict__ fmu,
                                                   const double* __restrict__ fvar, const double* __restrict__ y, double param,
                                                   double alpha, double lr, double* __restrict__ nat1, double* __restrict__ nat2,
                                                   double* __restrict__ lnorm, double* __restrict__ e_out, int* __restrict__ skipped) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    size_t i = j;
    if (idx) {
        const int64_t ii = idx[j];
        if (ii < 0 || (uint64_t)ii >= (uint64_t)n) return;
        i = (size_t)ii;
    }
    const double mu = fmu[i], v = fvar[i], yi = y[i], eta1 = nat1[i], eta2 = nat2[i];
    const double lc = 1.0 / v + 2.0 * alpha * eta2;
    bool ok = (v > 0.0) && (lc > 0.0);
    double L1 = 0.0, L2 = 0.0, e = NAN;
    if (ok) {
        const double vc = 1.0 / lc;
        const double mc = vc * (mu / v - alpha * eta1);
        double lz, d1, d2;
        pep_tilted<KIND>(mc, vc, yi, param, alpha, lz, d1, d2);
        L2 = 0.5 / (vc + 1.0 / d2);
        L1 = 2.0 * L2 * (d1 / d2 - mc);
        e = lz + 0.5 * (log(vc) + mc * mc / vc) - 0.5 * (log(v) + mu * mu / v);
        ok = isfinite(L1) && isfinite(L2);
    }
    if (!ok) {
        if (skipped) atomicAdd(skipped, 1);
        if (e_out) e_out[i] = NAN;
        return;
    }
    if (e_out) e_out[i] = e;
    if (lr != 0.0) {
        const double a1 = 1.0 - alpha, r1 = 1.0 - lr;
        nat1[i] = r1 * eta1 + lr * (a1 * eta1 + L1);
        nat2[i] = r1 * eta2 + lr * (a1 * eta2 + L2);
        if (lnorm) {
            const double l0 = lnorm[i];
            lnorm[i] = r1 * l0 + lr * (a1 * l0 + e);
        }
    }
}

// log Z, d1, d2 [n] at given cavities (mc, vc); a null output is not written
template <int KIND>
__global__ __launch_bounds__(256) void k_pep_tilted(size_t n, const double* __restrict__ mc, const double* __restrict__ vc,
                                                    const double* __restrict__ y, double param, double alpha, double* __restrict__ lz_out,
                                                    double* __restrict__ d1_out, double* __restrict__ d2_out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double lz, d1, d2;
    pep_tilted<KIND>(mc[i], vc[i], y[i], param, alpha, lz, d1, d2);
    if (lz_out) lz_out[i] = lz;
    if (d1_out) d1_out[i] = d1;
    if (d2_out) d2_out[i] = d2;
}

}  // namespace mfgm
