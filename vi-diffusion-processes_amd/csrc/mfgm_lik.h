// Per-observation variational expectations of the scalar non-Gaussian likelihoods (include/mfgm.h, mfgm_scalar_lik) and their
// gradients with respect to the expectation parameters: the quantities the CVI site update needs (markovflow/models/variational_cvi.py:
// 332-349, sparse_variational_cvi.py:176-221, where a GradientTape runs over gpflow's variational_expectations).
//
//   Bernoulli, probit link with jitter j (kind 1):  the 20-point Gauss-Hermite rule of gpflow's NDiagGHQuadrature,
//       X_k = mu + sqrt(2) sigma xi_k,  VE = sum_k W_k l(X_k),  l = log(j + (1 - 2j) Phi(s X)),  s = +1 for y == 1 else -1,
//       and the derivatives OF THE RULE (what a tape over it gives):  dmu = sum_k W_k l'(X_k),  dv = sum_k W_k l'(X_k) xi_k / (sqrt(2) sigma)
//   Poisson, exp link with bin size b (kind 2):  closed form, VE = y log b + y mu - b e^{mu + v/2} - lgamma(y + 1)
//
// One lane per observation: coalesced [n] loads and stores, no LDS, no atomics.  fp64 erfc / exp / log are software sequences on
// gfx950 (no hardware fp64 transcendentals), so the Bernoulli kernel is bound by VALU issue, not by HBM.
#pragma once
#include <hip/hip_runtime.h>

#include "mfgm_gh.h"
#include "mfgm_math.h"

namespace mfgm {

constexpr double kLikSqrt2 = 1.41421356237309504880;
constexpr double kLikInvSqrt2 = 0.70710678118654752440;
constexpr double kLikInvSqrt2Pi = 0.39894228040143267794;

// Bernoulli-probit: VE and (dVE/dmu, dVE/dv) at one observation.  v <= 0 gives NaN (sqrt of a negative, or a 0 / 0): not clamped.
MFGM_DEV void lik_bernoulli(double mu, double v, double y, double jit, double& ve, double& dmu, double& dv) {
    const double sigma = sqrt(v);
    const double sgn = (y == 1.0) ? 1.0 : -1.0;
    const double c = 1.0 - 2.0 * jit;
    const double sc = kLikSqrt2 * sigma;
    double a = 0.0, b = 0.0, e = 0.0;
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        double xi, w;
        gh_node(20, k, xi, w);
        const double X = mu + sc * xi;
        const double z = sgn * X;
        // p = j + (1 - 2j) Phi(z), Phi(z) = erfc(-z / sqrt 2) / 2: for y != 1 this is 1 - p_j(X) in the Phi(-X) form
        const double p = jit + c * (0.5 * erfc(-z * kLikInvSqrt2));
        const double dl = sgn * c * (kLikInvSqrt2Pi * exp(-0.5 * X * X)) / p;
        a += w * log(p);
        b += w * dl;
        e += w * dl * xi;
    }
    ve = a;
    dmu = b;
    dv = e / sc;
}

// Poisson-exp: closed form (gpflow.likelihoods.Poisson.variational_expectations and its derivatives)
MFGM_DEV void lik_poisson(double mu, double v, double y, double binsize, double& ve, double& dmu, double& dv) {
    const double m = binsize * exp(mu + 0.5 * v);
    ve = y * log(binsize) + y * mu - m - lgamma(y + 1.0);
    dmu = y - m;
    dv = -0.5 * m;
}

// ve [n], g1 = dmu - 2 dv mu, g2 = dv [n]; a null output is not written
template <int KIND>
__global__ __launch_bounds__(256) void k_scalar_lik(size_t n, const double* __restrict__ fmu, const double* __restrict__ fvar,
                                                    const double* __restrict__ y, double param, double* __restrict__ ve_out,
                                                    double* __restrict__ g1_out, double* __restrict__ g2_out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double mu = fmu[i], v = fvar[i], yi = y[i];
    double ve, dmu, dv;
    if (KIND == 1)
        lik_bernoulli(mu, v, yi, param, ve, dmu, dv);
    else
        lik_poisson(mu, v, yi, param, ve, dmu, dv);
    if (ve_out) ve_out[i] = ve;
    if (g1_out) g1_out[i] = dmu - 2.0 * dv * mu;
    if (g2_out) g2_out[i] = dv;
}

}  // namespace mfgm
