// Linear-readout likelihoods of the diffusion models (include/mfgm.h, mfgm_readout): p(y_i | x_i) = prod_j p_j(y_ij | h_j^T x_i + c_j)
// with a Gaussian, Bernoulli-probit or Poisson-exp factor per output.  Two kernels on the packed marginals of a lane-per-segment plan:
//   k_readout_site_update   update_data_sites of the CVI models at the listed nodes: marginal -> projections -> per-output scalar
//                           quantities -> (g1, g2) -> blend of the site arrays -> scatter of new - old into the posterior naturals
//   k_readout_obs_ve        the per-trajectory sums of the variational expectations (launch shape and reduction of k_mvn_obs_ve)
// One lane per observation.  The marginal (D + D (D + 1) / 2 doubles) and the accumulators of g1, g2 (the same count again) live in
// registers; H, c, the kinds and their parameters come from the kernel arguments (scalar registers), so the loop over the outputs and
// its branch on the kind are wave-uniform.  A NaN entry of y switches the output off by selects (no divergent branch).  The Bernoulli
// factor is bound by VALU issue (20 software fp64 erfc / exp / log per output), the others by the latency of the scattered node reads.
#pragma once
#include "mfgm_layout.h"
#include "mfgm_lik.h"
#include "mfgm_math.h"

namespace mfgm {

struct Readout {   // mfgm_readout (include/mfgm.h)
    int o, d, kind[8];
    double param[8], offset[8], H[64];
};

constexpr double kReadoutLog2Pi = 1.83787706640934548356;

// node block of node id = b T + t and the lane's position in it: element e of a kind with E doubles at (nb * E + e) * 64 + l
MFGM_DEV void readout_locate(const LevelDesc& lv, int T, unsigned id, size_t& nb, unsigned& l) {
    const unsigned cb = id / (unsigned)T, t = id - cb * (unsigned)T;
    const unsigned p = t / lv.R, s = t - p * lv.R, lane = cb * lv.P + p;
    nb = (size_t)(lane >> 6) * lv.R + s;
    l = lane & 63;
}

// the marginal of observation i: from the packed arrays at its node, or from natural [n, D] / [n, D, D] arrays (lower triangle read)
template <int D>
MFGM_DEV void readout_marginal(const double* __restrict__ mug, const double* __restrict__ Sigg, bool gathered, size_t i, size_t nb,
                               unsigned l, double (&m)[D], double (&S)[MFGM_NTRI(D)]) {
    constexpr int ET = MFGM_NTRI(D);
    if (gathered) {
#pragma unroll
        for (int e = 0; e < D; ++e) m[e] = mug[i * D + e];
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) S[tix(r, c)] = Sigg[(i * D + r) * D + c];
    } else {
#pragma unroll
        for (int e = 0; e < D; ++e) m[e] = mug[(nb * D + e) * 64 + l];
#pragma unroll
        for (int e = 0; e < ET; ++e) S[e] = Sigg[(nb * ET + e) * 64 + l];
    }
}

// VE_i = sum_j ve_j and, with WANT_G,  g1 = sum_j h_j (dm_j - 2 dv_j h_j^T mu),  g2 = sum_j dv_j h_j h_j^T  (lower triangle)
template <int D, bool WANT_G>
MFGM_DEV double readout_eval(const Readout& rd, const double (&m)[D], const double (&S)[MFGM_NTRI(D)], const double* __restrict__ yrow,
                             double (&g1)[D], double (&g2)[MFGM_NTRI(D)]) {
    double ve = 0.0;
    if (WANT_G) {
#pragma unroll
        for (int e = 0; e < D; ++e) g1[e] = 0.0;
#pragma unroll
        for (int e = 0; e < MFGM_NTRI(D); ++e) g2[e] = 0.0;
    }
#pragma unroll 1
    for (int j = 0; j < rd.o; ++j) {
        double h[D];
#pragma unroll
        for (int e = 0; e < D; ++e) h[e] = rd.H[j * D + e];
        double hm = 0.0, v = 0.0;
#pragma unroll
        for (int r = 0; r < D; ++r) {
            hm = __builtin_fma(h[r], m[r], hm);
            double sh = 0.0;
#pragma unroll
            for (int c = 0; c < D; ++c) sh = __builtin_fma(S[six(r, c)], h[c], sh);
            v = __builtin_fma(h[r], sh, v);
        }
        const double mj = hm + rd.offset[j];
        const double yraw = yrow[j];
        const bool seen = (yraw == yraw);
        const double y = seen ? yraw : 0.0;
        const int kind = rd.kind[j];
        const double prm = rd.param[j];
        double vj, dm, dv;
        if (kind == MFGM_LIK_BERNOULLI) {
            lik_bernoulli(mj, v, y, prm, vj, dm, dv);
        } else if (kind == MFGM_LIK_POISSON) {
            lik_poisson(mj, v, y, prm, vj, dm, dv);
        } else {
            const double r = y - mj, is2 = 1.0 / prm;
            vj = -0.5 * (kReadoutLog2Pi + log(prm)) - 0.5 * (r * r + v) * is2;
            dm = r * is2;
            dv = -0.5 * is2;
        }
        vj = seen ? vj : 0.0;
        dm = seen ? dm : 0.0;
        dv = seen ? dv : 0.0;
        ve += vj;
        if (WANT_G) {
            const double a = dm - 2.0 * dv * hm;
#pragma unroll
            for (int r = 0; r < D; ++r) {
                g1[r] = __builtin_fma(h[r], a, g1[r]);
                const double dh = dv * h[r];
#pragma unroll
                for (int c = 0; c <= r; ++c) g2[tix(r, c)] = __builtin_fma(dh, h[c], g2[tix(r, c)]);
            }
        }
    }
    return ve;
}

// sites <- (1 - lr) sites + lr g with g made here; theta_lin (VEC) / theta_diag (SYM, lower triangle) += new - old at the node.
// The node ids of one call are distinct (the scatter is a plain read-modify-write, as in k_site_update_pair).
template <int D>
static __global__ __launch_bounds__(256) void k_readout_site_update(LevelDesc lv, int T, Readout rd, const double* __restrict__ mug,
                                                                    const double* __restrict__ Sigg, int gathered,
                                                                    const long long* __restrict__ node_ids, int n,
                                                                    const double* __restrict__ y, double* __restrict__ theta_lin,
                                                                    double* __restrict__ theta_diag, double* __restrict__ sites_vec,
                                                                    double* __restrict__ sites_sym, double lr) {
    constexpr int ET = MFGM_NTRI(D);
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    size_t nb;
    unsigned l;
    readout_locate(lv, T, (unsigned)node_ids[i], nb, l);
    double m[D], S[ET], g1[D], g2[ET];
    readout_marginal<D>(mug, Sigg, gathered != 0, i, nb, l, m, S);
    readout_eval<D, true>(rd, m, S, y + (size_t)i * rd.o, g1, g2);
    const double keep = 1.0 - lr;
#pragma unroll
    for (int e = 0; e < D; ++e) {
        const size_t k = (size_t)i * D + e;
        const double old = sites_vec[k], nw = keep * old + lr * g1[e];
        sites_vec[k] = nw;
        theta_lin[(nb * D + e) * 64 + l] += nw - old;
    }
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            const size_t k = ((size_t)i * D + r) * D + c;
            const double old = sites_sym[k], nw = keep * old + lr * g2[tix(r, c)];
            sites_sym[k] = nw;
            theta_diag[(nb * ET + tix(r, c)) * 64 + l] += nw - old;
            if (c < r) {
                const size_t ku = ((size_t)i * D + c) * D + r;
                sites_sym[ku] = keep * sites_sym[ku] + lr * g2[tix(r, c)];
            }
        }
}

// ve[b * gridDim.x + x] = sum of VE_i over observations x * 256 ... of trajectory b (fixed order); the gathered marginals to out_mu
// [B n_per, D] / out_cov [B n_per, D, D] when given
template <int D>
static __global__ __launch_bounds__(256) void k_readout_obs_ve(LevelDesc lv, int T, Readout rd, const double* __restrict__ mug,
                                                               const double* __restrict__ Sigg, const long long* __restrict__ node_ids,
                                                               int n_per, const double* __restrict__ y, double* __restrict__ out_mu,
                                                               double* __restrict__ out_cov, double* __restrict__ ve) {
    constexpr int ET = MFGM_NTRI(D);
    __shared__ double red[256];
    const int b = blockIdx.y;
    double acc = 0.0;
    const int j = blockIdx.x * 256 + threadIdx.x;      // the grid covers n_per: one observation per lane
    if (j < n_per) {
        const size_t i = (size_t)b * n_per + j;
        size_t nb;
        unsigned l;
        readout_locate(lv, T, (unsigned)node_ids[i], nb, l);
        double m[D], S[ET], g1[D], g2[ET];
        readout_marginal<D>(mug, Sigg, false, i, nb, l, m, S);
        acc = readout_eval<D, false>(rd, m, S, y + i * rd.o, g1, g2);
        if (out_mu) {
#pragma unroll
            for (int e = 0; e < D; ++e) out_mu[i * D + e] = m[e];
        }
        if (out_cov) {
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int c = 0; c < D; ++c) out_cov[(i * D + r) * D + c] = S[six(r, c)];
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) ve[(size_t)b * gridDim.x + blockIdx.x] = red[0];
}

}  // namespace mfgm
