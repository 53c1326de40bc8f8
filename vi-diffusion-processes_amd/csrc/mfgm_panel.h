// Local kernels of the panel sparse CVI model (panel_variational_cvi.py): B independent series that share one kernel, one inducing grid
// of M states and one likelihood, state dimension d <= 8, on the PACKED arrays of the B-chain lane-per-segment plan (mfgm_layout.h).
// The three passes of mfgm_sparse.h (one wavefront per interval of one chain) in the shape a panel needs, where an interval holds a
// handful of points and there are thousands of chains:
//
//   k_panel_theta   : prior naturals (shared by every series, natural layout) + the [B, M+1, 2d, 2d] sites overlap-added, written
//                     straight into the packed VEC / SYM / FULL arrays; one workgroup per (64 lanes, step): the site blocks of a node
//                     are read as contiguous runs, transposed through LDS, and stored as 512-byte lane rows
//   k_panel_predict : one lane per data point; the pair mean and covariance of the point's interval are streamed entry by entry out of
//                     the packed marginals (neighbouring lanes are neighbouring points of one series and mostly hit the same
//                     addresses), fvar is a running sum; the likelihood, its gradients and the row's VE sum come from those very values
//   k_panel_sites   : one lane per (series, interval, row) walking its CSR range with 2d accumulators; one owner per entry
//
// No atomics anywhere: every sum has a fixed order, two launches agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "mfgm_layout.h"
#include "mfgm_lik.h"
#include "mfgm_math.h"

namespace mfgm {

struct PanelArgs {
    int B, M, d, N;
    const int* idx;            // [B, N] interval 0..M of each point
    const int* seg;            // [B, M + 2] CSR offsets per interval, relative to the row (site update only)
    const double* w;           // [B, N, 2d]
    const double* c;           // [B, N]
    const double* prior_mean;  // [d]    shared
    const double* prior_cov;   // [d, d] shared
};

constexpr int kPanelGaussian = 3;      // MFGM_LIK_GAUSSIAN; 1 / 2 are the kinds of mfgm_lik.h

// theta = prior naturals + overlap-added sites, packed.  nat1 [B, T+1, 2d], nat2 [B, T+1, 2d, 2d]; plin [T, d] (may be null),
// pdiag / psub [T, d, d] natural and shared; lin (VEC), diag (SYM), sub (FULL) packed, every position written (padding lanes and
// steps, and the sub-diagonal block of the last node, get zeros: what mfgm_pack leaves there).  Block (wave tile w, step s).
template <int D>
static __global__ __launch_bounds__(256) void k_panel_theta(LevelDesc lv, int T, const double* __restrict__ nat1,
                                                           const double* __restrict__ nat2, const double* __restrict__ plin,
                                                           const double* __restrict__ pdiag, const double* __restrict__ psub,
                                                           double* __restrict__ lin, double* __restrict__ diag, double* __restrict__ sub) {
    constexpr int NT = D * (D + 1) / 2, DD = D * D, D2 = 2 * D, EO = NT + DD + D, ST = EO | 1;      // odd row stride: conflict free
    __shared__ double tile[64 * ST];
    const int wt = blockIdx.x / lv.R, s = blockIdx.x - wt * lv.R, tid = threadIdx.x;
    for (int k = tid; k < 64 * EO; k += 256) {
        const int li = k / EO, o = k - li * EO, lane = wt * 64 + li;
        double v = 0.0;
        if (lane < lv.L) {
            const int b = lane / lv.P, t = (lane - b * lv.P) * lv.R + s;
            if (t < T) {
                const size_t site = (size_t)b * (T + 1) + t;            // site t: its second state is inducing state t
                const double* n_lo = nat2 + site * (D2 * D2);
                const double* n_hi = n_lo + D2 * D2;                      // site t+1: its first state is inducing state t
                if (o < NT) {
                    int i = 0;
                    while (tix(i + 1, 0) <= o) ++i;
                    const int j = o - tix(i, 0);
                    v = pdiag[((size_t)t * D + i) * D + j] + n_hi[i * D2 + j] + n_lo[(D + i) * D2 + (D + j)];
                } else if (o < NT + DD) {
                    const int r = o - NT, i = r / D, j = r - i * D;
                    if (t + 1 < T) v = psub[((size_t)t * D + i) * D + j] + 2.0 * n_hi[(D + i) * D2 + j];
                } else {
                    const int i = o - NT - DD;
                    v = (plin ? plin[(size_t)t * D + i] : 0.0) + nat1[(site + 1) * D2 + i] + nat1[site * D2 + D + i];
                }
            }
        }
        tile[li * ST + o] = v;
    }
    __syncthreads();
    const size_t node = (size_t)wt * lv.R + s;
    for (int k = tid; k < 64 * EO; k += 256) {
        const int li = k & 63, o = k >> 6;
        const double v = tile[li * ST + o];
        if (o < NT) diag[(node * NT + o) * 64 + li] = v;
        else if (o < NT + DD) sub[(node * DD + (o - NT)) * 64 + li] = v;
        else lin[(node * D + (o - NT - DD)) * 64 + li] = v;
    }
}

// One half of the pair: mu += w . m, v += w^T S w with S symmetric -- the prior's dense [d, d] block at the ends of the chain, else the
// packed lower triangle of node (b, t) (element e of a node lies 64 doubles after element e - 1).
template <int D>
MFGM_DEV void panel_half(const double* w, bool prior, const double* pm, const double* pc, const double* xs, const double* Ss, double& mu,
                         double& v) {
    const double* m = prior ? pm : xs;
    const double* S = prior ? pc : Ss;
    const int st = prior ? 1 : 64;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        mu = __builtin_fma(w[i], m[i * st], mu);
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double sij = S[(prior ? i * D + j : tix(i, j)) * st];
            v = __builtin_fma((i == j ? w[i] : 2.0 * w[i]) * w[j], sij, v);
        }
    }
}

// One workgroup per series, one lane per data point (strided by the workgroup).  x (VEC), Sig (SYM), Sub (FULL, Sigma_{t+1,t} at t)
// packed; fmu, fvar, ve, g1, g2 [B, N] and ve_series [B] may each be null.  KIND 0: prediction only.
template <int D, int KIND>
static __global__ __launch_bounds__(256) void k_panel_predict(PanelArgs a, LevelDesc lv, double param, const double* __restrict__ y,
                                                             const double* __restrict__ x, const double* __restrict__ Sig,
                                                             const double* __restrict__ Sub, double* __restrict__ fmu,
                                                             double* __restrict__ fvar, double* __restrict__ ve, double* __restrict__ g1,
                                                             double* __restrict__ g2, double* __restrict__ ve_series) {
    constexpr int NT = D * (D + 1) / 2, DD = D * D, D2 = 2 * D;
    __shared__ double red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    double total = 0.0;
    for (int i = tid; i < a.N; i += blockDim.x) {
        const size_t k = (size_t)b * a.N + i;
        const int m = min(max(a.idx[k], 0), a.M);
        double w[D2];
#pragma unroll
        for (int r = 0; r < D2; ++r) w[r] = a.w[k * D2 + r];
        const bool lo_prior = (m == 0), hi_prior = (m == a.M);
        // packed position of the nodes m - 1 and m of chain b (clamped where the prior stands in: the address is then not read)
        const int t_lo = lo_prior ? 0 : m - 1, t_hi = hi_prior ? a.M - 1 : m;
        const int p_lo = t_lo / lv.R, p_hi = t_hi / lv.R;
        const size_t l_lo = (size_t)b * lv.P + p_lo, l_hi = (size_t)b * lv.P + p_hi;
        const size_t n_lo = (l_lo >> 6) * lv.R + (t_lo - p_lo * lv.R), n_hi = (l_hi >> 6) * lv.R + (t_hi - p_hi * lv.R);
        const int q_lo = (int)(l_lo & 63), q_hi = (int)(l_hi & 63);
        double mu = 0.0, v = a.c[k];
        panel_half<D>(w, lo_prior, a.prior_mean, a.prior_cov, x + n_lo * D * 64 + q_lo, Sig + n_lo * NT * 64 + q_lo, mu, v);
        panel_half<D>(w + D, hi_prior, a.prior_mean, a.prior_cov, x + n_hi * D * 64 + q_hi, Sig + n_hi * NT * 64 + q_hi, mu, v);
        if (!lo_prior && !hi_prior) {
            const double* C = Sub + n_lo * DD * 64 + q_lo;          // Cov(x_m, x_{m-1}), stored at node m - 1
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int c = 0; c < D; ++c) v = __builtin_fma(2.0 * w[D + r] * w[c], C[(r * D + c) * 64], v);
        }
        if (fmu) fmu[k] = mu;
        if (fvar) fvar[k] = v;
        if (KIND != 0) {
            const double yi = y[k];
            double e = 0.0, q1 = 0.0, q2 = 0.0;
            if (yi == yi) {          // a NaN observation is an absent point
                double dmu, dv;
                if (KIND == 1) {
                    lik_bernoulli(mu, v, yi, param, e, dmu, dv);
                } else if (KIND == 2) {
                    lik_poisson(mu, v, yi, param, e, dmu, dv);
                } else {
                    const double r = yi - mu, is2 = 1.0 / param;
                    e = -0.5 * log(2.0 * M_PI * param) - 0.5 * (r * r + v) * is2;
                    dmu = r * is2;
                    dv = -0.5 * is2;
                }
                q1 = dmu - 2.0 * dv * mu;
                q2 = dv;
            }
            if (ve) ve[k] = e;
            if (g1) g1[k] = q1;
            if (g2) g2[k] = q2;
            total += e;
        }
    }
    if (KIND != 0 && ve_series) {
        // fixed order: the lane's own points in order, the wavefront's tree, then the wavefronts in order
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off, 64);
        if ((tid & 63) == 0) red[tid >> 6] = total;
        __syncthreads();
        if (tid == 0) {
            double s = red[0];
            for (int q = 1; q < (int)(blockDim.x >> 6); ++q) s += red[q];
            ve_series[b] = s;
        }
    }
}

// sites <- (1 - lr) sites + lr (sum_i g1_i w_i, sum_i g2_i w_i w_i^T) over the CSR range of (series b, interval m), in place; lane
// (b, m, r) owns nat1[b][m][r] and row r of nat2[b][m].  g2 (w_r w_c) with the product of the two w's taken first: entry (r, c) and
// entry (c, r) are the same bits.
template <int D>
static __global__ __launch_bounds__(256) void k_panel_sites(PanelArgs a, const double* __restrict__ g1, const double* __restrict__ g2,
                                                           double lr, double* __restrict__ nat1, double* __restrict__ nat2) {
    constexpr int D2 = 2 * D;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)a.B * (a.M + 1) * D2;
    if (gid >= total) return;
    const size_t bm = gid / D2, b = bm / (a.M + 1);
    const int r = (int)(gid - bm * D2), m = (int)(bm - b * (a.M + 1));
    int i0 = 0, i1 = 0;
    if (a.N > 0) {
        const int* sg = a.seg + b * (a.M + 2);
        i0 = min(max(sg[m], 0), a.N);
        i1 = min(max(sg[m + 1], i0), a.N);
    }
    double acc[D2], acc1 = 0.0;
#pragma unroll
    for (int c = 0; c < D2; ++c) acc[c] = 0.0;
    for (int i = i0; i < i1; ++i) {
        const size_t k = b * a.N + i;
        const double* w = a.w + k * D2;
        const double wr = w[r], q2 = g2[k];
        acc1 = __builtin_fma(g1[k], wr, acc1);
#pragma unroll
        for (int c = 0; c < D2; ++c) acc[c] = __builtin_fma(q2, wr * w[c], acc[c]);
    }
    double* row = nat2 + gid * D2;
#pragma unroll
    for (int c = 0; c < D2; ++c) row[c] = __builtin_fma(lr, acc[c], (1.0 - lr) * row[c]);
    nat1[gid] = __builtin_fma(lr, acc1, (1.0 - lr) * nat1[gid]);
}

}  // namespace mfgm
