// Local kernels of the spatio-temporal sparse CVI model (markovflow/models/spatio_temporal_variational.py:360-586): sparse CVI on pairs
// of inducing states whose state is Ms independent copies of a Markovian time kernel of dimension dt (D = Ms dt, 8 < D <= 32), one per
// spatial inducing point.  The projection of data point i onto its pair of inducing states is a Kronecker product
//
//   w_i[half D + j dt + k] = a_i[j] h_i[half dt + k],   a_i = chol(K_s(Z_s, Z_s))^-1 k_s(Z_s, x_i) [Ms],   h_i = H_t P^t_i [2 dt]
//
// so the two per-step passes of mfgm_sparse.h (k_sparse_predict_v, k_sparse_sites_q) read (Ms + 2 dt) doubles per point where the
// materialised w [N, 2D] costs 2D, and rebuild the rows of W in LDS:
//
//   k_st_predict  : q(f(x_i, t_i)) from the pair marginals of the interval (and the KL terms of the pair, as k_sparse_predict_v)
//   k_st_sites_q  : sites <- (1 - lr) sites + lr sum_i (g1_i w_i, g2_i w_i w_i^T) on the quadrant-packed nat2q
//
// Intervals, seg and the prior padding at both ends are those of mfgm_sparse.h.  No atomics: one owner per output entry, so two
// launches on the same inputs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "mfgm_sparse.h"

namespace mfgm {

struct StArgs {
    int M, Ms, dt, d, N;       // d = Ms dt
    const int* seg;            // [M + 2]
    const double* a;           // [N, Ms]
    const double* h;           // [N, 2 dt]
    const double* c;           // [N]
    const double* prior_mean;  // [d]
    const double* prior_cov;   // [d, d]
};

// Building rows of W in LDS (row stride st): entry l = half d + j dt + k of point i is a_i[j] h_i[half dt + k].  Thread tid of NT owns
// column l = tid mod 2d for the points sub, sub + nsub, ... of a chunk (sub = tid / 2d, nsub = NT / 2d; the threads beyond nsub 2d
// idle): the decode of l into (j, half, k) is done once per kernel, and a chunk costs its points two loads and one store each.
struct StStage {
    int l, sub, nsub, ja, jh;
    __device__ __forceinline__ StStage(const StArgs& a, int tid, int nt) {
        const int d = a.d, d2 = 2 * d;
        l = tid % d2;
        sub = tid / d2;
        nsub = nt / d2;
        const int half = (l >= d) ? 1 : 0, r = l - half * d, j = r / a.dt;
        ja = j;
        jh = half * a.dt + (r - j * a.dt);
    }
    // rows c0 .. c0 + np
    __device__ __forceinline__ void rows(const StArgs& a, int c0, int np, int st, double* __restrict__ sh) const {
        if (sub >= nsub) return;
        const int h2 = 2 * a.dt;
        for (int pt = sub; pt < np; pt += nsub) {
            const size_t i = (size_t)(c0 + pt);
            sh[pt * st + l] = a.a[i * a.Ms + ja] * a.h[i * h2 + jh];
        }
    }
};

// One wavefront per interval.  The three blocks of the pair covariance that matter (Sigma_{m-1}, Sigma_m, C = Sigma_{m,m-1}; the upper
// right block is C^T) stay in registers: for even d (PAIR) the 16-byte pair lane + 64 j of each block with lane `lane`, as
// k_sparse_predict_v holds them (a pair never leaves its row, and shares the row's two entries of w: 3 LDS reads per entry and 16
// index registers at d = 30, where entry-per-lane costs 4 reads and 32 registers, 256 VGPRs in all, and ran at 1.6 x the time of
// k_sparse_predict_v); for odd d the entry lane + 64 j (8-byte loads);
//   w^T PC w = w_lo^T S_lo w_lo + w_hi^T S_hi w_hi + 2 w_hi^T C w_lo.
// The data points are taken kStChunk at a time: their rows of W are built in LDS from a and h, every point costs one wavefront
// reduction and no barrier, and the chunk's results leave as one coalesced store.
constexpr int kStChunk = 32;
template <int NJ, bool PAIR>
static __global__ __launch_bounds__(64) void k_st_predict(StArgs a, const double* __restrict__ mu, const double* __restrict__ Sig,
                                                         const double* __restrict__ Sub, double* __restrict__ fmu,
                                                         double* __restrict__ fvar, SparseKl kl) {
    extern __shared__ double sh[];     // W [kStChunk][2d + 1], pair mean [2d], mu_prior - mu [2d]
    const int m = blockIdx.x, d = a.d, d2 = 2 * d, dd = d * d, lane = threadIdx.x;
    const int i0 = a.seg[m], i1 = a.seg[m + 1];
    if (i0 >= i1 && !kl.part) return;
    const int st = d2 + 1;
    double* sh_w = sh;
    double* sh_pm = sh + kStChunk * st;
    double* sh_dv = sh_pm + d2;
    const bool lo_prior = (m == 0), hi_prior = (m == a.M);
    const double* S_lo = lo_prior ? a.prior_cov : Sig + (size_t)(m - 1) * dd;
    const double* S_hi = hi_prior ? a.prior_cov : Sig + (size_t)m * dd;
    const double* C = (lo_prior || hi_prior) ? nullptr : Sub + (size_t)(m - 1) * dd;       // Cov(x_m, x_{m-1})
    constexpr int W = PAIR ? 2 : 1;          // entries per slot
    double lo[NJ][W], hi[NJ][W], cc[NJ][W];
    int row[NJ], col[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int p = lane + 64 * j, e = W * p;
        const bool ok = e < dd;
        row[j] = ok ? e / d : 0;
        col[j] = ok ? e - row[j] * d : 0;
        if constexpr (PAIR) {
            const double2 zero = make_double2(0.0, 0.0);
            const double2 vl = ok ? reinterpret_cast<const double2*>(S_lo)[p] : zero;
            const double2 vh = ok ? reinterpret_cast<const double2*>(S_hi)[p] : zero;
            const double2 vc = (ok && C) ? reinterpret_cast<const double2*>(C)[p] : zero;
            lo[j][0] = vl.x; lo[j][1] = vl.y; hi[j][0] = vh.x; hi[j][1] = vh.y; cc[j][0] = vc.x; cc[j][1] = vc.y;
        } else {
            lo[j][0] = ok ? S_lo[e] : 0.0;
            hi[j][0] = ok ? S_hi[e] : 0.0;
            cc[j][0] = (ok && C) ? C[e] : 0.0;
        }
    }
    if (lane < d2) {
        const bool h = lane >= d;
        const int kk = h ? lane - d : lane;
        sh_pm[lane] = h ? (hi_prior ? a.prior_mean[kk] : mu[(size_t)m * d + kk]) : (lo_prior ? a.prior_mean[kk] : mu[(size_t)(m - 1) * d + kk]);
    }
    if (kl.part) {
        // node m: aD Pd_m . (Sigma_m + dv_m dv_m^T);  pair (m, m-1): 2 aS Ps_{m-1} . (Sigma_{m,m-1} + dv_m dv_{m-1}^T);  dv = mu_prior - mu
        double tr = 0.0, mh = 0.0;
        if (!hi_prior) {
            if (lane < d2) {
                const bool h = lane >= d;
                const int kk = h ? lane - d : lane;
                const size_t t = h ? (size_t)m : (size_t)(lo_prior ? 0 : m - 1);
                sh_dv[lane] = (h || !lo_prior) ? kl.mup[t * d + kk] - mu[t * d + kk] : 0.0;
            }
            __syncthreads();
            const double* Pd = kl.Pd + (size_t)m * dd;
            const double* Ps = lo_prior ? nullptr : kl.Ps + (size_t)(m - 1) * dd;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int e = W * (lane + 64 * j);
                if (e < dd) {
#pragma unroll
                    for (int u = 0; u < W; ++u) {
                        const double pd = kl.aD * Pd[e + u];
                        const double ps = Ps ? 2.0 * kl.aS * Ps[e + u] : 0.0;
                        tr += pd * hi[j][u] + ps * cc[j][u];
                        mh += sh_dv[d + row[j]] * (pd * sh_dv[d + col[j] + u] + ps * sh_dv[col[j] + u]);
                    }
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            tr += __shfl_down(tr, off, 64);
            mh += __shfl_down(mh, off, 64);
        }
        if (lane == 0) {
            kl.part[m] = tr;
            kl.part[a.M + 1 + m] = mh;
        }
    }
    const StStage stage(a, lane, 64);
    for (int c0 = i0; c0 < i1; c0 += kStChunk) {
        const int np = min(kStChunk, i1 - c0);
        __syncthreads();                                   // the previous chunk's readers (and sh_pm's writers)
        stage.rows(a, c0, np, st, sh_w);
        __syncthreads();
        double my_m = 0.0, my_v = 0.0;
        for (int pt = 0; pt < np; ++pt) {
            const double* w = sh_w + pt * st;
            double qv = 0.0;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                double sl = 0.0, sv = 0.0, sc = 0.0;
#pragma unroll
                for (int u = 0; u < W; ++u) {
                    const double wlc = w[col[j] + u];
                    sl = __builtin_fma(lo[j][u], wlc, sl);
                    sv = __builtin_fma(hi[j][u], w[d + col[j] + u], sv);
                    sc = __builtin_fma(cc[j][u], wlc, sc);
                }
                qv += w[row[j]] * sl + w[d + row[j]] * (sv + 2.0 * sc);
            }
            double qm = (lane < d2) ? w[lane] * sh_pm[lane] : 0.0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                qm += __shfl_xor(qm, off, 64);
                qv += __shfl_xor(qv, off, 64);
            }
            if (lane == pt) {
                my_m = qm;
                my_v = qv;
            }
        }
        if (lane < np) {
            fmu[c0 + lane] = my_m;
            fvar[c0 + lane] = a.c[c0 + lane] + my_v;
        }
    }
}

// k_sparse_sites_q (mfgm_sparse.h) with the rows of W built in LDS from a and h: a workgroup of 256 threads takes kSitesQG consecutive
// intervals per round, thread tid owns the packed entries tid, tid + 256, ... of each site, the next round's old values are requested
// before this round's data points are walked.
template <int NE>           // packed entries per thread and site: ceil(QS / 256)
static __global__ __launch_bounds__(256) void k_st_sites_q(StArgs a, const double* __restrict__ g1, const double* __restrict__ g2, double lr,
                                                          double* __restrict__ nat1, double* __restrict__ nat2q) {
    extern __shared__ double sh[];     // kSitesQChunk x (w [2d], g1, g2)
    const int d = a.d, d2 = 2 * d, ET = d * (d + 1) / 2, EF = d * d, QS = 2 * ET + EF;
    const int tid = threadIdx.x, m_hi = a.M + 1;
    int rr[NE], cc[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int e = tid + k * 256;
        int r = 0, c = 0;
        if (e < QS) {
            if (e >= ET && e < ET + EF) {
                r = d + (e - ET) / d;
                c = (e - ET) % d;
            } else {
                const int t = (e < ET) ? e : e - ET - EF;
                int i = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
                while (i * (i + 1) / 2 > t) --i;
                while ((i + 1) * (i + 2) / 2 <= t) ++i;
                const int j = t - i * (i + 1) / 2;
                r = (e < ET) ? i : d + i;
                c = (e < ET) ? j : d + j;
            }
        }
        rr[k] = r;
        cc[k] = c;
    }
    const int st = d2 + 2;
    double old[kSitesQG][NE], nxt[kSitesQG][NE], old1[kSitesQG], nxt1[kSitesQG];
    auto load = [&](int m0, double (&o)[kSitesQG][NE], double (&o1)[kSitesQG]) {
#pragma unroll
        for (int gi = 0; gi < kSitesQG; ++gi) {
            const bool own = (m0 + gi < m_hi);
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                const int e = tid + k * 256;
                o[gi][k] = (own && e < QS) ? nat2q[(size_t)(m0 + gi) * QS + e] : 0.0;
            }
            o1[gi] = (own && tid < d2) ? nat1[(size_t)(m0 + gi) * d2 + tid] : 0.0;
        }
    };
    const StStage stage(a, tid, 256);
    const int mbase = blockIdx.x * (kSitesQG * kSitesQRounds);
    load(mbase, old, old1);
    for (int rd = 0; rd < kSitesQRounds; ++rd) {
        const int m0 = mbase + rd * kSitesQG;
        if (m0 >= m_hi) break;
        if (rd + 1 < kSitesQRounds) load(m0 + kSitesQG, nxt, nxt1);
        double acc[kSitesQG][NE], acc1[kSitesQG];
#pragma unroll
        for (int gi = 0; gi < kSitesQG; ++gi) {
#pragma unroll
            for (int k = 0; k < NE; ++k) acc[gi][k] = 0.0;
            acc1[gi] = 0.0;
        }
        // the data points of the round's sites are one contiguous range: staged through LDS together, kSitesQChunk at a time
        int segv[kSitesQG + 1];
#pragma unroll
        for (int gi = 0; gi <= kSitesQG; ++gi) segv[gi] = a.seg[min(m0 + gi, m_hi)];
        for (int c0 = segv[0]; c0 < segv[kSitesQG]; c0 += kSitesQChunk) {
            const int np = min(kSitesQChunk, segv[kSitesQG] - c0);
            __syncthreads();
            stage.rows(a, c0, np, st, sh);
            if (tid < np) { sh[tid * st + d2] = g1[c0 + tid]; sh[tid * st + d2 + 1] = g2[c0 + tid]; }
            __syncthreads();
#pragma unroll
            for (int gi = 0; gi < kSitesQG; ++gi) {
                const int p0 = max(segv[gi], c0) - c0, p1 = min(segv[gi + 1], c0 + np) - c0;
                for (int pt = p0; pt < p1; ++pt) {
                    const double* w = sh + pt * st;
                    const double gg = w[d2 + 1];
#pragma unroll
                    for (int k = 0; k < NE; ++k) acc[gi][k] = __builtin_fma(gg * w[rr[k]], w[cc[k]], acc[gi][k]);
                    if (tid < d2) acc1[gi] = __builtin_fma(w[d2], w[tid], acc1[gi]);
                }
            }
        }
#pragma unroll
        for (int gi = 0; gi < kSitesQG; ++gi) {
            if (m0 + gi < m_hi) {
#pragma unroll
                for (int k = 0; k < NE; ++k) {
                    const int e = tid + k * 256;
                    if (e < QS) nat2q[(size_t)(m0 + gi) * QS + e] = __builtin_fma(lr, acc[gi][k], (1.0 - lr) * old[gi][k]);
                }
                if (tid < d2) nat1[(size_t)(m0 + gi) * d2 + tid] = __builtin_fma(lr, acc1[gi], (1.0 - lr) * old1[gi]);
            }
#pragma unroll
            for (int k = 0; k < NE; ++k) old[gi][k] = nxt[gi][k];
            old1[gi] = nxt1[gi];
        }
    }
}

}  // namespace mfgm
