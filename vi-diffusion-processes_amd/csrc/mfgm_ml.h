// Local kernels of the multi-latent sparse CVI model (multi_latent_variational.py): sparse CVI on pairs of inducing states whose state
// stacks L independent latent processes (IndependentMultiOutput, D = sum dl), under a likelihood that couples the L latent values of a
// data point through the factorised marginals q(F) = prod_l q(F_l) (MultiStage: markovflow/likelihoods/mutlistage_likelihood.py;
// heteroskedastic Gaussian).  The projections of a point onto its pair of inducing states have disjoint supports -- latent l owns the
// slots off_l .. off_l + dl[l] of both halves -- so ONE row h_i [2D] carries all L of them, and the site of an interval is block-diagonal
// over latents:
//
//   k_ml_predict_lik : q(F_l(t_i)) for every latent from the within-latent blocks of the pair marginal, the coupled likelihood at those
//                      very values (VE_i, g1 [L], g2 [L]) and the interval's sum of VE_i, in one launch
//   k_ml_sites       : sites <- (1 - lr) sites + lr sum_i (g1[i, l(r)] h_ir, g2[i, l] h_ir h_ic), cross-latent entries decay only; on the
//                      dense [2D, 2D] site or on the quadrant-packed one
//
// Intervals, seg and the prior padding at both ends are those of mfgm_sparse.h.  No atomics: one owner per output entry and a fixed
// order of summation, so two launches on the same inputs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "mfgm_lik.h"

namespace mfgm {

constexpr int kMlMaxL = 8;

struct MlArgs {
    int M, L, N, D;
    int dl[kMlMaxL], off[kMlMaxL];
    const int* seg;            // [M + 2]
    const double* h;           // [N, 2D]
    const double* c;           // [N, L]
    const double* prior_mean;  // [D]
    const double* prior_cov;   // [D, D]
};

struct MlLik {
    int kind;                  // 0 none, 1 MultiStage (p0 = jitter, p1 = bin size), 2 heteroskedastic Gaussian
    double p0, p1;
};

constexpr double kMlLog2Pi = 1.83787706640934548356;

// The coupled likelihoods at the factorised marginals (m, v) [L] of one point: VE, dVE/dm_l, dVE/dv_l.  A latent that does not enter
// the point's case keeps (0, 0).
MFGM_DEV void ml_multistage(const double (&m)[3], const double (&v)[3], double y, double jit, double binsize, double& ve,
                            double (&dm)[3], double (&dv)[3]) {
    ve = 0.0;
#pragma unroll
    for (int l = 0; l < 3; ++l) dm[l] = dv[l] = 0.0;
    const bool is0 = (y == 0.0), is1 = (y == 1.0), big = (y >= 2.0);
    if (!(is0 || is1 || big)) return;          // negative, NaN, non-integer below 2: nothing (the reference's where-chain)
    double e, a, b;
    lik_bernoulli(m[0], v[0], is0 ? 1.0 : 0.0, jit, e, a, b);
    ve += e; dm[0] = a; dv[0] = b;
    if (is0) return;
    lik_bernoulli(m[1], v[1], is1 ? 1.0 : 0.0, jit, e, a, b);
    ve += e; dm[1] = a; dv[1] = b;
    if (is1) return;
    lik_poisson(m[2], v[2], y - 2.0, binsize, e, a, b);
    ve += e; dm[2] = a; dv[2] = b;
}

// y ~ N(F0, exp F1):  VE = -1/2 [log 2 pi + m1 + exp(-m1 + v1 / 2) ((m0 - y)^2 + v0)]
MFGM_DEV void ml_hetgauss(const double (&m)[3], const double (&v)[3], double y, double& ve, double (&dm)[3], double (&dv)[3]) {
    const double s = exp(-m[1] + 0.5 * v[1]);
    const double r = m[0] - y;
    const double q = r * r + v[0];
    ve = -0.5 * (kMlLog2Pi + m[1] + s * q);
    dm[0] = -s * r;
    dv[0] = -0.5 * s;
    dm[1] = -0.5 + 0.5 * s * q;
    dv[1] = -0.25 * s * q;
    dm[2] = dv[2] = 0.0;
}

// One wavefront per group of G consecutive intervals (G chosen by the host from the LDS the blocks need: 32 for small D, 1 at
// D = 32 with one latent), one lane per data point, 64 at a time over the group's contiguous range of points -- with two points per
// interval, as on config 5's shape, a wavefront per interval would run the 20-point rules of MultiStage on 2 lanes of 64.  LDS: for
// the G + 1 inducing states around the group (the prior's initial state at both ends of the chain) the within-latent blocks of their
// covariances (sum dl^2 doubles each) and their means, for every interval the same blocks of C = Sigma_{m,m-1}, and the chunk's rows
// of h (stride 2D + 1: a lane walks its own row without bank conflicts):
//   h^T PC h = h_lo^T S_lo h_lo + h_hi^T S_hi h_hi + 2 h_hi^T C h_lo   per latent.
// A lane finds the interval of its point by bisection in the group's CSR offsets.  The intervals' VE sums: the chunk's VE_i go through
// LDS and lane g adds those of interval g in point order -- a fixed order, whatever the grouping.
constexpr int kMlChunk = 64;
constexpr int kMlMaxGroup = 32;
template <int KIND>
static __global__ __launch_bounds__(64) void k_ml_predict_lik(MlArgs a, MlLik lik, int G, const double* __restrict__ y,
                                                             const double* __restrict__ mu, const double* __restrict__ Sig,
                                                             const double* __restrict__ Sub, double* __restrict__ fmu,
                                                             double* __restrict__ fvar, double* __restrict__ ve_part,
                                                             double* __restrict__ g1, double* __restrict__ g2) {
    extern __shared__ double sh[];
    const int D = a.D, D2 = 2 * D, L = a.L, lane = threadIdx.x;
    const int m0 = blockIdx.x * G, Gc = min(G, a.M + 1 - m0);          // intervals m0 .. m0 + Gc
    const int i0 = a.seg[m0], i1 = a.seg[m0 + Gc];
    if (i0 >= i1) {
        if (KIND != 0 && ve_part && lane < Gc) ve_part[m0 + lane] = 0.0;
        return;
    }
    int nblk = 0;
    for (int l = 0; l < L; ++l) nblk += a.dl[l] * a.dl[l];
    const int st = D2 + 1;
    double* sh_nc = sh;                              // [G + 1][nblk]  node covariances, node m0 - 1 + s at slot s
    double* sh_cc = sh_nc + (G + 1) * nblk;          // [G][nblk]      Cov(x_m, x_{m-1}) of interval m0 + g at slot g
    double* sh_nm = sh_cc + G * nblk;                // [G + 1][D]     node means
    double* sh_h = sh_nm + (G + 1) * D;              // [kMlChunk][2D + 1]
    double* sh_ve = sh_h + kMlChunk * st;            // [kMlChunk]
    int* sh_seg = reinterpret_cast<int*>(sh_ve + kMlChunk);          // [G + 1]
    for (int s = lane; s <= Gc; s += 64) sh_seg[s] = a.seg[m0 + s];
    {
        int b0 = 0;
        for (int l = 0; l < L; ++l) {
            const int n = a.dl[l], nn = n * n, o = a.off[l];
            for (int e = lane; e < (2 * Gc + 1) * nn; e += 64) {
                const int s = e / nn, k = e - s * nn, r = k / n, c = k - r * n;
                const size_t g = (size_t)(o + r) * D + o + c;
                if (s <= Gc) {
                    const int node = m0 - 1 + s;
                    const double* S = (node < 0 || node >= a.M) ? a.prior_cov : Sig + (size_t)node * D * D;
                    sh_nc[s * nblk + b0 + k] = S[g];
                } else {
                    const int gi = s - Gc - 1, m = m0 + gi;
                    sh_cc[gi * nblk + b0 + k] = (m > 0 && m < a.M) ? Sub[(size_t)(m - 1) * D * D + g] : 0.0;
                }
            }
            b0 += nn;
        }
    }
    for (int e = lane; e < (Gc + 1) * D; e += 64) {
        const int s = e / D, k = e - s * D, node = m0 - 1 + s;
        sh_nm[e] = (node < 0 || node >= a.M) ? a.prior_mean[k] : mu[(size_t)node * D + k];
    }
    double ve_acc = 0.0;          // lane g: interval m0 + g
    for (int c0 = i0; c0 < i1; c0 += kMlChunk) {
        const int np = min(kMlChunk, i1 - c0);
        __syncthreads();                                   // the previous chunk's readers (and the writers of the blocks)
        for (int e = lane; e < np * D2; e += 64) {         // the chunk's rows are contiguous: coalesced
            const int pt = e / D2;
            sh_h[pt * st + (e - pt * D2)] = a.h[(size_t)c0 * D2 + e];
        }
        __syncthreads();
        if (lane < np) {
            const size_t i = (size_t)(c0 + lane);
            int gi = 0, hi_g = Gc;                         // the last g with seg[g] <= i: its interval holds i (i < seg[Gc])
            while (hi_g - gi > 1) {
                const int mid = (gi + hi_g) >> 1;
                if (sh_seg[mid] <= (int)i) gi = mid; else hi_g = mid;
            }
            const double* w = sh_h + lane * st;
            double m3[3] = {0.0, 0.0, 0.0}, v3[3] = {1.0, 1.0, 1.0};
            int b0 = 0;
            constexpr int LMAX = (KIND == 1) ? 3 : (KIND == 2) ? 2 : kMlMaxL;          // the host checks L against the kind
#pragma unroll
            for (int l = 0; l < LMAX; ++l) {
                if (l < L) {
                    const int n = a.dl[l];
                    const double* wl = w + a.off[l];
                    const double* wh = wl + D;
                    const double* pl = sh_nm + gi * D + a.off[l];
                    const double* lo = sh_nc + gi * nblk + b0;
                    const double* hi = lo + nblk;
                    const double* cc = sh_cc + gi * nblk + b0;
                    double qm = 0.0, qv = 0.0;
                    for (int r = 0; r < n; ++r) {
                        double sl = 0.0, sv = 0.0, sc = 0.0;
                        for (int c = 0; c < n; ++c) {
                            sl = __builtin_fma(lo[r * n + c], wl[c], sl);
                            sv = __builtin_fma(hi[r * n + c], wh[c], sv);
                            sc = __builtin_fma(cc[r * n + c], wl[c], sc);
                        }
                        qv += wl[r] * sl + wh[r] * (sv + 2.0 * sc);
                        qm = __builtin_fma(wl[r], pl[r], qm);
                        qm = __builtin_fma(wh[r], pl[D + r], qm);
                    }
                    const double fv = a.c[i * L + l] + qv;
                    if (fmu) fmu[i * L + l] = qm;
                    if (fvar) fvar[i * L + l] = fv;
                    if (l < 3) {
                        m3[l] = qm;
                        v3[l] = fv;
                    }
                    b0 += n * n;
                }
            }
            if (KIND != 0) {
                double ve, dm[3], dv[3];
                if (KIND == 1)
                    ml_multistage(m3, v3, y[i], lik.p0, lik.p1, ve, dm, dv);
                else
                    ml_hetgauss(m3, v3, y[i], ve, dm, dv);
                sh_ve[lane] = ve;
#pragma unroll
                for (int l = 0; l < 3; ++l) {
                    if (l < L) {
                        if (g1) g1[i * L + l] = dm[l] - 2.0 * dv[l] * m3[l];
                        if (g2) g2[i * L + l] = dv[l];
                    }
                }
            }
        }
        if (KIND != 0 && ve_part) {
            __syncthreads();
            if (lane < Gc) {
                const int p0 = max(sh_seg[lane], c0) - c0, p1 = min(sh_seg[lane + 1], c0 + np) - c0;
                for (int pt = p0; pt < p1; ++pt) ve_acc += sh_ve[pt];
            }
        }
    }
    if (KIND != 0 && ve_part && lane < Gc) ve_part[m0 + lane] = ve_acc;
}

// One workgroup of 256 threads per interval; thread tid owns the entries tid, tid + 256, ... of the interval's nat2 (dense [2D, 2D],
// PACKED = false, or quadrant-packed, PACKED = true) and, for tid < 2D, entry tid of nat1.  An entry (r, c) whose slots belong to the
// same latent l accumulates g2[i, l] h_i[max] h_i[min] -- the same product for (r, c) and (c, r), so the dense form is symmetric to the
// bit; one whose slots belong to different latents accumulates nothing and leaves as (1 - lr) old exactly.  The interval's points go
// through LDS kMlSitesChunk at a time: row [h (2D) | g1 (L) | g2 (L)].
constexpr int kMlSitesChunk = 32;
template <int NE, bool PACKED>
static __global__ __launch_bounds__(256) void k_ml_sites(MlArgs a, const double* __restrict__ g1, const double* __restrict__ g2, double lr,
                                                        double* __restrict__ nat1, double* __restrict__ nat2) {
    extern __shared__ double sh[];     // kMlSitesChunk x (h [2D], g1 [L], g2 [L]), then the latent of every slot as int [2D]
    const int D = a.D, D2 = 2 * D, L = a.L, tid = threadIdx.x, m = blockIdx.x;
    const int ET = D * (D + 1) / 2, EF = D * D;
    const int QS = PACKED ? 2 * ET + EF : D2 * D2;
    const int st = D2 + 2 * L;
    int* sh_lat = reinterpret_cast<int*>(sh + kMlSitesChunk * st);
    for (int k = tid; k < D2; k += 256) {
        const int s = (k >= D) ? k - D : k;
        int l = 0;
        while (l + 1 < L && s >= a.off[l + 1]) ++l;
        sh_lat[k] = l;
    }
    __syncthreads();
    int rr[NE], cc[NE], gg[NE];          // gg: index of the entry's g2 within a staged row, or -1
    double old[NE], acc[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int e = tid + k * 256;
        int r = 0, c = 0;
        if (e < QS) {
            if (!PACKED) {
                r = e / D2;
                c = e - r * D2;
            } else if (e >= ET && e < ET + EF) {
                r = D + (e - ET) / D;
                c = (e - ET) % D;
            } else {
                const int t = (e < ET) ? e : e - ET - EF;
                int i = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
                while (i * (i + 1) / 2 > t) --i;
                while ((i + 1) * (i + 2) / 2 <= t) ++i;
                const int j = t - i * (i + 1) / 2;
                r = (e < ET) ? i : D + i;
                c = (e < ET) ? j : D + j;
            }
        }
        rr[k] = max(r, c);
        cc[k] = min(r, c);
        gg[k] = (e < QS && sh_lat[r] == sh_lat[c]) ? D2 + L + sh_lat[r] : -1;
        old[k] = (e < QS) ? nat2[(size_t)m * QS + e] : 0.0;
        acc[k] = 0.0;
    }
    const bool own1 = tid < D2;
    const int g1at = own1 ? D2 + sh_lat[tid] : 0;
    const double old1 = own1 ? nat1[(size_t)m * D2 + tid] : 0.0;
    double acc1 = 0.0;
    const int i0 = a.seg[m], i1 = a.seg[m + 1];
    for (int c0 = i0; c0 < i1; c0 += kMlSitesChunk) {
        const int np = min(kMlSitesChunk, i1 - c0);
        __syncthreads();
        for (int e = tid; e < np * D2; e += 256) {
            const int pt = e / D2;
            sh[pt * st + (e - pt * D2)] = a.h[(size_t)c0 * D2 + e];
        }
        for (int e = tid; e < np * L; e += 256) {
            const int pt = e / L, l = e - pt * L;
            sh[pt * st + D2 + l] = g1[(size_t)c0 * L + e];
            sh[pt * st + D2 + L + l] = g2[(size_t)c0 * L + e];
        }
        __syncthreads();
        for (int pt = 0; pt < np; ++pt) {
            const double* w = sh + pt * st;
#pragma unroll
            for (int k = 0; k < NE; ++k)
                if (gg[k] >= 0) acc[k] = __builtin_fma(w[gg[k]] * w[rr[k]], w[cc[k]], acc[k]);
            if (own1) acc1 = __builtin_fma(w[g1at], w[tid], acc1);
        }
    }
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int e = tid + k * 256;
        if (e < QS) nat2[(size_t)m * QS + e] = __builtin_fma(lr, acc[k], (1.0 - lr) * old[k]);
    }
    if (own1) nat1[(size_t)m * D2 + tid] = __builtin_fma(lr, acc1, (1.0 - lr) * old1);
}

}  // namespace mfgm
