// Local kernels of the factor-analysis sparse CVI model (factor_analysis_variational.py; markovflow/kernels/sde_kernel.py:881,
// FactorAnalysisKernel): sparse CVI on pairs of inducing states whose state stacks L independent latent processes g_l (D = sum dl, the
// layout of mfgm_ml.h), observed through P outputs that MIX the latents, f_p(t_i) = sum_l W_ipl g_l(t_i).  The mixing makes the marginal
// of an output depend on the cross-latent blocks of the pair covariance and the site of an interval dense across latents; both enter
// through L x L matrices only:
//
//   k_fa_predict_lik : the latent marginal of every point, a_i [L] and K_i [L, L] (all L (L + 1) / 2 blocks of h^T PC h), the output
//                      marginals fmu = W a, fvar = W K W^T, the scalar likelihood of every output at those very values, and the
//                      gradients folded back into latent space, gam1_i [L], gam2_i [L, L] -- one launch, (2D)^2 + P L^2 multiply-adds
//                      per point instead of the P (2D)^2 of P materialised rows
//   k_fa_sites       : sites <- (1 - lr) sites + lr sum_i (gam1[i, l(r)] h_ir, gam2_i[l(r), l(c)] h_ir h_ic), every entry accumulating;
//                      on the dense [2D, 2D] site or on the quadrant-packed one.  The weights are not read: they are inside gam.
//
// Symmetric L x L matrices travel as their lower triangle, row-major: (l, l') with l' <= l at l (l + 1) / 2 + l'.  Intervals, seg and the
// prior padding at both ends are those of mfgm_sparse.h.  No atomics: one owner per output entry and a fixed order of summation, so
// two launches on the same inputs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "mfgm_lik.h"

namespace mfgm {

constexpr int kFaMaxL = 8;
constexpr int kFaMaxP = 64;

struct FaArgs {
    int M, L, P, N, D;
    int dl[kFaMaxL], off[kFaMaxL];
    const int* seg;            // [M + 2]
    const double* h;           // [N, 2D]
    const double* c;           // [N, L]
    const double* w;           // [P, L] (w_stride 0) or [N, P, L] (w_stride P L)
    long long w_stride;
    const double* prior_mean;  // [D]
    const double* prior_cov;   // [D, D]
};

struct FaLik {                 // per output: MFGM_LIK_BERNOULLI 1, MFGM_LIK_POISSON 2, MFGM_LIK_GAUSSIAN 3 (0 everywhere: none)
    int kind[kFaMaxP];
    double param[kFaMaxP];
};

constexpr double kFaLog2Pi = 1.83787706640934548356;

// One wavefront per group of G consecutive intervals (G chosen by the host from the LDS the blocks need), one lane per data point, 64
// at a time over the group's contiguous range of points (the launch shape of k_ml_predict_lik).  LDS: for the G + 1 inducing states
// around the group (the prior's initial state at both ends of the chain) their FULL covariances and means, for every interval the full
// C = Sigma_{m,m-1}, the chunk's rows of h (stride 2D + 1), and, with time-invariant weights, W [P, L].  The stride between two nodes'
// blocks is odd, so lanes of different intervals that read the same element of their own block hit different banks; lanes of one
// interval read one address (a broadcast).  With PC = [[S_lo, C^T], [C, S_hi]] the block (l, l') of the quadratic form is
//   K[l, l'] = sum_{r in l, s in l'} h_lo[r] (S_lo[r][s] h_lo[s] + C[s][r] h_hi[s]) + h_hi[r] (S_hi[r][s] h_hi[s] + C[r][s] h_lo[s]),
// taken for l' <= l.  a [L], K [LT] and the accumulators gam1 [L], gam2 [LT] live in registers: every loop over latents is unrolled to
// LMAX with constant indices (an index known only at run time would move the arrays to scratch), the loops over the slots of a
// latent and over the outputs are not.  The output loop is wave-uniform: kind and parameter come from the kernel arguments.
constexpr int kFaChunk = 64;
constexpr int kFaMaxGroup = 32;
template <int LMAX, bool LIK, bool WCONST>
static __global__ __launch_bounds__(64) void k_fa_predict_lik(FaArgs a, FaLik lik, int G, const double* __restrict__ y,
                                                             const double* __restrict__ mu, const double* __restrict__ Sig,
                                                             const double* __restrict__ Sub, double* __restrict__ fmu,
                                                             double* __restrict__ fvar, double* __restrict__ lmu,
                                                             double* __restrict__ lcov, double* __restrict__ ve_part,
                                                             double* __restrict__ dm_out, double* __restrict__ dv_out,
                                                             double* __restrict__ gam1, double* __restrict__ gam2) {
    extern __shared__ double sh[];
    constexpr int LTMAX = LMAX * (LMAX + 1) / 2;
    const int D = a.D, D2 = 2 * D, L = a.L, P = a.P, LT = L * (L + 1) / 2, lane = threadIdx.x;
    const int m0 = blockIdx.x * G, Gc = min(G, a.M + 1 - m0);          // intervals m0 .. m0 + Gc
    const int i0 = a.seg[m0], i1 = a.seg[m0 + Gc];
    if (i0 >= i1) {
        if (LIK && ve_part && lane < Gc) ve_part[m0 + lane] = 0.0;
        return;
    }
    const int DD = D * D, NB = DD | 1, st = D2 + 1;
    double* sh_nc = sh;                              // [G + 1][NB]  node covariances, node m0 - 1 + s at slot s
    double* sh_cc = sh_nc + (G + 1) * NB;            // [G][NB]      Cov(x_m, x_{m-1}) of interval m0 + g at slot g
    double* sh_nm = sh_cc + G * NB;                  // [G + 1][D]   node means
    double* sh_h = sh_nm + (G + 1) * D;              // [kFaChunk][2D + 1]
    double* sh_ve = sh_h + kFaChunk * st;            // [kFaChunk]
    double* sh_w = sh_ve + kFaChunk;                 // [P L] (WCONST)
    int* sh_seg = reinterpret_cast<int*>(sh_w + (WCONST ? P * L : 0));          // [G + 1]
    for (int s = lane; s <= Gc; s += 64) sh_seg[s] = a.seg[m0 + s];
    for (int e = lane; e < (2 * Gc + 1) * DD; e += 64) {
        const int s = e / DD, k = e - s * DD;
        if (s <= Gc) {
            const int node = m0 - 1 + s;
            const double* S = (node < 0 || node >= a.M) ? a.prior_cov : Sig + (size_t)node * DD;
            sh_nc[s * NB + k] = S[k];
        } else {
            const int gi = s - Gc - 1, m = m0 + gi;
            sh_cc[gi * NB + k] = (m > 0 && m < a.M) ? Sub[(size_t)(m - 1) * DD + k] : 0.0;
        }
    }
    for (int e = lane; e < (Gc + 1) * D; e += 64) {
        const int s = e / D, k = e - s * D, node = m0 - 1 + s;
        sh_nm[e] = (node < 0 || node >= a.M) ? a.prior_mean[k] : mu[(size_t)node * D + k];
    }
    if (WCONST)
        for (int e = lane; e < P * L; e += 64) sh_w[e] = a.w[e];
    double ve_acc = 0.0;          // lane g: interval m0 + g
    for (int c0 = i0; c0 < i1; c0 += kFaChunk) {
        const int np = min(kFaChunk, i1 - c0);
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
            const double* hl = sh_h + lane * st;           // the lower state's half of the row; the upper state's is hl + D
            const double* hh = hl + D;
            const double* Slo = sh_nc + gi * NB;
            const double* Shi = Slo + NB;
            const double* C = sh_cc + gi * NB;
            const double* ml = sh_nm + gi * D;
            double av[LMAX], K[LTMAX];
#pragma unroll
            for (int l = 0; l < LMAX; ++l) {
                av[l] = 0.0;
                if (l < L) {
                    const int n = a.dl[l], o = a.off[l];
                    double q = 0.0;
                    for (int r = o; r < o + n; ++r) {
                        q = __builtin_fma(hl[r], ml[r], q);
                        q = __builtin_fma(hh[r], ml[D + r], q);
                    }
                    av[l] = q;
#pragma unroll
                    for (int k = 0; k <= l; ++k) {
                        const int nk = a.dl[k], ok = a.off[k];
                        double acc = 0.0;
                        for (int r = o; r < o + n; ++r) {
                            double sl = 0.0, su = 0.0;
                            for (int s = ok; s < ok + nk; ++s) {
                                sl = __builtin_fma(Slo[r * D + s], hl[s], sl);
                                sl = __builtin_fma(C[s * D + r], hh[s], sl);
                                su = __builtin_fma(Shi[r * D + s], hh[s], su);
                                su = __builtin_fma(C[r * D + s], hl[s], su);
                            }
                            acc = __builtin_fma(hl[r], sl, acc);
                            acc = __builtin_fma(hh[r], su, acc);
                        }
                        if (k == l) acc += a.c[i * L + l];
                        K[tix(l, k)] = acc;
                        if (lcov) lcov[i * LT + tix(l, k)] = acc;
                    }
                    if (lmu) lmu[i * L + l] = q;
                } else {
#pragma unroll
                    for (int k = 0; k <= l; ++k) K[tix(l, k)] = 0.0;
                }
            }
            double g1a[LMAX], g2a[LTMAX], ve_i = 0.0;
            if (LIK) {
#pragma unroll
                for (int l = 0; l < LMAX; ++l) g1a[l] = 0.0;
#pragma unroll
                for (int e = 0; e < LTMAX; ++e) g2a[e] = 0.0;
            }
            const double* wrow = WCONST ? sh_w : a.w + i * (size_t)a.w_stride;
#pragma unroll 1
            for (int p = 0; p < P; ++p) {
                double wl[LMAX];
#pragma unroll
                for (int l = 0; l < LMAX; ++l) wl[l] = (l < L) ? wrow[p * L + l] : 0.0;
                double fm = 0.0, fv = 0.0;
#pragma unroll
                for (int l = 0; l < LMAX; ++l) {
                    fm = __builtin_fma(wl[l], av[l], fm);
                    double t = 0.0;                        // sum_k W_k K[l, k] over all k, through the stored triangle
#pragma unroll
                    for (int k = 0; k < LMAX; ++k) t = __builtin_fma(wl[k], K[six(l, k)], t);
                    fv = __builtin_fma(wl[l], t, fv);
                }
                if (fmu) fmu[i * P + p] = fm;
                if (fvar) fvar[i * P + p] = fv;
                if (LIK) {
                    const double yraw = y[i * P + p];
                    const bool seen = (yraw == yraw);
                    const double yy = seen ? yraw : 0.0;
                    const int kind = lik.kind[p];
                    const double prm = lik.param[p];
                    double ve, dm, dv;
                    if (kind == 1) {
                        lik_bernoulli(fm, fv, yy, prm, ve, dm, dv);
                    } else if (kind == 2) {
                        lik_poisson(fm, fv, yy, prm, ve, dm, dv);
                    } else {
                        const double r = yy - fm, is2 = 1.0 / prm;
                        ve = -0.5 * (kFaLog2Pi + log(prm)) - 0.5 * (r * r + fv) * is2;
                        dm = r * is2;
                        dv = -0.5 * is2;
                    }
                    ve = seen ? ve : 0.0;
                    dm = seen ? dm : 0.0;
                    dv = seen ? dv : 0.0;
                    if (dm_out) dm_out[i * P + p] = dm;
                    if (dv_out) dv_out[i * P + p] = dv;
                    ve_i += ve;
                    const double g = seen ? dm - 2.0 * dv * fm : 0.0;
#pragma unroll
                    for (int l = 0; l < LMAX; ++l) {
                        g1a[l] = __builtin_fma(g, wl[l], g1a[l]);
                        const double dw = dv * wl[l];
#pragma unroll
                        for (int k = 0; k <= l; ++k) g2a[tix(l, k)] = __builtin_fma(dw, wl[k], g2a[tix(l, k)]);
                    }
                }
            }
            if (LIK) {
                sh_ve[lane] = ve_i;
#pragma unroll
                for (int l = 0; l < LMAX; ++l) {
                    if (l < L) {
                        if (gam1) gam1[i * L + l] = g1a[l];
                        if (gam2) {
#pragma unroll
                            for (int k = 0; k <= l; ++k) gam2[i * LT + tix(l, k)] = g2a[tix(l, k)];
                        }
                    }
                }
            }
        }
        if (LIK && ve_part) {
            __syncthreads();
            if (lane < Gc) {
                const int p0 = max(sh_seg[lane], c0) - c0, p1 = min(sh_seg[lane + 1], c0 + np) - c0;
                for (int pt = p0; pt < p1; ++pt) ve_acc += sh_ve[pt];
            }
        }
    }
    if (LIK && ve_part && lane < Gc) ve_part[m0 + lane] = ve_acc;
}

// One workgroup of 256 threads per interval; thread tid owns the entries tid, tid + 256, ... of the interval's nat2 (dense [2D, 2D],
// PACKED = false, or quadrant-packed, PACKED = true) and, for tid < 2D, entry tid of nat1 (the ownership of k_ml_sites).  Entry (r, c)
// accumulates gam2_i[l(r), l(c)] h_i[max(r, c)] h_i[min(r, c)] -- the same three factors in the same order for (r, c) and (c, r), so
// the dense form is symmetric to the bit.  The interval's points go through LDS kFaSitesChunk at a time:
// row [h (2D) | gam1 (L) | gam2 (LT)].
constexpr int kFaSitesChunk = 32;
template <int NE, bool PACKED>
static __global__ __launch_bounds__(256) void k_fa_sites(FaArgs a, const double* __restrict__ gam1, const double* __restrict__ gam2,
                                                        double lr, double* __restrict__ nat1, double* __restrict__ nat2) {
    extern __shared__ double sh[];     // kFaSitesChunk x (h [2D], gam1 [L], gam2 [LT]), then the latent of every slot as int [2D]
    const int D = a.D, D2 = 2 * D, L = a.L, LT = L * (L + 1) / 2, tid = threadIdx.x, m = blockIdx.x;
    const int ET = D * (D + 1) / 2, EF = D * D;
    const int QS = PACKED ? 2 * ET + EF : D2 * D2;
    const int st = D2 + L + LT;
    int* sh_lat = reinterpret_cast<int*>(sh + kFaSitesChunk * st);
    for (int k = tid; k < D2; k += 256) {
        const int s = (k >= D) ? k - D : k;
        int l = 0;
        while (l + 1 < L && s >= a.off[l + 1]) ++l;
        sh_lat[k] = l;
    }
    __syncthreads();
    int rr[NE], cc[NE], gg[NE];          // gg: index of the entry's gam2 within a staged row
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
        const int la = sh_lat[r], lb = sh_lat[c];
        gg[k] = D2 + L + tix(max(la, lb), min(la, lb));
        old[k] = (e < QS) ? nat2[(size_t)m * QS + e] : 0.0;
        acc[k] = 0.0;
    }
    const bool own1 = tid < D2;
    const int g1at = own1 ? D2 + sh_lat[tid] : 0;
    const double old1 = own1 ? nat1[(size_t)m * D2 + tid] : 0.0;
    double acc1 = 0.0;
    const int i0 = a.seg[m], i1 = a.seg[m + 1];
    for (int c0 = i0; c0 < i1; c0 += kFaSitesChunk) {
        const int np = min(kFaSitesChunk, i1 - c0);
        __syncthreads();
        for (int e = tid; e < np * D2; e += 256) {
            const int pt = e / D2;
            sh[pt * st + (e - pt * D2)] = a.h[(size_t)c0 * D2 + e];
        }
        for (int e = tid; e < np * L; e += 256) {
            const int pt = e / L;
            sh[pt * st + D2 + (e - pt * L)] = gam1[(size_t)c0 * L + e];
        }
        for (int e = tid; e < np * LT; e += 256) {
            const int pt = e / LT;
            sh[pt * st + D2 + L + (e - pt * LT)] = gam2[(size_t)c0 * LT + e];
        }
        __syncthreads();
        for (int pt = 0; pt < np; ++pt) {
            const double* w = sh + pt * st;
#pragma unroll
            for (int k = 0; k < NE; ++k) acc[k] = __builtin_fma(w[gg[k]] * w[rr[k]], w[cc[k]], acc[k]);
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
