// Sparse Power Expectation Propagation: the fused site update of the sites-on-inducing-state-pairs model (include/mfgm.h,
// mfgm_sparse_pep_sites[_q]; markovflow/models/sparse_pep.py with the differences DESIGN.md section 14 lists).
//
// Every data point of an interval removes the same fraction beta = alpha / n_m of the same site, so the cavity belongs to the
// INTERVAL: two [2d, 2d] factorisations per interval, not per data point.  With n = 2d, per interval m that holds data, from the pair
// marginal N(mu, S) (assembled from the marginal blocks as k_cond_predict does) and the site (nat1, nat2):
//   S = L L^T,  Li = L^-1,  Lam = Li^T Li,  u = Li mu,  h = Li^T u,  g_q = 1/2 (log det S + |u|^2)
//   Lc = chol(Lam + 2 beta nat2),  Lci = Lc^-1,  uc = Lci (h - beta nat1),  g_c = 1/2 (-log det Lam_c + |uc|^2)
//   per point i:  t = Lci w_i,  s = |t|^2,  mc = t . uc,  (log Z, d1, d2) = pep_tilted(mc, s + c_i),
//                 L2 = 1/2 / (s + 1/d2),  L1 = 2 L2 (d1/d2 - mc),  e_i = log Z + g_c - g_q
//   X <- (1 - lr) X + lr ((1 - alpha) X + sum_i dX_i),  X = (nat1, nat2, lnorm),  dX_i = (L1 w_i, L2 w_i w_i^T, e_i)
// (the cavity covariance Sc = Lci^T Lci is never formed: w^T Sc w = |Lci w|^2 and w^T Sc hc = (Lci w) . (Lci hc)).
//
// Mapping: one wavefront per workgroup; NP = 2d rounded up to a power of two lanes per interval, 64 / NP consecutive intervals per
// wavefront, each with its own LDS region: the n x (n + 1) matrix that is factorised and inverted in place (lower triangle; the upper
// triangle receives Lam), three vectors, and kSpepChunk staged data points (w, t).  The factorisations run lanes-over-rows, the
// inverses and products lanes-over-columns, the tilted moments lanes-over-points, the site read-modify-write lanes-over-columns of one
// site row at a time.  An interval with more than kSpepChunk points takes one further read-modify-write of its site per extra chunk.
#pragma once
#include <hip/hip_runtime.h>

#include "mfgm_pep.h"
#include "mfgm_sparse.h"

namespace mfgm {

constexpr int kSpepChunk = 8;      // data points of an interval staged through LDS at a time

// doubles of LDS per interval: matrix, diag / v1 / v2, w and t chunks, (L1, L2, y, c) per staged point
MFGM_HD size_t spep_lds_doubles(int n) { return (size_t)n * (n + 1) + 3 * (size_t)n + 2 * (size_t)kSpepChunk * n + 4 * kSpepChunk; }

// index of entry (r, c), r >= c, of a symmetric [2d, 2d] site in the quadrant-packed form (include/mfgm.h)
MFGM_DEV int spep_qidx(int r, int c, int d) {
    const int ET = d * (d + 1) / 2;
    if (r < d) return r * (r + 1) / 2 + c;
    if (c < d) return ET + (r - d) * d + c;
    return ET + d * d + (r - d) * (r - d + 1) / 2 + (c - d);
}

// In-place Cholesky factor of the lower triangle of A (stride st) by the NP lanes of an interval, lanes over rows; returns
// sum log L_ii, clears ok when a pivot is not positive.  Called by every lane of the wavefront.
template <int NP>
MFGM_DEV double spep_cholesky(double* A, int n, int st, int l, bool& ok) {
    double ld = 0.0;
    for (int j = 0; j < n; ++j) {
        double s = 0.0;
        if (l >= j && l < n) {
            s = A[l * st + j];
            for (int k = 0; k < j; ++k) s = __builtin_fma(-A[l * st + k], A[j * st + k], s);
        }
        const double piv = __shfl(s, j, NP);
        if (!(piv > 0.0) || !isfinite(piv)) ok = false;
        const double ljj = sqrt(piv);
        __syncthreads();
        if (l >= j && l < n) A[l * st + j] = (l == j) ? ljj : s / ljj;
        __syncthreads();
        ld += log(ljj);
    }
    return ld;
}

// In-place inverse of the lower-triangular factor, row by row, lanes over columns
MFGM_DEV void spep_tri_inverse(double* A, int n, int st, int l) {
    for (int i = 0; i < n; ++i) {
        double x = 0.0;
        if (l <= i) {
            const double dii = A[i * st + i];
            if (l == i) x = 1.0 / dii;
            else {
                double s = 0.0;
                for (int k = l; k < i; ++k) s = __builtin_fma(A[i * st + k], A[k * st + l], s);
                x = -s / dii;
            }
        }
        __syncthreads();
        if (l <= i) A[i * st + l] = x;
        __syncthreads();
    }
}

// nat2 is the dense [M + 1, 2d, 2d] tensor (packed == 0) or the quadrant-packed [M + 1, d (d + 1) + d^2] one (packed != 0)
template <int KIND, int NP>
static __global__ __launch_bounds__(64) void k_spep_sites(SparseArgs a, int packed, const double* __restrict__ y, double param, double alpha,
                                                         double lr, const double* __restrict__ mu, const double* __restrict__ Sig,
                                                         const double* __restrict__ Sub, double* __restrict__ nat1,
                                                         double* __restrict__ nat2, double* __restrict__ lnorm,
                                                         double* __restrict__ e_out, int* __restrict__ skipped) {
    constexpr int G = 64 / NP;
    extern __shared__ double sh[];
    const int d = a.d, n = 2 * d, st = n + 1;
    const int sub = threadIdx.x / NP, l = threadIdx.x % NP;
    const int m = a.m_lo + (int)blockIdx.x * G + sub;
    const bool own = m < a.m_hi;
    const int i0 = own ? a.seg[m - a.m_lo] : 0, cnt = own ? a.seg[m - a.m_lo + 1] - i0 : 0;
    double* A = sh + (size_t)sub * spep_lds_doubles(n);
    double* dg = A + n * st;
    double* v1 = dg + n;
    double* v2 = v1 + n;
    double* wsh = v2 + n;
    double* tsh = wsh + kSpepChunk * n;
    double* res = tsh + kSpepChunk * n;          // [kSpepChunk][4]: L1, L2, y, c
    const size_t ssize = packed ? (size_t)d * (d + 1) + (size_t)d * d : (size_t)n * n;
    double* site2 = nat2 + (size_t)(own ? m : 0) * ssize;
    double* site1 = nat1 + (size_t)(own ? m : 0) * n;

    int maxcnt = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) maxcnt = max(maxcnt, __shfl_xor(maxcnt, off, 64));

    bool ok = true;
    double gcq = 0.0;                      // g_c - g_q
    if (maxcnt > 0) {                      // wavefront-uniform: some interval of this wavefront holds data
        const bool act = cnt > 0;
        // pair marginal: lower triangle of S and the pair mean
        {
            const bool lo_prior = (m == 0), hi_prior = (m == a.M);
            const double* S_lo = lo_prior ? a.prior_cov : Sig + (size_t)(m - 1) * d * d;
            const double* S_hi = hi_prior ? a.prior_cov : Sig + (size_t)m * d * d;
            const double* C = (lo_prior || hi_prior) ? nullptr : Sub + (size_t)(m - 1) * d * d;
            if (act && l < n) {
                for (int r = l; r < n; ++r) {          // column l, rows r >= l
                    double v;
                    if (r < d) v = S_lo[r * d + l];
                    else if (l >= d) v = S_hi[(r - d) * d + (l - d)];
                    else v = C ? C[(r - d) * d + l] : 0.0;
                    A[r * st + l] = v;
                }
                const bool hi = l >= d;
                const int kk = hi ? l - d : l;
                v1[l] = hi ? (hi_prior ? a.prior_mean[kk] : mu[(size_t)m * d + kk]) : (lo_prior ? a.prior_mean[kk] : mu[(size_t)(m - 1) * d + kk]);
            } else if (l < n) {
                for (int r = l; r < n; ++r) A[r * st + l] = (r == l) ? 1.0 : 0.0;
                v1[l] = 0.0;
            }
        }
        __syncthreads();
        const double ldS = spep_cholesky<NP>(A, n, st, l, ok);        // 1/2 log det S
        spep_tri_inverse(A, n, st, l);
        // u = Li mu
        double u = 0.0;
        if (l < n)
            for (int k = 0; k <= l; ++k) u = __builtin_fma(A[l * st + k], v1[k], u);
        double uu = u * u;
#pragma unroll
        for (int off = NP / 2; off > 0; off >>= 1) uu += __shfl_xor(uu, off, NP);
        __syncthreads();
        if (l < n) v1[l] = u;
        __syncthreads();
        // h = Li^T u;  Lam = Li^T Li into the strict upper triangle and dg
        double h = 0.0;
        if (l < n) {
            for (int k = l; k < n; ++k) h = __builtin_fma(A[k * st + l], v1[k], h);
            for (int i = l; i < n; ++i) {              // Lam[i][l], i >= l
                double s = 0.0;
                for (int k = i; k < n; ++k) s = __builtin_fma(A[k * st + i], A[k * st + l], s);
                if (i == l) dg[l] = s;
                else A[l * st + i] = s;
            }
        }
        __syncthreads();
        // Lam_c = Lam + 2 beta nat2 (lower triangle), hc = h - beta nat1
        const double beta = act ? alpha / (double)cnt : 0.0;
        if (l < n) {
            for (int r = l; r < n; ++r) {
                const double nv = act ? site2[packed ? spep_qidx(r, l, d) : r * n + l] : 0.0;
                A[r * st + l] = __builtin_fma(2.0 * beta, nv, (r == l) ? dg[l] : A[l * st + r]);
            }
            v2[l] = act ? __builtin_fma(-beta, site1[l], h) : 0.0;
        }
        __syncthreads();
        const double ldC = spep_cholesky<NP>(A, n, st, l, ok);        // 1/2 log det Lam_c
        spep_tri_inverse(A, n, st, l);
        double uc = 0.0;
        if (l < n)
            for (int k = 0; k <= l; ++k) uc = __builtin_fma(A[l * st + k], v2[k], uc);
        double ucc = uc * uc;
#pragma unroll
        for (int off = NP / 2; off > 0; off >>= 1) ucc += __shfl_xor(ucc, off, NP);
        __syncthreads();
        if (l < n) v2[l] = uc;
        __syncthreads();
        gcq = (-ldC + 0.5 * ucc) - (ldS + 0.5 * uu);
        if (!act) ok = true;
    }

    const double keep = 1.0 - lr, a1 = 1.0 - alpha;
    double esum = 0.0;
    int nskip = 0;
    for (int c0 = 0; c0 == 0 || c0 < maxcnt; c0 += kSpepChunk) {
        const int np = min(max(cnt - c0, 0), kSpepChunk);
        for (int e = l; e < np * n; e += NP) wsh[e] = a.w[(size_t)(i0 + c0) * n + e];
        for (int p = l; p < np; p += NP) {
            res[4 * p + 2] = y[i0 + c0 + p];
            res[4 * p + 3] = a.c[i0 + c0 + p];
        }
        __syncthreads();
        if (l < n)
            for (int p = 0; p < np; ++p) {
                double t = 0.0;
                for (int k = 0; k <= l; ++k) t = __builtin_fma(A[l * st + k], wsh[p * n + k], t);
                tsh[p * n + l] = t;
            }
        __syncthreads();
        for (int p = l; p < np; p += NP) {
            double s = 0.0, mc = 0.0;
            for (int r = 0; r < n; ++r) {
                const double t = tsh[p * n + r];
                s = __builtin_fma(t, t, s);
                mc = __builtin_fma(t, v2[r], mc);
            }
            double lz, d1, d2;
            pep_tilted<KIND>(mc, s + res[4 * p + 3], res[4 * p + 2], param, alpha, lz, d1, d2);
            const double L2 = 0.5 / (s + 1.0 / d2);
            const double L1 = 2.0 * L2 * (d1 / d2 - mc);
            const bool fin = isfinite(L1) && isfinite(L2);
            res[4 * p] = fin ? L1 : 0.0;
            res[4 * p + 1] = fin ? L2 : 0.0;
            if (fin) esum += lz + gcq;
            else if (ok) ++nskip;
        }
        __syncthreads();
        if (lr != 0.0 && own && ok && l < n) {
            // the first chunk carries the damping of the old site, later chunks add their sums
            const double f_old = (c0 == 0) ? keep + lr * a1 : 1.0;
            double acc1 = 0.0;
            for (int p = 0; p < np; ++p) acc1 = __builtin_fma(res[4 * p], wsh[p * n + l], acc1);
            site1[l] = __builtin_fma(lr, acc1, f_old * site1[l]);
            for (int r = packed ? l : 0; r < n; ++r) {
                double acc = 0.0;
                for (int p = 0; p < np; ++p) acc = __builtin_fma(res[4 * p + 1] * wsh[p * n + r], wsh[p * n + l], acc);
                double* x = site2 + (packed ? spep_qidx(r, l, d) : r * n + l);
                *x = __builtin_fma(lr, acc, f_old * *x);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int off = NP / 2; off > 0; off >>= 1) {
        esum += __shfl_xor(esum, off, NP);
        nskip += __shfl_xor(nskip, off, NP);
    }
    if (own && l == 0) {
        if (!ok) {
            esum = NAN;
            nskip = cnt;
        }
        if (e_out) e_out[m] = esum;
        if (ok && lr != 0.0 && lnorm) lnorm[m] = __builtin_fma(lr, esum, (keep + lr * a1) * lnorm[m]);
        if (nskip > 0 && skipped) atomicAdd(skipped, nskip);
    }
}

}  // namespace mfgm
