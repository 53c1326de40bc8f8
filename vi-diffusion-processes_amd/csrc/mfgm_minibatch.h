// ---- mini-batch sparse CVI: the data pass of one unsorted batch (mfgm_sparse_batch_predict_lik / mfgm_sparse_batch_seg) ----------------
// DESIGN.md section 26.  A batch drawn from a larger data set is a new tensor of n time points in any order every step, so nothing
// about it can be kept: the interval of a point, its conditional row (w_i, c_i) of p(f(t_i) | s(z-), s(z+)), the marginal q(f(t_i)) and
// the likelihood terms are all made here, in one launch, from the time point alone.  One lane per time point:
//   interval   m = #{z_j < t}: binary search in the inducing points (global memory through the cache; every lane walks the same top of
//              the tree), the gaps t - z- and z+ - t with both ends padded at -/+ kBatchInf
//   row        per term, the forward half of cond_score_term (mfgm_sparse_score.h) on the same device functions:
//                Q_mp = Q2 + A2 Q1 A2^T,  x = Q_mp^-1 A2 Q1 h,  y = h - A2^T x,  w+ = x,  w- = A1^T y,  c = h^T Q1 y
//              with Q under the exact-Q rule, so a point ON an inducing point has Q2 = 0 exactly, and an exactly-zero Q_mp has x = 0
//   marginal   fmu = w . pmu_m + shift,  fvar = c + w^T PC_m w  straight from the marginal blocks mu, Sig, Sub (the prior pads both ends)
//   likelihood ve, g1, g2 of mfgm_lik.h / the Gaussian formula, times `scale`; g1 in the expectation parameters of the zero-mean part
// The row is the one array indexed by a term's run-time offset; it lives in a lane-private LDS column (16 x 64 doubles, 8 KiB: the
// lanes of a wavefront hit 64 consecutive doubles, no bank conflict) instead of registers, where that indexing would mean scratch, and
// leaves for memory through one coalesced store of the wavefront's 64 rows.  Instantiated on the largest term block like
// k_sparse_cond_score.  The lanes' ve are summed by a fixed shuffle tree, the wavefronts by k_score_sum in index order: no atomics.
//
// k_batch_seg: CSR offsets of the SORTED batch per interval, one lane per inducing point and one binary search each: no histogram, no
// integer atomics, no scan.
#pragma once
#include "mfgm_lik.h"
#include "mfgm_sparse_score.h"

namespace mfgm {

constexpr double kBatchInf = 1e10;      // conditionals.interval_gaps' APPROX_INF

struct BatchArgs {
    int M, d;
    long long n;
    const double* z;            // [M] inducing points, increasing
    const double* t;            // [n] any order
    const double* shift;        // [n] or null
    const double* y;            // [n] (kind != 0)
    const double* prior_mean;   // [d]
    const double* prior_cov;    // [d, d]
    const double* mu;           // [M, d]
    const double* Sig;          // [M, d, d]
    const double* Sub;          // [M, d, d]  Sigma_{t+1,t} at t
    int* idx;                   // [n]        every output may be null
    double* w;                  // [n, 2d]
    double* c;                  // [n]
    double* fmu;
    double* fvar;
    double* ve;
    double* g1;
    double* g2;
    double* part;               // [blocks] the wavefronts' ve sums, or null
    int* info;
    int kind;
    double param, scale, jitter;
};

// The row of one term of shape (D0, D1, D2) at the gaps d1 = t - z-, d2 = z+ - t: w- to rows O .., w+ to rows d + O .. of the lane's LDS
// column `col` (stride 64), c accumulated.
template <int NMAX, int D0, int D1, int D2>
MFGM_DEV void cond_row_term(const TermDesc& td0, double jit, int d, double d1, double d2, double* col, double& c, int& bad) {
    constexpr int N = D0 * D1 * D2, NT = MFGM_NTRI(N);
    if constexpr (N <= NMAX) {
        TermDesc td = td0;
        const int O = td.offset;
        const int mode = td.nx == 0 ? 0 : (td.nx == 1 ? 1 : 2);
        const FactorBlk<D0> g0 = factor_slot<D0>(td, 0, d2, false, td.nx);      // transition 2: t -> z+
        const FactorBlk<D1> g1 = factor_slot<D1>(td, 1, d2, false, td.nx);
        const FactorBlk<D2> g2 = factor_slot<D2>(td, 2, d2, false, td.nx);
        const FactorBlk<D0> f0 = factor_slot<D0>(td, 0, d1, false, td.nx);      // transition 1: z- -> t
        const FactorBlk<D1> f1 = factor_slot<D1>(td, 1, d1, false, td.nx);
        const FactorBlk<D2> f2 = factor_slot<D2>(td, 2, d1, false, td.nx);
        double Qmp[NT], invd[N];
        // Q_mp = Q2 + A2 Q1 A2^T, column by column
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double v[N], t[N];
#pragma unroll
            for (int i = 0; i < N; ++i) { v[i] = (i == k) ? 1.0 : 0.0; t[i] = v[i]; }
            kron_vec<D0, D1, D2, true>(g0.a, g1.a, g2.a, v);
            q_times<D0, D1, D2>(f0, f1, f2, mode, jit, v);
            kron_vec<D0, D1, D2, false>(g0.a, g1.a, g2.a, v);
            q_times<D0, D1, D2>(g0, g1, g2, mode, jit, t);
#pragma unroll
            for (int i = k; i < N; ++i) Qmp[tix(i, k)] = v[i] + t[i];
        }
        bool zero = true;
#pragma unroll
        for (int e = 0; e < NT; ++e) zero = zero && (Qmp[e] == 0.0);
        if (zero) {
#pragma unroll
            for (int i = 0; i < N; ++i) Qmp[tix(i, i)] = 1.0;
        }
        int bd = 0;
        chol_inplace<N>(Qmp, invd, bd);
        bad |= bd;
        const double keep = zero ? 0.0 : 1.0;
        double u[N], x[N], y[N];
#pragma unroll
        for (int i = 0; i < N; ++i) u[i] = (i == 0) ? 1.0 : 0.0;               // h = e_0
        q_times<D0, D1, D2>(f0, f1, f2, mode, jit, u);                          // u = Q1 h
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = u[i];
        kron_vec<D0, D1, D2, false>(g0.a, g1.a, g2.a, x);
        trsv_lower<N>(Qmp, invd, x);
        trsv_lower_t<N>(Qmp, invd, x);
#pragma unroll
        for (int i = 0; i < N; ++i) { x[i] *= keep; y[i] = x[i]; }             // x = Q_mp^-1 A2 Q1 h
        kron_vec<D0, D1, D2, true>(g0.a, g1.a, g2.a, y);                        // A2^T x
#pragma unroll
        for (int i = 0; i < N; ++i) y[i] = ((i == 0) ? 1.0 : 0.0) - y[i];      // y = h - A2^T x
        double ct = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) ct = __builtin_fma(u[i], y[i], ct);         // c = h^T Q1 y (Q1 symmetric)
        c += ct;
        kron_vec<D0, D1, D2, true>(f0.a, f1.a, f2.a, y);                        // w- = A1^T y
#pragma unroll
        for (int i = 0; i < N; ++i) {
            col[(O + i) * 64] = y[i];
            col[(d + O + i) * 64] = x[i];
        }
    }
}

// mu += w . m, v += w^T S w for one half of the pair, w in the LDS column `col` (stride 64), S [d, d] full symmetric
MFGM_DEV void batch_half(const double* col, int d, const double* __restrict__ m, const double* __restrict__ S, double& mu, double& v) {
    for (int r = 0; r < d; ++r) {
        const double wr = col[r * 64];
        double t = 0.0;
        for (int j = 0; j < d; ++j) t = __builtin_fma(S[r * d + j], col[j * 64], t);
        mu = __builtin_fma(wr, m[r], mu);
        v = __builtin_fma(wr, t, v);
    }
}

template <int NMAX>
static __global__ __launch_bounds__(64) void k_sparse_batch(BatchArgs A, KernelTermsDev kt) {
    __shared__ double sh_w[16 * 64];
    const int lane = threadIdx.x, d = A.d, d2 = 2 * d, M = A.M;
    const long long gi = (long long)blockIdx.x * 64 + lane;
    const bool active = gi < A.n;
    const long long i = active ? gi : A.n - 1;      // idle lanes of the last wavefront repeat its last point and write nothing
    const double t = A.t[i];
    const bool fin = (t - t) == 0.0;
    // m = #{z_j < t} (a NaN compares false everywhere); never outside 0 .. M
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A.z[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    const int m = fin ? lo : 0;
    double* col = sh_w + lane;
    for (int r = 0; r < d2; ++r) col[r * 64] = 0.0;
    double c = 0.0;
    int bad = 0;
    if (fin) {
        const double d1 = t - (m == 0 ? -kBatchInf : A.z[m - 1]);
        const double d2g = (m == M ? kBatchInf : A.z[m]) - t;
        for (int q = 0; q < kt.nterm; ++q) {
            TermDesc td;
            td.offset = kt.offset[q];
            td.nx = 0;
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                td.kind[f] = kt.kind[q][f];
                td.rate[f] = kt.rate[q][f];
                td.var[f] = kt.var[q][f];
                td.nx += factor_exact(td.kind[f]) ? 0 : 1;
            }
            switch (kt.shape[q]) {
                case KT_SHAPE_1: cond_row_term<NMAX, 1, 1, 1>(td, A.jitter, d, d1, d2g, col, c, bad); break;
                case KT_SHAPE_2: cond_row_term<NMAX, 2, 1, 1>(td, A.jitter, d, d1, d2g, col, c, bad); break;
                case KT_SHAPE_3: cond_row_term<NMAX, 3, 1, 1>(td, A.jitter, d, d1, d2g, col, c, bad); break;
                case KT_SHAPE_22: cond_row_term<NMAX, 2, 2, 1>(td, A.jitter, d, d1, d2g, col, c, bad); break;
                case KT_SHAPE_23: cond_row_term<NMAX, 2, 3, 1>(td, A.jitter, d, d1, d2g, col, c, bad); break;
                case KT_SHAPE_32: cond_row_term<NMAX, 3, 2, 1>(td, A.jitter, d, d1, d2g, col, c, bad); break;
                default: cond_row_term<NMAX, 2, 2, 2>(td, A.jitter, d, d1, d2g, col, c, bad); break;
            }
        }
    }
    // the marginal: the pair of interval m from the marginal blocks, the prior at both ends with a zero cross block there
    const bool lo_prior = (m == 0), hi_prior = (m == M);
    double g = 0.0, v = c;      // g: the mean of the zero-mean part
    batch_half(col, d, lo_prior ? A.prior_mean : A.mu + (size_t)(m - 1) * d, lo_prior ? A.prior_cov : A.Sig + (size_t)(m - 1) * d * d, g, v);
    batch_half(col + d * 64, d, hi_prior ? A.prior_mean : A.mu + (size_t)m * d, hi_prior ? A.prior_cov : A.Sig + (size_t)m * d * d, g, v);
    if (!lo_prior && !hi_prior) {
        const double* C = A.Sub + (size_t)(m - 1) * d * d;      // Cov(x_m, x_{m-1})
        for (int r = 0; r < d; ++r) {
            double s = 0.0;
            for (int j = 0; j < d; ++j) s = __builtin_fma(C[r * d + j], col[j * 64], s);
            v = __builtin_fma(2.0 * col[(d + r) * 64], s, v);
        }
    }
    const double sh = A.shift ? A.shift[i] : 0.0;
    const double fm = g + sh;
    double e = 0.0, q1 = 0.0, q2 = 0.0;
    if (A.kind != 0) {
        const double yi = A.y[i];
        if (fin && yi == yi) {      // a NaN observation is an absent point
            double dmu, dv;
            if (A.kind == 1) {            // the kinds of mfgm_lik.h; 3 is MFGM_LIK_GAUSSIAN
                lik_bernoulli(fm, v, yi, A.param, e, dmu, dv);
            } else if (A.kind == 2) {
                lik_poisson(fm, v, yi, A.param, e, dmu, dv);
            } else {
                const double r = yi - fm, is2 = 1.0 / A.param;
                e = -0.5 * log(2.0 * M_PI * A.param) - 0.5 * (r * r + v) * is2;
                dmu = r * is2;
                dv = -0.5 * is2;
            }
            e *= A.scale;
            q1 = A.scale * (dmu - 2.0 * dv * g);
            q2 = A.scale * dv;
        }
    }
    if (active) {
        if (A.idx) A.idx[i] = m;
        if (A.c) A.c[i] = c;
        if (A.fmu) A.fmu[i] = fm;
        if (A.fvar) A.fvar[i] = v;
        if (A.ve) A.ve[i] = e;
        if (A.g1) A.g1[i] = q1;
        if (A.g2) A.g2[i] = q2;
    }
    if (A.part) {
        double s = active ? e : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) A.part[blockIdx.x] = s;
    }
    if (A.w) {
        // the wavefront's rows are one contiguous run of 64 * 2d doubles
        __syncthreads();
        const long long row0 = (long long)blockIdx.x * 64;
        for (int k = lane; k < 64 * d2; k += 64) {
            const int r = k / d2, cc = k - r * d2;
            if (row0 + r < A.n) A.w[(size_t)row0 * d2 + k] = sh_w[cc * 64 + r];
        }
    }
    // as in k_kernel_ssm: every writer of this word in the launch writes 1
    if (bad && *A.info == 0) *A.info = 1;
}

// seg[0] = 0, seg[m + 1] = #{t_i <= z_m}, seg[M + 1] = n for t sorted (NaN last, as torch.sort leaves them)
static __global__ __launch_bounds__(64) void k_batch_seg(int M, const double* __restrict__ z, int n, const double* __restrict__ t,
                                                        int* __restrict__ seg) {
    const int k = blockIdx.x * 64 + threadIdx.x;      // entry 0 .. M + 1
    if (k > M + 1) return;
    int lo = 0;
    if (k == M + 1) {
        lo = n;
    } else if (k > 0) {
        const double zm = z[k - 1];
        int hi = n;
        while (lo < hi) {
            const int mid = (int)(((long long)lo + hi) >> 1);
            if (t[mid] <= zm) lo = mid + 1;
            else hi = mid;
        }
    }
    seg[k] = lo;
}

}  // namespace mfgm
