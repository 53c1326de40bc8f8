// ---- kernel score of the sparse-CVI bound through the conditionals p(f(t_i) | s(z-), s(z+)) (mfgm_sparse_cond_score) -----------------
// DESIGN.md section 21.  At fixed q the bound depends on the kernel through the projections w_i and the conditional variances c_i of
// the data points: fmu_i = w_i . mu_pair, fvar_i = c_i + w_i^T Sigma_pair w_i.  A, Q and Pinf are block diagonal over the kernel's
// terms, so w and c are too; one term with emission slice h = e_0 and the gaps D1 = t - z-, D2 = z+ - t has, in covariance form
// (Q1^-1 does not exist when a data point sits on an inducing point),
//   Q_mp = Q2 + A2 Q1 A2^T,   x = Q_mp^-1 A2 Q1 h,   y = h - A2^T x,   w+ = x,   w- = A1^T y,   c = h^T Q1 y.
// Reverse mode from  wb = a mu_pair + 2 b Sigma_pair w  and  cb = b  (a = d ve / d fmu, b = d ve / d fvar):
//   u = Q1 h,  p = A2^T x,  yb = b u + A1 wb-,  z = Q_mp^-1 (wb+ - A2 yb),  q = A2^T z,  ub = b y + q,
// and every cotangent is a sum of outer products of these n-vectors, so with the pull-back  dQ = dP - dA P A^T - A dP A^T - A P dA^T
// the whole derivative is a set of vector-matrix-vector forms (the (q, p) forms of Q1 and Q2 on dP cancel):
//   on dA1:  y^T dA1 wb-  - ub^T dA1 (P A1^T h) - h^T dA1 (P A1^T ub) + q^T dA1 (P A1^T p) + p^T dA1 (P A1^T q)
//   on dA2:  z^T dA2 (Q1 y + P p)  +  x^T dA2 (P q - yb - Q1 q)
//   on dP :  ub^T dP h - (A1^T ub)^T dP (A1^T h) + (A1^T q)^T dP (A1^T p) - z^T dP x   (+ b w^T dP w of the prior padding at the two ends).
// dA and dP of a term are Kronecker products with one factor replaced by its closed-form derivative (factor_der), so a form costs one
// kron_vec and a dot product: no n x n array exists except the packed Q_mp, which is built column by column from kron_vecs.  Q acts as
// k_kernel_ssm builds it (factor_slot's m blocks under the exact-Q rule), so a zero gap gives an exactly-zero Q; an exactly-zero Q_mp
// block (a term without process noise and no jitter) has x = z = 0.
//
// One lane per data point, a uniform loop over the terms; instantiated on the largest term block like k_kernel_score.  The lanes of a
// wavefront are summed by a fixed shuffle tree, the wavefronts by k_score_sum in a fixed order: no floating-point atomics.
#pragma once
#include "mfgm_score.h"
#include "mfgm_sparse.h"

namespace mfgm {

struct CondScoreArgs {
    SparseArgs sp;
    const double* gap_lo;   // [N] t_i - z-  (the caller pads the ends)
    const double* gap_hi;   // [N] z+ - t_i
    const double* a;        // [N] d ve_i / d fmu_i
    const double* b;        // [N] d ve_i / d fvar_i
    const double* mu;       // [M, d]
    const double* Sig;      // [M, d, d]
    const double* Sub;      // [M, d, d]  Sigma_{t+1,t} at t
    double* part;           // [kScorePlanes][nblk]
    int* info;
    double jitter;
    int nblk;
};

// v := Q v for the Q of one transition: factor_slot's blocks under the exact-Q rule (mode as expand_at's) plus the jitter
template <int D0, int D1, int D2>
MFGM_DEV void q_times(const FactorBlk<D0>& f0, const FactorBlk<D1>& f1, const FactorBlk<D2>& f2, int mode, double jitter,
                      double (&v)[D0 * D1 * D2]) {
    constexpr int N = D0 * D1 * D2;
    double t[N];
#pragma unroll
    for (int i = 0; i < N; ++i) t[i] = v[i];
    if (mode == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = 0.0;
    } else {
        kron_vec<D0, D1, D2, false>(f0.m, f1.m, f2.m, v);
        if (mode == 2) {
            double s[N];
#pragma unroll
            for (int i = 0; i < N; ++i) s[i] = t[i];
            kron_vec<D0, D1, D2, false>(f0.p, f1.p, f2.p, s);
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = s[i] - v[i];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = __builtin_fma(jitter, t[i], v[i]);
}

// l^T K r for K = u0 (x) u1 (x) u2 with factor F's block replaced by dF
template <int D0, int D1, int D2, int F, int DF>
MFGM_DEV double kron_form(const double (&u0)[D0 * D0], const double (&u1)[D1 * D1], const double (&u2)[D2 * D2], const double (&dF)[DF * DF],
                          const double (&l)[D0 * D1 * D2], const double (&r)[D0 * D1 * D2]) {
    constexpr int N = D0 * D1 * D2;
    double v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = r[i];
    if constexpr (F == 0) kron_vec<D0, D1, D2, false>(dF, u1, u2, v);
    else if constexpr (F == 1) kron_vec<D0, D1, D2, false>(u0, dF, u2, v);
    else kron_vec<D0, D1, D2, false>(u0, u1, dF, v);
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) t = __builtin_fma(l[i], v[i], t);
    return t;
}

// acc[2 F] += s l^T (d A / d rate_F) r for the transition of length dt
template <int D0, int D1, int D2, int F, int DF>
MFGM_DEV void form_a_slot(const TermDesc& td, double dt, const FactorBlk<D0>& f0, const FactorBlk<D1>& f1, const FactorBlk<D2>& f2,
                          const double (&l)[D0 * D1 * D2], const double (&r)[D0 * D1 * D2], double s, double (&acc)[6]) {
    if (td.kind[F] == 0) return;
    // the gap is made opaque per form: the derivative blocks of every slot and both transitions would otherwise be computed once and
    // held in registers through the whole term
    double dto = dt;
    asm volatile("" : "+v"(dto));
    const FactorDer<DF> g = factor_der<DF>(td.kind[F], td.rate[F], td.var[F], dto);
    acc[2 * F] = __builtin_fma(s, kron_form<D0, D1, D2, F, DF>(f0.a, f1.a, f2.a, g.da, l, r), acc[2 * F]);
}

template <int D0, int D1, int D2>
MFGM_DEV void form_a(const TermDesc& td, double dt, const FactorBlk<D0>& f0, const FactorBlk<D1>& f1, const FactorBlk<D2>& f2,
                     const double (&l)[D0 * D1 * D2], const double (&r)[D0 * D1 * D2], double s, double (&acc)[6]) {
    form_a_slot<D0, D1, D2, 0, D0>(td, dt, f0, f1, f2, l, r, s, acc);
    form_a_slot<D0, D1, D2, 1, D1>(td, dt, f0, f1, f2, l, r, s, acc);
    form_a_slot<D0, D1, D2, 2, D2>(td, dt, f0, f1, f2, l, r, s, acc);
}

// acc[2 F | 2 F + 1] += s l^T (d Pinf / d rate_F | d var_F) r
template <int D0, int D1, int D2, int F, int DF>
MFGM_DEV void form_p_slot(const TermDesc& td, const FactorBlk<D0>& f0, const FactorBlk<D1>& f1, const FactorBlk<D2>& f2,
                          const double (&l)[D0 * D1 * D2], const double (&r)[D0 * D1 * D2], double s, double (&acc)[6]) {
    if (td.kind[F] == 0) return;
    double zo = 0.0;      // opaque for the same reason
    asm volatile("" : "+v"(zo));
    const FactorDer<DF> g = factor_der<DF>(td.kind[F], td.rate[F], td.var[F], zo);
    acc[2 * F] = __builtin_fma(s, kron_form<D0, D1, D2, F, DF>(f0.p, f1.p, f2.p, g.dpl, l, r), acc[2 * F]);
    acc[2 * F + 1] = __builtin_fma(s, kron_form<D0, D1, D2, F, DF>(f0.p, f1.p, f2.p, g.dpv, l, r), acc[2 * F + 1]);
}

template <int D0, int D1, int D2>
MFGM_DEV void form_p(const TermDesc& td, const FactorBlk<D0>& f0, const FactorBlk<D1>& f1, const FactorBlk<D2>& f2,
                     const double (&l)[D0 * D1 * D2], const double (&r)[D0 * D1 * D2], double s, double (&acc)[6]) {
    form_p_slot<D0, D1, D2, 0, D0>(td, f0, f1, f2, l, r, s, acc);
    form_p_slot<D0, D1, D2, 1, D1>(td, f0, f1, f2, l, r, s, acc);
    form_p_slot<D0, D1, D2, 2, D2>(td, f0, f1, f2, l, r, s, acc);
}

// wb[i] = a mu_pair[o + i] + 2 b (Sigma_pair w)[o + i] for the rows o .. o + N - 1 of one half (hi: the state on the right) of the
// pair of interval m, straight from the marginal blocks (the prior pads both ends); w [2d] of the data point
template <int N>
MFGM_DEV void pair_cotangent(const CondScoreArgs& A, int m, bool hi, int O, const double* __restrict__ w, double av, double bv,
                             double (&wb)[N]) {
    const int d = A.sp.d, M = A.sp.M;
    const bool lo_prior = (m == 0), hi_prior = (m == M);
    const bool prior = hi ? hi_prior : lo_prior;
    const int node = hi ? m : m - 1;
    const double* S = prior ? A.sp.prior_cov : A.Sig + (size_t)node * d * d;
    const double* mean = prior ? A.sp.prior_mean : A.mu + (size_t)node * d;
    const double* C = (lo_prior || hi_prior) ? nullptr : A.Sub + (size_t)(m - 1) * d * d;      // Cov(x_hi, x_lo)
    const double* wsame = w + (hi ? d : 0);
    const double* wother = w + (hi ? 0 : d);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int r = O + i;
        double t = 0.0;
        for (int j = 0; j < d; ++j) t = __builtin_fma(S[r * d + j], wsame[j], t);
        if (C) {
            for (int j = 0; j < d; ++j) t = __builtin_fma(hi ? C[r * d + j] : C[j * d + r], wother[j], t);
        }
        wb[i] = __builtin_fma(av, mean[r], 2.0 * bv * t);
    }
}

// One term of shape (D0, D1, D2) for the lane's data point.  ARGS: CondScoreArgs, or another struct with sp.M, sp.d, jitter and a
// pair_cotangent of its own (the panel's reads the packed moments of a B-chain plan, mfgm_panel_score.h).
template <int NMAX, int D0, int D1, int D2, class ARGS>
MFGM_DEV void cond_score_term(const ARGS& A, const TermDesc& td0, int m, const double* __restrict__ w, double d1, double d2,
                              double av, double bv, double (&acc)[6], int& bad) {
    constexpr int N = D0 * D1 * D2, NT = MFGM_NTRI(N);
    if constexpr (N <= NMAX) {
        TermDesc td = td0;
        const int O = td.offset;
        const int mode = td.nx == 0 ? 0 : (td.nx == 1 ? 1 : 2);
        const double jit = A.jitter;
        const FactorBlk<D0> g0 = factor_slot<D0>(td, 0, d2, false, td.nx);      // transition 2: t -> z+
        const FactorBlk<D1> g1 = factor_slot<D1>(td, 1, d2, false, td.nx);
        const FactorBlk<D2> g2 = factor_slot<D2>(td, 2, d2, false, td.nx);
        double Qmp[NT], invd[N];
        {
            const FactorBlk<D0> f0 = factor_slot<D0>(td, 0, d1, false, td.nx);  // transition 1: z- -> t
            const FactorBlk<D1> f1 = factor_slot<D1>(td, 1, d1, false, td.nx);
            const FactorBlk<D2> f2 = factor_slot<D2>(td, 2, d1, false, td.nx);
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
        __builtin_amdgcn_sched_barrier(0);
        // transition 1 again, from an opaque copy of the gap: its blocks would otherwise stay in registers through the factorisation
        double d1o = d1;
        asm volatile("" : "+v"(d1o));
        const FactorBlk<D0> f0 = factor_slot<D0>(td, 0, d1o, false, td.nx);
        const FactorBlk<D1> f1 = factor_slot<D1>(td, 1, d1o, false, td.nx);
        const FactorBlk<D2> f2 = factor_slot<D2>(td, 2, d1o, false, td.nx);
        double h[N], u[N], x[N], p[N], y[N];
#pragma unroll
        for (int i = 0; i < N; ++i) { h[i] = (i == 0) ? 1.0 : 0.0; u[i] = h[i]; }
        q_times<D0, D1, D2>(f0, f1, f2, mode, jit, u);                      // u = Q1 h
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = u[i];
        kron_vec<D0, D1, D2, false>(g0.a, g1.a, g2.a, x);
        trsv_lower<N>(Qmp, invd, x);
        trsv_lower_t<N>(Qmp, invd, x);
#pragma unroll
        for (int i = 0; i < N; ++i) { x[i] *= keep; p[i] = x[i]; }         // x = Q_mp^-1 A2 Q1 h
        kron_vec<D0, D1, D2, true>(g0.a, g1.a, g2.a, p);                    // p = A2^T x
#pragma unroll
        for (int i = 0; i < N; ++i) y[i] = h[i] - p[i];
        double wbm[N], yb[N], z[N], q[N], ub[N];
        pair_cotangent<N>(A, m, false, O, w, av, bv, wbm);
#pragma unroll
        for (int i = 0; i < N; ++i) yb[i] = wbm[i];
        kron_vec<D0, D1, D2, false>(f0.a, f1.a, f2.a, yb);
#pragma unroll
        for (int i = 0; i < N; ++i) yb[i] = __builtin_fma(bv, u[i], yb[i]);  // yb = b u + A1 wb-
        {
            double t[N];
#pragma unroll
            for (int i = 0; i < N; ++i) t[i] = yb[i];
            kron_vec<D0, D1, D2, false>(g0.a, g1.a, g2.a, t);
            pair_cotangent<N>(A, m, true, O, w, av, bv, z);
#pragma unroll
            for (int i = 0; i < N; ++i) z[i] -= t[i];
        }
        trsv_lower<N>(Qmp, invd, z);
        trsv_lower_t<N>(Qmp, invd, z);
#pragma unroll
        for (int i = 0; i < N; ++i) { z[i] *= keep; q[i] = z[i]; }         // z = Q_mp^-1 (wb+ - A2 yb)
        kron_vec<D0, D1, D2, true>(g0.a, g1.a, g2.a, q);                    // q = A2^T z
#pragma unroll
        for (int i = 0; i < N; ++i) ub[i] = __builtin_fma(bv, y[i], q[i]);
        __builtin_amdgcn_sched_barrier(0);
        // ---- forms on dA2 and the (z, x) form on dP
        {
            double r[N], t[N];
#pragma unroll
            for (int i = 0; i < N; ++i) { r[i] = y[i]; t[i] = p[i]; }
            q_times<D0, D1, D2>(f0, f1, f2, mode, jit, r);
            kron_vec<D0, D1, D2, false>(f0.p, f1.p, f2.p, t);
#pragma unroll
            for (int i = 0; i < N; ++i) r[i] += t[i];
            form_a<D0, D1, D2>(td, d2, g0, g1, g2, z, r, 1.0, acc);         // z^T dA2 (Q1 y + P p)
#pragma unroll
            for (int i = 0; i < N; ++i) { r[i] = q[i]; t[i] = q[i]; }
            q_times<D0, D1, D2>(f0, f1, f2, mode, jit, r);
            kron_vec<D0, D1, D2, false>(f0.p, f1.p, f2.p, t);
#pragma unroll
            for (int i = 0; i < N; ++i) r[i] = t[i] - yb[i] - r[i];
            form_a<D0, D1, D2>(td, d2, g0, g1, g2, x, r, 1.0, acc);         // x^T dA2 (P q - yb - Q1 q)
            form_p<D0, D1, D2>(td, f0, f1, f2, z, x, -1.0, acc);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- forms on dA1 and the rest of dP
        form_a<D0, D1, D2>(td, d1o, f0, f1, f2, y, wbm, 1.0, acc);
        form_p<D0, D1, D2>(td, f0, f1, f2, ub, h, 1.0, acc);
        {
            double ah[N], au[N], aq[N], ap[N], t[N];
#pragma unroll
            for (int i = 0; i < N; ++i) { ah[i] = h[i]; au[i] = ub[i]; aq[i] = q[i]; ap[i] = p[i]; }
            kron_vec<D0, D1, D2, true>(f0.a, f1.a, f2.a, ah);
            kron_vec<D0, D1, D2, true>(f0.a, f1.a, f2.a, au);
            kron_vec<D0, D1, D2, true>(f0.a, f1.a, f2.a, aq);
            kron_vec<D0, D1, D2, true>(f0.a, f1.a, f2.a, ap);
            form_p<D0, D1, D2>(td, f0, f1, f2, au, ah, -1.0, acc);
            form_p<D0, D1, D2>(td, f0, f1, f2, aq, ap, 1.0, acc);
#pragma unroll
            for (int i = 0; i < N; ++i) t[i] = ah[i];
            kron_vec<D0, D1, D2, false>(f0.p, f1.p, f2.p, t);
            form_a<D0, D1, D2>(td, d1o, f0, f1, f2, ub, t, -1.0, acc);
#pragma unroll
            for (int i = 0; i < N; ++i) t[i] = au[i];
            kron_vec<D0, D1, D2, false>(f0.p, f1.p, f2.p, t);
            form_a<D0, D1, D2>(td, d1o, f0, f1, f2, h, t, -1.0, acc);
#pragma unroll
            for (int i = 0; i < N; ++i) t[i] = ap[i];
            kron_vec<D0, D1, D2, false>(f0.p, f1.p, f2.p, t);
            form_a<D0, D1, D2>(td, d1o, f0, f1, f2, q, t, 1.0, acc);
#pragma unroll
            for (int i = 0; i < N; ++i) t[i] = aq[i];
            kron_vec<D0, D1, D2, false>(f0.p, f1.p, f2.p, t);
            form_a<D0, D1, D2>(td, d1o, f0, f1, f2, p, t, 1.0, acc);
        }
        // ---- the prior padding of the two end intervals: fvar holds w^T (Pinf + jitter I) w there
        if (m == 0 || m == A.sp.M) {
            double wp[N];
            const double* wh = w + (m == 0 ? 0 : A.sp.d) + O;
#pragma unroll
            for (int i = 0; i < N; ++i) wp[i] = wh[i];
            form_p<D0, D1, D2>(td, f0, f1, f2, wp, wp, bv, acc);
        }
    }
}

// The lane's point through every term: the uniform loop over the terms, each term's six sums added over the wavefront by a fixed
// shuffle tree into part[plane][blockIdx.x] (an idle lane, active == false, adds nothing).  Returns the lane's bad-block flag.
template <int NMAX, class ARGS>
MFGM_DEV int cond_score_lane(const ARGS& A, const KernelTermsDev& kt, int m, const double* __restrict__ w, double d1, double d2, double av,
                             double bv, bool active, double* __restrict__ part, int nblk) {
    int bad = 0;
    for (int c = 0; c < kt.nterm; ++c) {
        TermDesc td;
        td.offset = kt.offset[c];
        td.nx = 0;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            td.kind[f] = kt.kind[c][f];
            td.rate[f] = kt.rate[c][f];
            td.var[f] = kt.var[c][f];
            td.nx += factor_exact(td.kind[f]) ? 0 : 1;
        }
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        switch (kt.shape[c]) {
            case KT_SHAPE_1: cond_score_term<NMAX, 1, 1, 1>(A, td, m, w, d1, d2, av, bv, acc, bad); break;
            case KT_SHAPE_2: cond_score_term<NMAX, 2, 1, 1>(A, td, m, w, d1, d2, av, bv, acc, bad); break;
            case KT_SHAPE_3: cond_score_term<NMAX, 3, 1, 1>(A, td, m, w, d1, d2, av, bv, acc, bad); break;
            case KT_SHAPE_22: cond_score_term<NMAX, 2, 2, 1>(A, td, m, w, d1, d2, av, bv, acc, bad); break;
            case KT_SHAPE_23: cond_score_term<NMAX, 2, 3, 1>(A, td, m, w, d1, d2, av, bv, acc, bad); break;
            case KT_SHAPE_32: cond_score_term<NMAX, 3, 2, 1>(A, td, m, w, d1, d2, av, bv, acc, bad); break;
            default: cond_score_term<NMAX, 2, 2, 2>(A, td, m, w, d1, d2, av, bv, acc, bad); break;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            double s = active ? acc[k] : 0.0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
            if (threadIdx.x == 0) part[(size_t)(c * 6 + k) * nblk + blockIdx.x] = s;
        }
    }
    return bad;
}

template <int NMAX>
static __global__ __launch_bounds__(64) void k_sparse_cond_score(CondScoreArgs A, KernelTermsDev kt) {
    const int gi = blockIdx.x * 64 + threadIdx.x;
    const int N = A.sp.N;
    const bool active = gi < N;
    const int i = active ? gi : N - 1;      // idle lanes of the last wavefront repeat its last point and add nothing
    // the interval of the point: the last m with seg[m] <= i
    int lo = 0, hi = A.sp.M;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (A.sp.seg[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const int m = lo;
    const double* w = A.sp.w + (size_t)i * (2 * A.sp.d);
    const int bad = cond_score_lane<NMAX>(A, kt, m, w, A.gap_lo[i], A.gap_hi[i], A.a[i], A.b[i], active, A.part, A.nblk);
    // as in k_kernel_ssm: every writer of this word in the launch writes 1
    if (bad && *A.info == 0) *A.info = 1;
}

}  // namespace mfgm
