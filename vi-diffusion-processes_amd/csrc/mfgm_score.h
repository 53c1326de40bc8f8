// ---- log-likelihood score of the kernel terms in one pass over the posterior pairwise moments (mfgm_packed_kernel_score) --------
// Fisher's identity: d/dh log Z(h) = E_post[d/dh log p_h(x)].  The prior log density of a Gauss-Markov chain is a sum over the
// transitions of terms quadratic in (x_k, x_k+1), so the expectation needs only the posterior pairwise moments (mu, Sigma_tt,
// Sigma_{t+1,t}) of the selected inverse.  With moments centred on the prior state mean,
//   S = Sigma_k + mu_k mu_k^T,  S' = Sigma_k+1 + mu_k+1 mu_k+1^T,  C = Sigma_{k+1,k} + mu_k+1 mu_k^T,
//   W = C - A S,  M = S' - A C^T - W A^T  (= E[(x' - A x)(x' - A x)^T]),
//   G_Q = 1/2 (Q^-1 M Q^-1 - Q^-1),  G_A = Q^-1 W,  G_P0 = 1/2 (P0^-1 S_0 P0^-1 - P0^-1),
// and Q = P - A P A^T + jitter I, the cotangents are pulled back once per transition to the factors' variables,
//   Gp = G_Q - A^T G_Q A  (on dP),   Ga = G_A - 2 G_Q A P  (on dA),
// after which the product rule across the Kronecker factors is a reduction of Ga / Gp to each factor's own block (kron_marginal)
// met by that factor's closed-form (da, dp / d rate, dp / d var) (factor_der).
//
// A, Q and their inverses are block diagonal over the terms, so a term needs only its own diagonal blocks of the moments.  The
// kernel therefore walks a lane's segment once per term (a uniform loop) and loads just that term's block -- in total fewer bytes
// than one pass over the whole arrays.  Same lane-per-segment mapping as k_kernel_ssm; the transition into a segment's first node
// takes the previous node from the neighbouring lane.  P and Q are rebuilt from factor_blocks / expand_at of mfgm_kernel_ssm.h, so Q
// is that kernel's Q and a zero gap gives an exactly-zero block.  The Kronecker products A = (x) a_f and Pinf = (x) p_f are never
// formed: they act factor by factor (kron_apply / kron_vec), with T = A S and Z = (W + T / 2) A^T giving M = S' - Z - Z^T.
//
// The kernel is instantiated on the LARGEST TERM BLOCK of the tree (1, 2, 3, 4, 6, 8), not on the plan's d, which only enters the
// strides: a Sum of 3 x 3 blocks at d = 8 runs the 3 x 3 code.  Branches on the term structure are wave-uniform, the term's offset
// only enters scalar address arithmetic, nothing in registers is indexed by a runtime value; no atomics, no scratch in any
// instantiation (tools/isa_regs.py on this unit's listing: rerun it when the toolchain changes, the 6 x 6 and 8 x 8 blocks sit close
// to the register file's size).  The 6 x 6 and 8 x 8 product blocks keep W / G_A / Ga in a lane-private LDS column (no barrier) and
// form M column by column (column k of T from column k of S, straight into M), and the 8 x 8 block keeps the packed M / G_Q / Gp
// there too, so that one n x n array at most is in registers beside the factor blocks.
// Per-lane partials go to the plan workspace [8 * 6][Lpad] and k_score_sum adds them per chain in a fixed order.
#pragma once
#include "mfgm_kernel_ssm.h"

namespace mfgm {

constexpr int kScorePlanes = 8 * 3 * 2;   // (term, slot, rate | var)

// d a / d rate, d p / d rate and d p / d var of factor_blocks (p is linear in var for every kind)
template <int DF>
struct FactorDer {
    double da[DF * DF], dpl[DF * DF], dpv[DF * DF];
};

template <int DF>
MFGM_DEV FactorDer<DF> factor_der(int kind, double l, double v, double dt) {
    FactorDer<DF> r;
#pragma unroll
    for (int e = 0; e < DF * DF; ++e) { r.da[e] = 0.0; r.dpl[e] = 0.0; r.dpv[e] = 0.0; }
    if constexpr (DF == 1) {
        if (kind == MFGM_FACTOR_MATERN12) {
            r.da[0] = -dt * exp(-l * dt);
            r.dpv[0] = 1.0;
        } else if (kind == MFGM_FACTOR_CONSTANT) {
            r.dpv[0] = 1.0;
        }
    } else if constexpr (DF == 2) {
        if (kind == MFGM_FACTOR_MATERN32) {
            const double ex = exp(-l * dt), u = l * dt;
            r.da[0] = ex * (-u * dt);
            r.da[1] = ex * (-dt * dt);
            r.da[2] = ex * (u * (u - 2.0));
            r.da[3] = ex * (dt * (u - 2.0));
            r.dpl[3] = 2.0 * v * l;
            r.dpv[0] = 1.0;
            r.dpv[3] = l * l;
        } else {   // MFGM_FACTOR_HARMONIC
            double s, c;
            sincos(l * dt, &s, &c);
            r.da[0] = -dt * s;
            r.da[1] = -dt * c;
            r.da[2] = dt * c;
            r.da[3] = -dt * s;
            r.dpv[0] = 1.0;
            r.dpv[3] = 1.0;
        }
    } else {       // MFGM_FACTOR_MATERN52: a = ex g(l), da = ex (g' - dt g), simplified
        const double ex = exp(-l * dt), u = l * dt, h = 0.5 * dt * dt, l2 = l * l;
        r.da[0] = ex * (-l2 * dt * h);
        r.da[1] = ex * (-2.0 * u * h);
        r.da[2] = ex * (-dt * h);
        r.da[3] = ex * (l2 * h * (u - 3.0));
        r.da[4] = ex * (2.0 * l * h * (u - 3.0));
        r.da[5] = ex * (h * (u - 3.0));
        r.da[6] = ex * (l2 * dt * (-3.0 + 3.0 * u - 0.5 * u * u));
        r.da[7] = ex * (u * (-6.0 + 6.0 * u - u * u));
        r.da[8] = ex * (dt * (-3.0 + 3.0 * u - 0.5 * u * u));
        const double t = 2.0 * v * l / 3.0;
        r.dpl[2] = -t;
        r.dpl[6] = -t;
        r.dpl[4] = t;
        r.dpl[8] = 4.0 * v * l2 * l;
        r.dpv[0] = 1.0;
        r.dpv[2] = -l2 / 3.0;
        r.dpv[6] = -l2 / 3.0;
        r.dpv[4] = l2 / 3.0;
        r.dpv[8] = l2 * l2;
    }
    return r;
}

// entry (i, j) of u0 (x) u1 (x) u2 at compile-time indices: the Kronecker products A and Pinf are never held as n x n arrays
template <int D0, int D1, int D2>
MFGM_DEV double kron_at(const double (&u0)[D0 * D0], const double (&u1)[D1 * D1], const double (&u2)[D2 * D2], int i, int j) {
    const int i0 = i / (D1 * D2), i1 = (i / D2) % D1, i2 = i % D2;
    const int j0 = j / (D1 * D2), j1 = (j / D2) % D1, j2 = j % D2;
    return u0[i0 * D0 + j0] * u1[i1 * D1 + j1] * u2[i2 * D2 + j2];
}

// one line of kron_apply: v := K v (or K^T v, TR) for K = u0 (x) u1 (x) u2, one factor at a time; at(i0, i1, i2) is the line's entry
template <int D0, int D1, int D2, bool TR, class At>
MFGM_DEV void kron_line(const double (&u0)[D0 * D0], const double (&u1)[D1 * D1], const double (&u2)[D2 * D2], At at) {
    if constexpr (D0 > 1) {
#pragma unroll
        for (int i1 = 0; i1 < D1; ++i1)
#pragma unroll
            for (int i2 = 0; i2 < D2; ++i2) {
                double v[D0];
#pragma unroll
                for (int i = 0; i < D0; ++i) {
                    double t = 0.0;
#pragma unroll
                    for (int j = 0; j < D0; ++j) t = __builtin_fma(TR ? u0[j * D0 + i] : u0[i * D0 + j], at(j, i1, i2), t);
                    v[i] = t;
                }
#pragma unroll
                for (int i = 0; i < D0; ++i) at(i, i1, i2) = v[i];
            }
    } else {
#pragma unroll
        for (int i1 = 0; i1 < D1; ++i1)
#pragma unroll
            for (int i2 = 0; i2 < D2; ++i2) at(0, i1, i2) *= u0[0];
    }
    if constexpr (D1 > 1) {
#pragma unroll
        for (int i0 = 0; i0 < D0; ++i0)
#pragma unroll
            for (int i2 = 0; i2 < D2; ++i2) {
                double v[D1];
#pragma unroll
                for (int i = 0; i < D1; ++i) {
                    double t = 0.0;
#pragma unroll
                    for (int j = 0; j < D1; ++j) t = __builtin_fma(TR ? u1[j * D1 + i] : u1[i * D1 + j], at(i0, j, i2), t);
                    v[i] = t;
                }
#pragma unroll
                for (int i = 0; i < D1; ++i) at(i0, i, i2) = v[i];
            }
    } else {
#pragma unroll
        for (int i0 = 0; i0 < D0; ++i0)
#pragma unroll
            for (int i2 = 0; i2 < D2; ++i2) at(i0, 0, i2) *= u1[0];
    }
    if constexpr (D2 > 1) {
#pragma unroll
        for (int i0 = 0; i0 < D0; ++i0)
#pragma unroll
            for (int i1 = 0; i1 < D1; ++i1) {
                double v[D2];
#pragma unroll
                for (int i = 0; i < D2; ++i) {
                    double t = 0.0;
#pragma unroll
                    for (int j = 0; j < D2; ++j) t = __builtin_fma(TR ? u2[j * D2 + i] : u2[i * D2 + j], at(i0, i1, j), t);
                    v[i] = t;
                }
#pragma unroll
                for (int i = 0; i < D2; ++i) at(i0, i1, i) = v[i];
            }
    } else {
#pragma unroll
        for (int i0 = 0; i0 < D0; ++i0)
#pragma unroll
            for (int i1 = 0; i1 < D1; ++i1) at(i0, i1, 0) *= u2[0];
    }
}

// v := K v (or K^T v) for a vector v [n]
template <int D0, int D1, int D2, bool TR>
MFGM_DEV void kron_vec(const double (&u0)[D0 * D0], const double (&u1)[D1 * D1], const double (&u2)[D2 * D2],
                       double (&v)[D0 * D1 * D2]) {
    kron_line<D0, D1, D2, TR>(u0, u1, u2, [&](int i0, int i1, int i2) -> double& { return v[(i0 * D1 + i1) * D2 + i2]; });
}

// X := K X (ROWS = false) or X := X K^T (ROWS = true) for K = u0 (x) u1 (x) u2, or with K^T in K's place (TR), in place and one
// Kronecker factor at a time: the n x n product K is never formed, and a line of X costs n (D0 + D1 + D2) multiplications, not n^2.
template <int D0, int D1, int D2, bool TR, bool ROWS>
MFGM_DEV void kron_apply(const double (&u0)[D0 * D0], const double (&u1)[D1 * D1], const double (&u2)[D2 * D2],
                         double (&X)[D0 * D1 * D2 * D0 * D1 * D2]) {
    constexpr int n = D0 * D1 * D2;
#pragma unroll
    for (int l = 0; l < n; ++l) {
        auto at = [&](int i0, int i1, int i2) -> double& {
            const int i = (i0 * D1 + i1) * D2 + i2;
            return ROWS ? X[l * n + i] : X[i * n + l];
        };
        kron_line<D0, D1, D2, TR>(u0, u1, u2, at);
        if constexpr (n >= 6) __builtin_amdgcn_sched_barrier(0);      // one line at a time: interleaved lines cost registers
    }
}

// r[e_F] = sum over the other two factors' indices of G[i][j] u_g[e_g] u_h[e_h]: the cotangent of factor F's block when the Kronecker
// product's other factors are u_g, u_h (u_F is not read).  G full n x n, or symmetric packed lower (SYM).
template <int D0, int D1, int D2, int F, bool SYM, int NG, int R2>
MFGM_DEV void kron_marginal(const double (&G)[NG], const double (&u0)[D0 * D0], const double (&u1)[D1 * D1], const double (&u2)[D2 * D2],
                            double (&r)[R2], const double* lds = nullptr) {
    constexpr int n = D0 * D1 * D2, DF = (F == 0 ? D0 : (F == 1 ? D1 : D2));
    static_assert(NG == (SYM ? MFGM_NTRI(n) : n * n) && R2 == DF * DF, "kron_marginal: sizes");
#pragma unroll
    for (int e = 0; e < DF * DF; ++e) r[e] = 0.0;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        const int i0 = i / (D1 * D2), i1 = (i / D2) % D1, i2 = i % D2;
#pragma unroll
        for (int j = 0; j < n; ++j) {
            const int j0 = j / (D1 * D2), j1 = (j / D2) % D1, j2 = j % D2;
            const int e0 = i0 * D0 + j0, e1 = i1 * D1 + j1, e2 = i2 * D2 + j2;
            const double g = SYM ? G[six(i, j)] : (lds ? lds[(i * n + j) * 64] : G[i * n + j]);
            if constexpr (F == 0) r[e0] = __builtin_fma(g, u1[e1] * u2[e2], r[e0]);
            else if constexpr (F == 1) r[e1] = __builtin_fma(g, u0[e0] * u2[e2], r[e1]);
            else r[e2] = __builtin_fma(g, u0[e0] * u1[e1], r[e2]);
        }
    }
}

template <int N2>
MFGM_DEV double dot_flat(const double (&x)[N2], const double (&y)[N2]) {
    double t = 0.0;
#pragma unroll
    for (int e = 0; e < N2; ++e) t = __builtin_fma(x[e], y[e], t);
    return t;
}

// M := L^{-T} M   (full N x N, column by column)
template <int N>
MFGM_DEV void trsm_left_lower_t(const double (&L)[MFGM_NTRI(N)], const double (&invd)[N], double (&M)[N * N]) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {
            double t = M[i * N + c];
#pragma unroll
            for (int k = i + 1; k < N; ++k) t = __builtin_fma(-L[tix(k, i)], M[k * N + c], t);
            M[i * N + c] = t * invd[i];
        }
    }
}

// M := 1/2 (K^-1 M K^-1 - K^-1) with K = L L^T, through the whitened L^-1 M L^-T - I
template <int N>
MFGM_DEV void score_cotangent(const double (&L)[MFGM_NTRI(N)], const double (&invd)[N], double (&M)[N * N]) {
    trsm_left_lower<N>(L, invd, M);
    trsm_right_lower_t<N>(L, invd, M);
#pragma unroll
    for (int i = 0; i < N; ++i) M[i * N + i] -= 1.0;
    trsm_left_lower_t<N>(L, invd, M);
    trsm_right_lower<N>(L, invd, M);
#pragma unroll
    for (int e = 0; e < N * N; ++e) M[e] *= 0.5;
}

// the term's block (offset O, a uniform value: scalar address arithmetic) of the centred second moment S = Sigma + mu mu^T of node
// (w, s), packed lower, and of mu
template <int N>
MFGM_DEV void ld_score_moment(const double* __restrict__ xg, const double* __restrict__ Sg, int D, int R, int s, LaneRef w, int O,
                              double (&mu)[N], double (&S)[MFGM_NTRI(N)]) {
    const double* px = xg + ((size_t)w.tile * R + s) * (size_t)(D * 64) + w.l;
    const double* pS = Sg + ((size_t)w.tile * R + s) * (size_t)(D * (D + 1) / 2 * 64) + w.l;
#pragma unroll
    for (int i = 0; i < N; ++i) mu[i] = px[(O + i) * 64];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int row = (O + i) * (O + i + 1) / 2 + O;
#pragma unroll
        for (int j = 0; j <= i; ++j) S[tix(i, j)] = pS[(row + j) * 64];
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) S[tix(i, j)] = __builtin_fma(mu[i], mu[j], S[tix(i, j)]);
}

struct ScoreArgs {
    LevelDesc lv;
    const double* dts;   // [B, n-1]
    const double* x;     // VEC, centred
    const double* Sig;   // SYM
    const double* Sub;   // FULL, Sigma_{t+1,t} at node t
    double* part;        // [kScorePlanes][Lpad]
    int* info;
    double jitter;
    int allexact;        // every factor exact and no jitter: Q is zero everywhere
    int d;               // the plan's state dimension: strides of the packed arrays only
};

// acc[2 f + 0 | 1] += the contribution of one transition (or of the initial state: no Ga) to slot f's (rate, var): the cotangents
// are first reduced to the factor's own block (kron_marginal), then met by the factor's derivative blocks
template <int D0, int D1, int D2, int F, bool WITH_A, int DF>
MFGM_DEV void score_slot(const TermDesc& td, double dt, const FactorBlk<D0>& f0, const FactorBlk<D1>& f1, const FactorBlk<D2>& f2,
                         const double (&Ga)[D0 * D1 * D2 * D0 * D1 * D2], const double (&Gp)[MFGM_NTRI(D0 * D1 * D2)], double (&acc)[6],
                         const double* lds) {
    if (td.kind[F] == 0) return;
    const FactorDer<DF> g = factor_der<DF>(td.kind[F], td.rate[F], td.var[F], dt);
    double r[DF * DF];
    kron_marginal<D0, D1, D2, F, true>(Gp, f0.p, f1.p, f2.p, r);
    double rate = dot_flat(r, g.dpl);
    acc[2 * F + 1] += dot_flat(r, g.dpv);
    if constexpr (WITH_A) {
        kron_marginal<D0, D1, D2, F, false>(Ga, f0.a, f1.a, f2.a, r, lds);
        rate += dot_flat(r, g.da);
    }
    acc[2 * F] += rate;
}

template <int D0, int D1, int D2, bool WITH_A>
MFGM_DEV void score_contract(const TermDesc& td, double dt, const FactorBlk<D0>& f0, const FactorBlk<D1>& f1, const FactorBlk<D2>& f2,
                             const double (&Ga)[D0 * D1 * D2 * D0 * D1 * D2], const double (&Gp)[MFGM_NTRI(D0 * D1 * D2)],
                             double (&acc)[6], const double* lds = nullptr) {
    // lds: Ga is read from the lane's LDS column (element e at lds[64 e]) instead of from the array
    score_slot<D0, D1, D2, 0, WITH_A, D0>(td, dt, f0, f1, f2, Ga, Gp, acc, lds);
    score_slot<D0, D1, D2, 1, WITH_A, D1>(td, dt, f0, f1, f2, Ga, Gp, acc, lds);
    score_slot<D0, D1, D2, 2, WITH_A, D2>(td, dt, f0, f1, f2, Ga, Gp, acc, lds);
}

// One term of shape (D0, D1, D2) over the lane's segment.  The live set is kept at three n x n arrays: a node's moments are loaded
// again for the transition out of it (a cache hit: the wavefront read them one step earlier) instead of being carried, the
// symmetric matrices stay packed, and the steps below reuse their operands' registers.
template <int NMAX, int D0, int D1, int D2>
MFGM_DEV void score_walk(const ScoreArgs& a, const TermDesc& td0, int b, int p, int len, LaneRef me, double* wl, double (&acc)[6],
                         int& bad) {
    constexpr int N = D0 * D1 * D2, NT = MFGM_NTRI(N);
    constexpr bool PARK = N >= 6;      // W waits in the lane's LDS column while M and G_Q are formed
    constexpr bool PARKM = N >= 8;     // ... and so does the packed M / G_Q / Gp, behind it, until the contraction
    if constexpr (N <= NMAX) {
        TermDesc td = td0;
        const int R = a.lv.R, n = a.lv.n, O = td.offset, D = a.d;
        const double* dtb = a.dts + (size_t)b * (n - 1);
        const int mode = td.nx == 0 ? 0 : (td.nx == 1 ? 1 : 2);
        // the node before the current one: the neighbouring lane's last node in front of the segment's first
        LaneRef prev = LaneRef::of(me.tile * 64 + me.l - 1);
        int sprev = R - 1;
        for (int s = 0; s < len; ++s) {
            const int t = p * R + s;
            // The parameters are made opaque once per node: everything that depends on them alone (Pinf, its derivatives and all
            // their Kronecker products, several hundred values) would otherwise be hoisted out of the loop and held in registers.
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                asm volatile("" : "+s"(td.rate[f]));
                asm volatile("" : "+s"(td.var[f]));
            }
            if (t == 0) {
                // initial state: G_P0 on dPinf
                const FactorBlk<D0> f0 = factor_slot<D0>(td, 0, 0.0, true, td.nx);
                const FactorBlk<D1> f1 = factor_slot<D1>(td, 1, 0.0, true, td.nx);
                const FactorBlk<D2> f2 = factor_slot<D2>(td, 2, 0.0, true, td.nx);
                double P0[NT], invd[N], G[N * N], mu[N], Sc[NT];
#pragma unroll
                for (int i = 0; i < N; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) P0[tix(i, j)] = kron_at<D0, D1, D2>(f0.p, f1.p, f2.p, i, j) + (i == j ? a.jitter : 0.0);
                int bd = 0;
                chol_inplace<N>(P0, invd, bd);
                bad |= bd;
                ld_score_moment<N>(a.x, a.Sig, D, R, s, me, O, mu, Sc);
#pragma unroll
                for (int i = 0; i < N; ++i)
#pragma unroll
                    for (int j = 0; j < N; ++j) G[i * N + j] = Sc[six(i, j)];
                score_cotangent<N>(P0, invd, G);
#pragma unroll
                for (int i = 0; i < N; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) Sc[tix(i, j)] = G[i * N + j];
                score_contract<D0, D1, D2, false>(td, 0.0, f0, f1, f2, G, Sc, acc);
            } else {
                const double dt = dtb[t - 1];
                bool zero = true;
                {
                    // the exact-zero test needs k_kernel_ssm's Q; it is built again after M (from an opaque copy of the gap, or it would
                    // stay in registers through the widest part of the step)
                    const FactorBlk<D0> f0 = factor_slot<D0>(td, 0, dt, false, td.nx);
                    const FactorBlk<D1> f1 = factor_slot<D1>(td, 1, dt, false, td.nx);
                    const FactorBlk<D2> f2 = factor_slot<D2>(td, 2, dt, false, td.nx);
                    double Adead[N * N], Q[NT];     // expand_at's A is not used: the stores are dead
                    expand_at<N, D0, D1, D2, 0>(f0.a, f1.a, f2.a, f0.p, f1.p, f2.p, f0.m, f1.m, f2.m, mode, Adead, Q);
#pragma unroll
                    for (int i = 0; i < N; ++i)
#pragma unroll
                        for (int j = 0; j <= i; ++j) zero = zero && (Q[tix(i, j)] + (i == j ? a.jitter : 0.0) == 0.0);
                }
                if (zero) {
                    // exact-Q rule: a zero block carries no score (zero gap, Constant); next to a non-zero one it is not positive definite
                    if (dt != 0.0 && !a.allexact) bad = 1;
                } else {
                    double dto = dt;
                    asm volatile("" : "+v"(dto));
                    const FactorBlk<D0> f0 = factor_slot<D0>(td, 0, dto, false, td.nx);
                    const FactorBlk<D1> f1 = factor_slot<D1>(td, 1, dto, false, td.nx);
                    const FactorBlk<D2> f2 = factor_slot<D2>(td, 2, dto, false, td.nx);
                    // W = C - A S;  Z = (W + T / 2) A^T with T = A S, so that M = S' - Z - Z^T (T A^T is symmetric);  A and Pinf act
                    // through kron_apply, factor by factor.  W waits in `wl` (LDS for the 6 x 6 and 8 x 8 blocks) until G_A.
                    double W[N * N], M[NT], X[N * N];      // (W is unused, and so unallocated, when it is parked)
                    double* ml = wl + N * N * 64;
                    auto Mr = [&](int e) -> double& {
                        if constexpr (PARKM) return ml[e * 64];
                        else return M[e];
                    };
                    if constexpr (PARK) {
                        // The 6 x 6 and 8 x 8 blocks stream the phase column by column: column k of T = A S is formed from column k
                        // of S alone (kron_vec), turns column k of C (in LDS) into W's, and its Y = W + T / 2 goes straight into
                        // M -= Y[:, k] A[:, k]^T + A[:, k] Y[:, k]^T.  Neither T, Y nor Z is ever an n x n array.
                        double Sp[NT];
                        {
                            double mu[N], mup[N];
                            ld_score_moment<N>(a.x, a.Sig, D, R, sprev, prev, O, mup, Sp);
#pragma unroll
                            for (int i = 0; i < N; ++i) mu[i] = (a.x + ((size_t)me.tile * R + s) * (size_t)(D * 64) + me.l)[(O + i) * 64];
                            const double* pC = a.Sub + ((size_t)prev.tile * R + sprev) * (size_t)(D * D * 64) + prev.l;
#pragma unroll
                            for (int i = 0; i < N; ++i)
#pragma unroll
                                for (int j = 0; j < N; ++j) wl[(i * N + j) * 64] = __builtin_fma(mu[i], mup[j], pC[((O + i) * D + O + j) * 64]);
                            ld_score_moment<N>(a.x, a.Sig, D, R, s, me, O, mu, M);
                            if constexpr (PARKM) {
#pragma unroll
                                for (int e = 0; e < NT; ++e) ml[e * 64] = M[e];
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int k = 0; k < N; ++k) {
                            double v[N], y[N];
#pragma unroll
                            for (int i = 0; i < N; ++i) v[i] = Sp[six(i, k)];
                            kron_vec<D0, D1, D2, false>(f0.a, f1.a, f2.a, v);          // T[:, k]
#pragma unroll
                            for (int i = 0; i < N; ++i) {
                                const double w = wl[(i * N + k) * 64] - v[i];
                                wl[(i * N + k) * 64] = w;
                                y[i] = __builtin_fma(0.5, v[i], w);
                            }
#pragma unroll
                            for (int i = 0; i < N; ++i) v[i] = kron_at<D0, D1, D2>(f0.a, f1.a, f2.a, i, k);      // A[:, k]
#pragma unroll
                            for (int i = 0; i < N; ++i)
#pragma unroll
                                for (int j = 0; j <= i; ++j)
                                    Mr(tix(i, j)) = __builtin_fma(-y[j], v[i], __builtin_fma(-y[i], v[j], Mr(tix(i, j))));
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    } else {
                        {
                            double mu[N], mup[N], Sp[NT];
                            ld_score_moment<N>(a.x, a.Sig, D, R, sprev, prev, O, mup, Sp);
#pragma unroll
                            for (int i = 0; i < N; ++i) mu[i] = (a.x + ((size_t)me.tile * R + s) * (size_t)(D * 64) + me.l)[(O + i) * 64];
                            const double* pC = a.Sub + ((size_t)prev.tile * R + sprev) * (size_t)(D * D * 64) + prev.l;
                            // C = Sigma_{t,t-1} + mu mup^T goes straight to its place (W's registers, or the LDS column)
#pragma unroll
                            for (int i = 0; i < N; ++i)
#pragma unroll
                                for (int j = 0; j < N; ++j) {
                                    const double c = __builtin_fma(mu[i], mup[j], pC[((O + i) * D + O + j) * 64]);
                                    if constexpr (PARK) wl[(i * N + j) * 64] = c;
                                    else W[i * N + j] = c;
                                }
#pragma unroll
                            for (int i = 0; i < N; ++i)
#pragma unroll
                                for (int j = 0; j < N; ++j) X[i * N + j] = Sp[six(i, j)];
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        kron_apply<D0, D1, D2, false, false>(f0.a, f1.a, f2.a, X);          // T = A S
#pragma unroll
                        for (int e = 0; e < N * N; ++e) {
                            double w;
                            if constexpr (PARK) {
                                w = wl[e * 64] - X[e];
                                wl[e * 64] = w;
                            } else {
                                w = W[e] - X[e];
                                W[e] = w;
                            }
                            X[e] = __builtin_fma(0.5, X[e], w);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        kron_apply<D0, D1, D2, false, true>(f0.a, f1.a, f2.a, X);           // Z
                        {
                            double mu[N];
                            ld_score_moment<N>(a.x, a.Sig, D, R, s, me, O, mu, M);
                        }
#pragma unroll
                        for (int i = 0; i < N; ++i)
#pragma unroll
                            for (int j = 0; j <= i; ++j) M[tix(i, j)] -= X[i * N + j] + X[j * N + i];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    double Q[NT], invd[N];
                    {
                        double Adead[N * N];
                        expand_at<N, D0, D1, D2, 0>(f0.a, f1.a, f2.a, f0.p, f1.p, f2.p, f0.m, f1.m, f2.m, mode, Adead, Q);
#pragma unroll
                        for (int i = 0; i < N; ++i) Q[tix(i, i)] += a.jitter;
                    }
                    int bd = 0;
                    chol_inplace<N>(Q, invd, bd);
                    bad |= bd;
#pragma unroll
                    for (int i = 0; i < N; ++i)
#pragma unroll
                        for (int j = 0; j < N; ++j) X[i * N + j] = Mr(six(i, j));
                    __builtin_amdgcn_sched_barrier(0);
                    score_cotangent<N>(Q, invd, X);          // G_Q
#pragma unroll
                    for (int i = 0; i < N; ++i)
#pragma unroll
                        for (int j = 0; j <= i; ++j) Mr(tix(i, j)) = X[i * N + j];
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (PARK) {
                        // G_A = Q^-1 W column by column in the LDS column: W is never a register array
#pragma unroll
                        for (int c = 0; c < N; ++c) {
                            double v[N];
#pragma unroll
                            for (int i = 0; i < N; ++i) v[i] = wl[(i * N + c) * 64];
                            trsv_lower<N>(Q, invd, v);
                            trsv_lower_t<N>(Q, invd, v);
#pragma unroll
                            for (int i = 0; i < N; ++i) wl[(i * N + c) * 64] = v[i];
                        }
                    } else {
                        trsm_left_lower<N>(Q, invd, W);
                        trsm_left_lower_t<N>(Q, invd, W);        // G_A
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    // pull back:  Ga = G_A - 2 G_Q A P (in W);  Gp = G_Q - A^T G_Q A (in M, lower triangle)
#pragma unroll
                    for (int i = 0; i < N; ++i)
#pragma unroll
                        for (int j = 0; j < N; ++j) X[i * N + j] = Mr(six(i, j));
                    kron_apply<D0, D1, D2, true, true>(f0.a, f1.a, f2.a, X);            // G_Q A
                    kron_apply<D0, D1, D2, false, true>(f0.p, f1.p, f2.p, X);           // G_Q A P   (P symmetric)
#pragma unroll
                    for (int e = 0; e < N * N; ++e) {
                        if constexpr (PARK) wl[e * 64] = __builtin_fma(-2.0, X[e], wl[e * 64]);
                        else W[e] = __builtin_fma(-2.0, X[e], W[e]);
                    }
#pragma unroll
                    for (int i = 0; i < N; ++i)
#pragma unroll
                        for (int j = 0; j < N; ++j) X[i * N + j] = Mr(six(i, j));
                    kron_apply<D0, D1, D2, true, true>(f0.a, f1.a, f2.a, X);            // G_Q A
                    kron_apply<D0, D1, D2, true, false>(f0.a, f1.a, f2.a, X);           // A^T G_Q A
#pragma unroll
                    for (int i = 0; i < N; ++i)
#pragma unroll
                        for (int j = 0; j <= i; ++j) Mr(tix(i, j)) -= X[i * N + j];
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (PARKM) {
#pragma unroll
                        for (int e = 0; e < NT; ++e) M[e] = ml[e * 64];
                    }
                    if constexpr (PARK) score_contract<D0, D1, D2, true>(td, dto, f0, f1, f2, X, M, acc, wl);
                    else score_contract<D0, D1, D2, true>(td, dto, f0, f1, f2, W, M, acc);
                }
            }
            prev = me;
            sprev = s;
        }
    }
}

// NMAX: the largest term block of the tree (1, 2, 3, 4, 6 or 8), NOT the plan's d: a Sum of 3 x 3 blocks at d = 8 runs the code of
// 3 x 3 blocks.  The 6 x 6 and 8 x 8 product blocks park one n x n array in LDS (a lane-private column, no barrier).
template <int NMAX>
static __global__ __launch_bounds__(64) void k_kernel_score(ScoreArgs a, KernelTermsDev kt) {
    __shared__ double park[NMAX >= 8 ? (NMAX * NMAX + MFGM_NTRI(NMAX)) * 64 : (NMAX >= 6 ? NMAX * NMAX * 64 : 1)];
    double* wl = park + (NMAX >= 6 ? threadIdx.x : 0);
    const int lane = blockIdx.x * 64 + threadIdx.x;
    if (lane >= a.lv.L) return;
    const LaneRef me{(int)blockIdx.x, (int)threadIdx.x};
    const int P = a.lv.P, R = a.lv.R, n = a.lv.n;
    const int b = lane / P, p = lane - b * P;
    const int len = min(R, n - p * R);
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
            case KT_SHAPE_1: score_walk<NMAX, 1, 1, 1>(a, td, b, p, len, me, wl, acc, bad); break;
            case KT_SHAPE_2: score_walk<NMAX, 2, 1, 1>(a, td, b, p, len, me, wl, acc, bad); break;
            case KT_SHAPE_3: score_walk<NMAX, 3, 1, 1>(a, td, b, p, len, me, wl, acc, bad); break;
            case KT_SHAPE_22: score_walk<NMAX, 2, 2, 1>(a, td, b, p, len, me, wl, acc, bad); break;
            case KT_SHAPE_23: score_walk<NMAX, 2, 3, 1>(a, td, b, p, len, me, wl, acc, bad); break;
            case KT_SHAPE_32: score_walk<NMAX, 3, 2, 1>(a, td, b, p, len, me, wl, acc, bad); break;
            default: score_walk<NMAX, 2, 2, 2>(a, td, b, p, len, me, wl, acc, bad); break;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) a.part[(size_t)(c * 6 + k) * a.lv.Lpad + lane] = acc[k];
    }
    // as in k_kernel_ssm: every writer of this word in the launch writes 1
    if (bad && *a.info == 0) *a.info = 1;
}

// where plane q = 6 c + 2 slot + j of the partials goes in a chain's [8, 3, 2] block (the caller's slot order), -1: nowhere
struct ScoreDest {
    int dst[kScorePlanes];
};

// score[b][dst[q]] = sum_p part[q][b P + p]: one block per (chain, plane), fixed summation order
static __global__ __launch_bounds__(256) void k_score_sum(const double* __restrict__ part, int P, int Lpad, ScoreDest sd,
                                                         double* __restrict__ score) {
    __shared__ double sh[4];
    const int b = blockIdx.x, q = blockIdx.y;
    const int dst = sd.dst[q];
    if (dst < 0) return;
    double s = 0.0;
    for (int p = threadIdx.x; p < P; p += 256) s += part[(size_t)q * Lpad + (size_t)b * P + p];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) score[(size_t)b * kScorePlanes + dst] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

}  // namespace mfgm
