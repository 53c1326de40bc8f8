// ---- sums of products of stationary SDE kernels -> packed SSM parameters (mfgm_packed_kernel_ssm, include/mfgm.h) -------------
// Terms (Sum / ConcatKernel, kernels/sde_kernel.py:540-687) of up to 3 factors each (Product, sde_kernel.py:691-826): Matern-1/2 /
// OU, -3/2, -5/2 (kernels/matern.py:27-520), Constant (kernels/constant.py:28-153), HarmonicOscillator (kernels/periodic.py:27-203).
// Same lane-per-segment mapping and packed outputs as k_stationary_ssm (mfgm_local.h).
//
// Register discipline (no scratch, no LDS, no atomics): the term structure is a kernel argument, so every branch on it is
// wave-uniform, and nothing in registers is indexed by a runtime value.  The host moves a term's 1 x 1 factors (Matern-1/2 / OU,
// Constant: scalars, which commute through a Kronecker product) behind its 2 x 2 and 3 x 3 ones; the remaining "shape" -- (), (2),
// (3), (2,2), (2,3), (3,2), (2,2,2) -- and the term's offset select a compile-time instantiation (a uniform switch), inside which the
// factor blocks are sized and indexed at compile time and Kronecker-expanded straight into the term's diagonal block of A and Q.
//
// Each lane builds len + 1 transitions instead of 2 len: the transition t -> t+1 gives A of node t and (Q, b) of node t + 1, so a
// harmonic factor costs one sincos per node.
#pragma once
#include "mfgm_math.h"
#include "mfgm_sweeps.h"

namespace mfgm {

struct KernelTermsDev {
    int nterm;
    int shape[8];         // KT_SHAPE_* of the term's non-scalar factors (slots 0 ..), scalar / absent slots after them
    int offset[8];        // first state index of the term
    int kind[8][3];       // MFGM_FACTOR_*; 0 = absent slot (1 x 1 identity)
    double rate[8][3];
    double var[8][3];
    double mean[8];
    double jitter;
};

// the fields of one term, read once per term from the kernel argument (read from it inside every offset instantiation below, the
// argument would be copied to scratch)
struct TermDesc {
    int offset, nx;
    int kind[3];
    double rate[3], var[3];
};

enum { KT_SHAPE_1 = 0, KT_SHAPE_2, KT_SHAPE_3, KT_SHAPE_22, KT_SHAPE_23, KT_SHAPE_32, KT_SHAPE_222 };

MFGM_DEV constexpr bool factor_exact(int kind) { return kind == MFGM_FACTOR_CONSTANT || kind == MFGM_FACTOR_HARMONIC || kind == 0; }

// Factor block A_f(dt) and P_f (row-major DF x DF) of a factor of state dimension DF.  The Matern entries are k_stationary_ssm's
// expressions.
template <int DF>
MFGM_DEV void factor_blocks(int kind, double l, double v, double dt, double (&a)[DF * DF], double (&p)[DF * DF]) {
#pragma unroll
    for (int e = 0; e < DF * DF; ++e) { a[e] = 0.0; p[e] = 0.0; }
    if constexpr (DF == 1) {
        if (kind == MFGM_FACTOR_MATERN12) {
            a[0] = exp(-l * dt);
            p[0] = v;
        } else if (kind == MFGM_FACTOR_CONSTANT) {
            a[0] = 1.0;
            p[0] = v;
        } else {   // absent slot
            a[0] = 1.0;
            p[0] = 1.0;
        }
    } else if constexpr (DF == 2) {
        if (kind == MFGM_FACTOR_MATERN32) {
            const double ex = exp(-l * dt);
            a[0] = ex * (1.0 + l * dt);
            a[1] = ex * dt;
            a[2] = ex * (-l * l * dt);
            a[3] = ex * (1.0 - l * dt);
            p[0] = v;
            p[3] = v * l * l;
        } else {   // MFGM_FACTOR_HARMONIC
            double s, c;
            sincos(l * dt, &s, &c);
            a[0] = c;
            a[1] = -s;
            a[2] = s;
            a[3] = c;
            p[0] = v;
            p[3] = v;
        }
    } else {       // MFGM_FACTOR_MATERN52
        const double ex = exp(-l * dt);
        const double l2 = l * l, l3 = l2 * l, l4 = l2 * l2, h = 0.5 * dt * dt;
        a[0] = ex * (1.0 + l * dt + l2 * h);
        a[1] = ex * (dt + 2.0 * l * h);
        a[2] = ex * h;
        a[3] = ex * (-l3 * h);
        a[4] = ex * (1.0 + l * dt - 2.0 * l2 * h);
        a[5] = ex * (dt - l * h);
        a[6] = ex * (-l3 * dt + l4 * h);
        a[7] = ex * (-3.0 * l2 * dt + 2.0 * l3 * h);
        a[8] = ex * (1.0 - 2.0 * l * dt + l2 * h);
        const double l23 = l * l / 3.0;
        p[0] = v;
        p[2] = -v * l23;
        p[6] = -v * l23;
        p[4] = v * l23;
        p[8] = v * l * l * l * l;
    }
}

// m := P - A P A^T (diff) or A P A^T, in k_stationary_ssm's operation order (A P by fma from 0, then fma(-AP, A^T) onto P; that
// kernel's extra terms outside the block are exact zeros), so a Matern term alone reproduces its Q bit for bit.
template <int DF>
MFGM_DEV void factor_noise(const double (&a)[DF * DF], const double (&p)[DF * DF], bool diff, double (&m)[DF * DF]) {
    double ap[DF * DF];
#pragma unroll
    for (int i = 0; i < DF; ++i)
#pragma unroll
        for (int j = 0; j < DF; ++j) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < DF; ++k) t = __builtin_fma(a[i * DF + k], p[k * DF + j], t);
            ap[i * DF + j] = t;
        }
#pragma unroll
    for (int i = 0; i < DF; ++i)
#pragma unroll
        for (int j = 0; j < DF; ++j) {
            double q = diff ? p[i * DF + j] : 0.0;
#pragma unroll
            for (int k = 0; k < DF; ++k) q = __builtin_fma(diff ? -ap[i * DF + k] : ap[i * DF + k], a[j * DF + k], q);
            m[i * DF + j] = q;
        }
}

// Factor slot f of term c: A_f, P_f and the Q operand m (P_g - M_g for the one inexact factor g, M_f when there are several inexact
// factors, P_f for the exact kinds and on the initial node).  Returned by value: the optimiser would otherwise merge the identical
// code of two 1 x 1 slots into stores through a selected pointer, which no longer fit in registers.
template <int DF>
struct FactorBlk {
    double a[DF * DF], p[DF * DF], m[DF * DF];
};

template <int DF>
MFGM_DEV FactorBlk<DF> factor_slot(const TermDesc& td, int f, double dt, bool init, int nx) {
    FactorBlk<DF> r;
    const int kind = td.kind[f];
    factor_blocks<DF>(kind, td.rate[f], td.var[f], dt, r.a, r.p);
    if (init || factor_exact(kind)) {
#pragma unroll
        for (int e = 0; e < DF * DF; ++e) r.m[e] = r.p[e];
    } else {
        factor_noise<DF>(r.a, r.p, nx == 1, r.m);
    }
    return r;
}

// mode: 0 Q_term = 0, 1 Q_term = (x) m_f (one inexact factor), 2 Q_term = (x) p_f - (x) m_f, 3 Pinf block = (x) p_f (initial node)
template <int D, int D0, int D1, int D2, int O>
MFGM_DEV void expand_at(const double (&a0)[D0 * D0], const double (&a1)[D1 * D1], const double (&a2)[D2 * D2],
                        const double (&p0)[D0 * D0], const double (&p1)[D1 * D1], const double (&p2)[D2 * D2],
                        const double (&m0)[D0 * D0], const double (&m1)[D1 * D1], const double (&m2)[D2 * D2], int mode,
                        double (&A)[D * D], double (&Q)[MFGM_NTRI(D)]) {
    constexpr int n = D0 * D1 * D2;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        const int i0 = i / (D1 * D2), i1 = (i / D2) % D1, i2 = i % D2;
#pragma unroll
        for (int j = 0; j < n; ++j) {
            const int j0 = j / (D1 * D2), j1 = (j / D2) % D1, j2 = j % D2;
            const int e0 = i0 * D0 + j0, e1 = i1 * D1 + j1, e2 = i2 * D2 + j2;
            if (mode != 3) A[(O + i) * D + O + j] = a0[e0] * a1[e1] * a2[e2];
            if (j > i) continue;
            double q = 0.0;
            if (mode == 1) q = m0[e0] * m1[e1] * m2[e2];
            else if (mode == 2) q = p0[e0] * p1[e1] * p2[e2] - m0[e0] * m1[e1] * m2[e2];
            else if (mode == 3) q = p0[e0] * p1[e1] * p2[e2];
            Q[tix(O + i, O + j)] = q;
        }
    }
}

// the term of shape (D0, D1, D2) at the uniform offset o: one compile-time instantiation per admissible offset
template <int D, int D0, int D1, int D2, int O = 0>
MFGM_DEV void expand_shape(const TermDesc& td, double dt, bool init, double (&A)[D * D], double (&Q)[MFGM_NTRI(D)]) {
    if constexpr (O + D0 * D1 * D2 <= D) {
        if (td.offset != O) {
            expand_shape<D, D0, D1, D2, O + 1>(td, dt, init, A, Q);
            return;
        }
        const FactorBlk<D0> f0 = factor_slot<D0>(td, 0, dt, init, td.nx);
        const FactorBlk<D1> f1 = factor_slot<D1>(td, 1, dt, init, td.nx);
        const FactorBlk<D2> f2 = factor_slot<D2>(td, 2, dt, init, td.nx);
        const int mode = init ? 3 : (td.nx == 0 ? 0 : (td.nx == 1 ? 1 : 2));
        expand_at<D, D0, D1, D2, O>(f0.a, f1.a, f2.a, f0.p, f1.p, f2.p, f0.m, f1.m, f2.m, mode, A, Q);
    }
}

// where a transition's factor parameters come from: the kernel argument (one set for the whole grid) ...
struct TermParamsArg {
    const KernelTermsDev& kt;
    MFGM_DEV double rate(int c, int f) const { return kt.rate[c][f]; }
    MFGM_DEV double var(int c, int f) const { return kt.var[c][f]; }
};
// ... or anything else with rate(c, f) / var(c, f) of term c, slot f (mfgm_piecewise_ssm.h: a lane's row of the region tables)

// One transition of length dt: A (full) and Q without jitter (packed lower); init: Q := Pinf and A untouched.  The structure of the
// terms is kt's, their rates and variances are prm's.
template <int D, class Params>
MFGM_DEV void terms_transition(const KernelTermsDev& kt, const Params& prm, double dt, bool init, double (&A)[D * D],
                               double (&Q)[MFGM_NTRI(D)]) {
    if (!init) {
#pragma unroll
        for (int e = 0; e < D * D; ++e) A[e] = 0.0;
    }
#pragma unroll
    for (int e = 0; e < MFGM_NTRI(D); ++e) Q[e] = 0.0;
    for (int c = 0; c < kt.nterm; ++c) {
        TermDesc td;
        td.offset = kt.offset[c];
        td.nx = 0;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            td.kind[f] = kt.kind[c][f];
            td.rate[f] = prm.rate(c, f);
            td.var[f] = prm.var(c, f);
            td.nx += factor_exact(td.kind[f]) ? 0 : 1;
        }
        switch (kt.shape[c]) {
            case KT_SHAPE_1: expand_shape<D, 1, 1, 1>(td, dt, init, A, Q); break;
            case KT_SHAPE_2: expand_shape<D, 2, 1, 1>(td, dt, init, A, Q); break;
            case KT_SHAPE_3: expand_shape<D, 3, 1, 1>(td, dt, init, A, Q); break;
            case KT_SHAPE_22: expand_shape<D, 2, 2, 1>(td, dt, init, A, Q); break;
            case KT_SHAPE_23: expand_shape<D, 2, 3, 1>(td, dt, init, A, Q); break;
            case KT_SHAPE_32: expand_shape<D, 3, 2, 1>(td, dt, init, A, Q); break;
            default: expand_shape<D, 2, 2, 2>(td, dt, init, A, Q); break;
        }
    }
}

template <int D>
static __global__ __launch_bounds__(64) void k_kernel_ssm(LevelDesc lv, KernelTermsDev kt, const double* __restrict__ dts /* [B, n-1] */,
                                                        double* __restrict__ Ag, double* __restrict__ offg, double* __restrict__ cholg,
                                                        int* info) {
    constexpr int ET = MFGM_NTRI(D), EF = D * D;
    const int lane = blockIdx.x * 64 + threadIdx.x;
    if (lane >= lv.L) return;
    const LaneRef me{(int)blockIdx.x, (int)threadIdx.x};
    const int P = lv.P, R = lv.R, n = lv.n;
    const int b = lane / P, p = lane - b * P;
    const int len = min(R, n - p * R);
    const double* dtb = dts + (size_t)b * (n - 1);
    int bad = 0;
    // s = -1: the transition into the segment's first node (or the initial state); s >= 0: the transition out of node p R + s
    for (int s = -1; s < len; ++s) {
        const int t = p * R + s;
        double A[EF], Q[ET], off[D];
        const bool init = (t < 0);
        const bool has = (t + 1 < n);
        if (has) {
            terms_transition<D>(kt, TermParamsArg{kt}, init ? 0.0 : dtb[t], init, A, Q);
        } else {
#pragma unroll
            for (int e = 0; e < EF; ++e) A[e] = 0.0;
        }
        if (s >= 0) {
            if (!has) {
#pragma unroll
                for (int e = 0; e < EF; ++e) A[e] = 0.0;
            }
            st_node<EF>(Ag, R, s, me, A);
        }
        if (!has || s + 1 >= len) continue;
        // (Q, b) of node t + 1
        bool zero = true;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double o = kt.mean[i];
            if (!init) {
#pragma unroll
                for (int k = 0; k < D; ++k) o = __builtin_fma(-A[i * D + k], kt.mean[k], o);
            }
            off[i] = o;
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                Q[tix(i, j)] += (i == j ? kt.jitter : 0.0);
                zero = zero && (Q[tix(i, j)] == 0.0);
            }
        }
        zero = zero && !init;
        if (zero) {
#pragma unroll
            for (int i = 0; i < D; ++i) Q[tix(i, i)] = 1.0;   // cholesky_or_zero: factor the identity, store zeros
        }
        double invd[D];
        int bd = 0;
        chol_inplace<D>(Q, invd, bd);
        bad |= bd;
        if (zero) {
#pragma unroll
            for (int e = 0; e < ET; ++e) Q[e] = 0.0;
        }
        st_node<D>(offg, R, s + 1, me, off);
        st_node<ET>(cholg, R, s + 1, me, Q);
    }
    // the only writers of this word in the launch all write 1 (same effect as atomicMax(info, 1) after the stream's earlier work)
    if (bad && *info == 0) *info = 1;
}

}  // namespace mfgm
