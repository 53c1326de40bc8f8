// ---- mean functions of a driven kernel SDE: impulse and step responses (mfgm_action_coefficients / mfgm_action_mean, include/mfgm.h) --
// markovflow/mean_function.py `ImpulseMeanFunction`, `StepMeanFunction`: the deterministic response of dx = F x dt + u(t) dt + L dw to
// actions at the times t_0 <= ... <= t_{K-1}.  With j = #{k : t_k < t} and k = j - 1:  mu(t) = shift_k + A(t - t_k) c_k  (zero for
// j = 0), where  c_k = A(t_k - t_{k-1}) c_{k-1} + rhs_k,  c_{-1} = 0.
//
// The recurrence is serial in K, but stationary transitions form a semigroup, A(a) A(b) = A(a + b), so the scan over segments of
// `seg` actions needs no matrix products and no transition is ever stored:
//   k_action_local   one lane per (chain, segment): the recurrence from zero over the segment, local prefixes -> coef, the segment's
//                    last value p_s -> ends;
//   k_action_ends    one lane per chain: C_s = A(T_s - T_{s-1}) C_{s-1} + p_s over the segment ends T_s (in place in ends);
//   k_action_apply   one lane per action of the segments s >= 1: coef_k += A(t_k - T_{s-1}) C_{s-1}; the gap is a difference of two
//                    times, not a sum of gaps.
// Every output entry has one owner and a fixed order of operations: no atomics, two calls give identical bits.
//
// The evaluation (k_action_mean) is one lane per query point: binary search in the chain's action times (global memory through the
// cache: the lanes of a wave share the lines), A(t - t_k) from terms_transition<D> in registers, the d x d mat-vec, the shift and the
// dot product with the emission row in the same lane.
//
// Register discipline as mfgm_kernel_ssm.h: the term structure is a kernel argument (wave-uniform branches), nothing in registers is
// indexed by a runtime value; the Q that terms_transition also builds is never read here and is removed as dead code.  No LDS, no
// scratch.
#pragma once
#include "mfgm_kernel_ssm.h"

namespace mfgm {

// A(dt) alone
template <int D>
MFGM_DEV void action_transition(const KernelTermsDev& kt, double dt, double (&A)[D * D]) {
    double Q[MFGM_NTRI(D)];
    terms_transition<D>(kt, TermParamsArg{kt}, dt, false, A, Q);
}

// y := add + A x  (fma chain onto add, ascending column)
template <int D>
MFGM_DEV void action_affine(const double (&A)[D * D], const double (&x)[D], const double (&add)[D], double (&y)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double t = add[i];
#pragma unroll
        for (int k = 0; k < D; ++k) t = __builtin_fma(A[i * D + k], x[k], t);
        y[i] = t;
    }
}

// the last action of segment s: min(K, (s + 1) seg) - 1
MFGM_DEV int action_seg_last(int K, int seg, int s) {
    const long long e = ((long long)s + 1) * seg;
    return (int)(e < K ? e : K) - 1;
}

// coef may alias rhs: a lane reads rhs_k before it writes coef_k, and no other lane touches that entry
template <int D>
static __global__ __launch_bounds__(64) void k_action_local(KernelTermsDev kt, int B, int K, int seg, int S,
                                                          const double* __restrict__ times /* [B, K] */, const double* rhs /* [B, K, D] */,
                                                          double* coef /* [B, K, D] */, double* __restrict__ ends /* [B, S, D] */) {
    const long long lane = (long long)blockIdx.x * 64 + threadIdx.x;
    if (lane >= (long long)B * S) return;
    const int b = (int)(lane / S), s = (int)(lane - (long long)b * S);
    const int k0 = (int)((long long)s * seg), k1 = action_seg_last(K, seg, s) + 1;
    const double* tb = times + (size_t)b * K;
    double c[D];
#pragma unroll
    for (int i = 0; i < D; ++i) c[i] = 0.0;
    double tprev = tb[k0];
    for (int k = k0; k < k1; ++k) {
        const size_t at = ((size_t)b * K + k) * D;
        const double t = tb[k];
        double r[D];
#pragma unroll
        for (int i = 0; i < D; ++i) r[i] = rhs[at + i];
        if (k > k0) {
            double A[D * D], n[D];
            action_transition<D>(kt, t - tprev, A);
            action_affine<D>(A, c, r, n);
#pragma unroll
            for (int i = 0; i < D; ++i) c[i] = n[i];
        } else {
#pragma unroll
            for (int i = 0; i < D; ++i) c[i] = r[i];
        }
#pragma unroll
        for (int i = 0; i < D; ++i) coef[at + i] = c[i];
        tprev = t;
    }
    const size_t eo = (size_t)lane * D;
#pragma unroll
    for (int i = 0; i < D; ++i) ends[eo + i] = c[i];
}

template <int D>
static __global__ __launch_bounds__(64) void k_action_ends(KernelTermsDev kt, int B, int K, int seg, int S,
                                                         const double* __restrict__ times, double* __restrict__ ends) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double* tb = times + (size_t)b * K;
    double* eb = ends + (size_t)b * S * D;
    double c[D];
#pragma unroll
    for (int i = 0; i < D; ++i) c[i] = eb[i];
    double tprev = tb[action_seg_last(K, seg, 0)];
    for (int s = 1; s < S; ++s) {
        const double t = tb[action_seg_last(K, seg, s)];
        double A[D * D], p[D], n[D];
#pragma unroll
        for (int i = 0; i < D; ++i) p[i] = eb[(size_t)s * D + i];
        action_transition<D>(kt, t - tprev, A);
        action_affine<D>(A, c, p, n);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            c[i] = n[i];
            eb[(size_t)s * D + i] = n[i];
        }
        tprev = t;
    }
}

template <int D>
static __global__ __launch_bounds__(64) void k_action_apply(KernelTermsDev kt, int B, int K, int seg, int S,
                                                          const double* __restrict__ times, const double* __restrict__ ends,
                                                          double* __restrict__ coef) {
    // the actions of segment 0 are final already: lanes over k = seg .. K - 1 of every chain
    const int Kr = K - seg;
    const long long lane = (long long)blockIdx.x * 64 + threadIdx.x;
    if (lane >= (long long)B * Kr) return;
    const int b = (int)(lane / Kr), k = seg + (int)(lane - (long long)b * Kr);
    const int s = k / seg;
    const double* tb = times + (size_t)b * K;
    const size_t at = ((size_t)b * K + k) * D;
    double A[D * D], C[D], l[D], n[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        C[i] = ends[((size_t)b * S + s - 1) * D + i];
        l[i] = coef[at + i];
    }
    action_transition<D>(kt, tb[k] - tb[action_seg_last(K, seg, s - 1)], A);
    action_affine<D>(A, C, l, n);
#pragma unroll
    for (int i = 0; i < D; ++i) coef[at + i] = n[i];
}

struct ActionMeanArgs {
    int B, K;
    long long N;
    const double* times;   // [B, K]
    const double* coef;    // [B, K, D]
    const double* shift;   // [B, K, D] or null
    const double* tps;     // [B, N]
    double* state_mean;    // [B, N, D] or null
    double* f_mean;        // [B, N] or null
    double emission[8];
};

template <int D>
static __global__ __launch_bounds__(64) void k_action_mean(KernelTermsDev kt, ActionMeanArgs a) {
    const long long lane = (long long)blockIdx.x * 64 + threadIdx.x;
    if (lane >= (long long)a.B * a.N) return;
    const int b = (int)(lane / a.N);
    const double* tb = a.times + (size_t)b * a.K;
    const double t = a.tps[lane];
    // j = #{k : t_k < t}: an action is not seen at its own time (a NaN compares false everywhere: j = 0)
    int lo = 0, hi = a.K;
    while (lo < hi) {
        const int mid = (int)(((long long)lo + hi) >> 1);
        if (tb[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    double mu[D];
#pragma unroll
    for (int i = 0; i < D; ++i) mu[i] = 0.0;
    if (lo > 0) {
        const int k = lo - 1;
        const size_t at = ((size_t)b * a.K + k) * D;
        double A[D * D], c[D], sh[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            c[i] = a.coef[at + i];
            sh[i] = a.shift ? a.shift[at + i] : 0.0;
        }
        action_transition<D>(kt, t - tb[k], A);
        action_affine<D>(A, c, sh, mu);
    }
    if (a.state_mean) {
#pragma unroll
        for (int i = 0; i < D; ++i) a.state_mean[(size_t)lane * D + i] = mu[i];
    }
    if (a.f_mean) {
        double f = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) f = __builtin_fma(a.emission[i], mu[i], f);
        a.f_mean[lane] = f;
    }
}

}  // namespace mfgm
