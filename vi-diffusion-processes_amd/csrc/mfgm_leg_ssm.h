// ---- latent exponentially generated (LEG) kernels -> SSM parameters (mfgm_packed_leg_ssm, mfgm_leg_transitions, include/mfgm.h) ----
// markovflow/kernels/latent_exp_generated.py:79-142 `LatentExponentiallyGenerated`: dx = -1/2 G x dt + N dw with G = N N^T + R - R^T,
// so F = -1/2 G, Pinf = I, A(dt) = expm(F dt), Q(dt) = I - A A^T.  The only kernel of the family without a closed-form transition:
// every transition needs a D x D matrix exponential.
//
// Exponential: scaling and squaring on a Taylor polynomial in Horner form.  With theta = |F|_1 dt the lane picks
//   s = 0 for theta <= 1/2, else ilogb(theta) + 2            (theta / 2^s in [1/4, 1/2))
//   m = the smallest degree whose first dropped term (theta / 2^s)^(m+1) / (m+1)! is <= 1e-18   (m <= 15 at 1/2, 7 at 0.01)
// then P = I + (h / m) F, P <- I + (h / k) F P for k = m-1 .. 1 with h = dt / 2^s (exact), and squares P s times.  Everything is a
// function of dt alone, so equal gaps give bit-identical results wherever they sit; dt = 0 gives h = 0, P = I and Q = 0 exactly.
//
// Register discipline, as in mfgm_kernel_ssm.h: every array in registers is indexed at compile time, the loops over the degree and
// over the squarings are runtime loops around fully unrolled D^3 bodies.  No atomics, no scratch.  F travels by value in the kernel
// argument; every lane copies it to D^2 doubles of LDS once (one wavefront per block, identical values from every lane, a barrier
// before any lane leaves), and a Horner step reads it back row by row (all lanes read one address: a broadcast).  In scalar registers
// F would need 2 D^2 of them -- 98 at D = 7, 128 at D = 8, against 102 per wavefront.
//
// k_leg_ssm keeps the lane-per-segment mapping, the packed outputs, the len + 1 transitions per lane and the *info convention of
// k_kernel_ssm.  A lane keeps (dt, A, chol Q, b) of its previous transition in the registers they were computed in and recomputes
// only when the next gap differs: on a uniform grid a lane evaluates one exponential and then only stores.
#pragma once
#include "mfgm_math.h"
#include "mfgm_sweeps.h"

namespace mfgm {

struct LegDev {
    double F[64];         // row-major D x D (stride D)
    double mean[8];
    double jitter;
    double norm1;         // max_j sum_i |F_ij|
};

constexpr int kLegMaxDegree = 18;
constexpr double kLegTruncation = 1e-18;

// every lane of the block: Fs := F (the same values from every lane), then a barrier
template <int D>
MFGM_DEV void leg_stage_feedback(const LegDev& lg, double* Fs) {
#pragma unroll
    for (int e = 0; e < D * D; ++e) Fs[e] = lg.F[e];
    __syncthreads();
}

// P := expm(F dt), F in LDS
template <int D>
MFGM_DEV void leg_expm(const double* Fs, double norm1, double dt, double (&P)[D * D]) {
    const double theta = norm1 * dt;
    int s = 0;
    if (theta > 0.5) s = min(ilogb(theta), 62) + 2;      // a NaN or negative gap: s = 0, the result is whatever the series gives
    const double h = ldexp(dt, -s), th = ldexp(theta, -s);
    int m = 1;
    double term = th;                                     // th^m / m!
    while (m < kLegMaxDegree) {
        term *= th / (double)(m + 1);
        if (!(term > kLegTruncation)) break;
        ++m;
    }
    {
        const double c = h / (double)m;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) P[i * D + j] = __builtin_fma(c, Fs[i * D + j], i == j ? 1.0 : 0.0);
    }
    for (int k = m - 1; k >= 1; --k) {
        const double c = h / (double)k;
        double Pn[D * D];
        // keeps the reads of F inside the step: hoisted out of the loop they would hold 2 D^2 registers next to P and Pn
        asm volatile("" ::: "memory");
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double f[D];
#pragma unroll
            for (int l = 0; l < D; ++l) f[l] = Fs[i * D + l];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int l = 0; l < D; ++l) acc = __builtin_fma(f[l], P[l * D + j], acc);
                Pn[i * D + j] = __builtin_fma(c, acc, i == j ? 1.0 : 0.0);
            }
        }
#pragma unroll
        for (int e = 0; e < D * D; ++e) P[e] = Pn[e];
    }
    for (int r = 0; r < s; ++r) {
        double Pn[D * D];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int l = 0; l < D; ++l) acc = __builtin_fma(P[i * D + l], P[l * D + j], acc);
                Pn[i * D + j] = acc;
            }
#pragma unroll
        for (int e = 0; e < D * D; ++e) P[e] = Pn[e];
    }
}

// lower triangle of Q = I - A A^T + jitter I (the same sum for (i, j) and (j, i): symmetric by construction)
template <int D>
MFGM_DEV void leg_noise(const LegDev& lg, const double (&A)[D * D], double (&Q)[MFGM_NTRI(D)]) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double q = (i == j ? 1.0 : 0.0);
#pragma unroll
            for (int k = 0; k < D; ++k) q = __builtin_fma(-A[i * D + k], A[j * D + k], q);
            Q[tix(i, j)] = q + (i == j ? lg.jitter : 0.0);
        }
}

template <int D>
static __global__ __launch_bounds__(64) void k_leg_ssm(LevelDesc lv, LegDev lg, const double* __restrict__ dts /* [B, n-1] */,
                                                     double* __restrict__ Ag, double* __restrict__ offg, double* __restrict__ cholg,
                                                     int* info) {
    constexpr int ET = MFGM_NTRI(D), EF = D * D;
    __shared__ double Fs[EF];
    leg_stage_feedback<D>(lg, Fs);
    const int lane = blockIdx.x * 64 + threadIdx.x;
    if (lane >= lv.L) return;
    const LaneRef me{(int)blockIdx.x, (int)threadIdx.x};
    const int P = lv.P, R = lv.R, n = lv.n;
    const int b = lane / P, p = lane - b * P;
    const int len = min(R, n - p * R);
    const double* dtb = dts + (size_t)b * (n - 1);
    int bad = 0;
    // the lane's previous transition: recomputed only when the gap changes (a NaN gap never compares equal)
    double A[EF], C[ET], off[D];
    double dprev = __builtin_nan("");
    // s = -1: the transition into the segment's first node (or the initial state); s >= 0: the transition out of node p R + s
    for (int s = -1; s < len; ++s) {
        const int t = p * R + s;
        if (t < 0) {
            // node 0: (m, chol((1 + jitter) I))
            double c0[ET], m0[D], invd[D];
#pragma unroll
            for (int e = 0; e < ET; ++e) c0[e] = 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                c0[tix(i, i)] = 1.0 + lg.jitter;
                m0[i] = lg.mean[i];
            }
            int bd = 0;
            chol_inplace<D>(c0, invd, bd);
            bad |= bd;
            st_node<D>(offg, R, 0, me, m0);
            st_node<ET>(cholg, R, 0, me, c0);
            continue;
        }
        if (t + 1 >= n) {       // the chain's last node has no transition out of it
            st_node_zero<EF>(Ag, R, s, me);
            continue;
        }
        // At the segment's last slot only A is stored (the next lane writes the node's (Q, b)); Q, b and the factor are computed
        // there all the same, so that the kept tuple always belongs to one gap -- one unused Cholesky per segment on irregular grids.
        const double dt = dtb[t];
        if (!(dt == dprev)) {
            dprev = dt;
            leg_expm<D>(Fs, lg.norm1, dt, A);
            leg_noise<D>(lg, A, C);
            bool zero = true;
#pragma unroll
            for (int e = 0; e < ET; ++e) zero = zero && (C[e] == 0.0);
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double o = lg.mean[i];
#pragma unroll
                for (int k = 0; k < D; ++k) o = __builtin_fma(-A[i * D + k], lg.mean[k], o);
                off[i] = o;
            }
            if (zero) {
#pragma unroll
                for (int i = 0; i < D; ++i) C[tix(i, i)] = 1.0;   // cholesky_or_zero: factor the identity, store zeros
            }
            double invd[D];
            int bd = 0;
            chol_inplace<D>(C, invd, bd);
            bad |= bd;
            if (zero) {
#pragma unroll
                for (int e = 0; e < ET; ++e) C[e] = 0.0;
            }
        }
        if (s >= 0) st_node<EF>(Ag, R, s, me, A);
        if (s + 1 < len) {      // (Q, b) of node t + 1 (the next segment's lane writes its own first node)
            st_node<D>(offg, R, s + 1, me, off);
            st_node<ET>(cholg, R, s + 1, me, C);
        }
    }
    // the only writers of this word in the launch all write 1 (same effect as atomicMax(info, 1) after the stream's earlier work)
    if (bad && *info == 0) *info = 1;
}

// (A, Q) of n arbitrary non-negative gaps in natural layout, one lane per gap: A [n, D, D], Q [n, D, D] = I - A A^T + jitter I
template <int D>
static __global__ __launch_bounds__(64) void k_leg_transitions(LegDev lg, long n, const double* __restrict__ dts,
                                                             double* __restrict__ Ag, double* __restrict__ Qg) {
    constexpr int ET = MFGM_NTRI(D), EF = D * D;
    __shared__ double Fs[EF];
    leg_stage_feedback<D>(lg, Fs);
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= (size_t)n) return;
    double A[EF], Q[ET];
    leg_expm<D>(Fs, lg.norm1, dts[i], A);
    leg_noise<D>(lg, A, Q);
    double* a = Ag + i * EF;
    double* q = Qg + i * EF;
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int c = 0; c < D; ++c) {
            a[r * D + c] = A[r * D + c];
            q[r * D + c] = Q[six(r, c)];
        }
}

}  // namespace mfgm
