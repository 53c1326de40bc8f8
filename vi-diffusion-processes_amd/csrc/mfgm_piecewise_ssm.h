// ---- piecewise-stationary SDE kernels (change points) -> packed SSM parameters (mfgm_packed_piecewise_ssm, include/mfgm.h) -------
// markovflow/kernels/piecewise_stationary.py `PiecewiseKernel`: K change points c_0 <= ... <= c_{K-1} cut the time axis into K + 1
// regions, region r(t) = #{c_k <= t}; every region has the same term structure (the KernelTermsDev of mfgm_kernel_ssm.h) and its own
// rates, variances and state mean.  The transition t_k -> t_k+1 uses the parameters of r(t_k) (its left end), node 0 holds
// chol(Pinf_r(t_0) + jitter) and a zero mean.
//
// Same lane-per-segment mapping, packed outputs, len + 1 transitions per lane and *info convention as k_kernel_ssm, and the same
// register discipline: the structure is a kernel argument (wave-uniform branches), and NOTHING in registers is indexed by the region.
// A lane carries its region as an integer, found by binary search in the change-point table (global memory, at most a few cache
// lines); the region's rates and variances are loaded from the tables at the point where terms_transition builds a term's TermDesc
// (three slots, compile-time indexed), the region's state mean is kept in D registers and re-read only when the lane's region changes.
// No LDS, no atomics, no scratch.
#pragma once
#include "mfgm_kernel_ssm.h"

namespace mfgm {

struct PiecewiseDev {
    int nregion;              // K + 1 >= 1
    int src[8][3];            // slot f of term c holds the caller's factor src[c][f] (the host moves 1 x 1 factors behind the others)
    const double* cp;         // [nregion - 1] change points, non-decreasing
    const double* rate;       // [nregion, 8, 3] in the caller's factor order
    const double* var;        // [nregion, 8, 3]
    const double* mean;       // [nregion, 8]
};

// r(t) = #{c_k <= t}, in 0 .. nregion - 1 whatever t is (a NaN compares false everywhere: region 0)
MFGM_DEV int pw_region(const PiecewiseDev& pw, double t) {
    int lo = 0, hi = pw.nregion - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pw.cp[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the factor parameters of one region: a row of the tables
struct TermParamsRegion {
    const PiecewiseDev& pw;
    int r;
    MFGM_DEV double rate(int c, int f) const { return pw.rate[(r * 8 + c) * 3 + pw.src[c][f]]; }
    MFGM_DEV double var(int c, int f) const { return pw.var[(r * 8 + c) * 3 + pw.src[c][f]]; }
};

template <int D>
static __global__ __launch_bounds__(64) void k_piecewise_ssm(LevelDesc lv, KernelTermsDev kt, PiecewiseDev pw,
                                                           const double* __restrict__ tps /* [B, n] */, double* __restrict__ Ag,
                                                           double* __restrict__ offg, double* __restrict__ cholg, int* info) {
    constexpr int ET = MFGM_NTRI(D), EF = D * D;
    const int lane = blockIdx.x * 64 + threadIdx.x;
    if (lane >= lv.L) return;
    const LaneRef me{(int)blockIdx.x, (int)threadIdx.x};
    const int P = lv.P, R = lv.R, n = lv.n;
    const int b = lane / P, p = lane - b * P;
    const int len = min(R, n - p * R);
    const double* tpb = tps + (size_t)b * n;
    int bad = 0;
    int rcur = -1;
    double mean[D];
#pragma unroll
    for (int i = 0; i < D; ++i) mean[i] = 0.0;
    // s = -1: the transition into the segment's first node (or the initial state); s >= 0: the transition out of node p R + s
    for (int s = -1; s < len; ++s) {
        const int t = p * R + s;
        double A[EF], Q[ET], off[D];
        const bool init = (t < 0);
        const bool has = (t + 1 < n);
        if (has) {
            // the left end of the transition (the first point itself for the initial state) decides the region
            const double tl = tpb[init ? 0 : t];
            const int r = pw_region(pw, tl);
            if (r != rcur) {
                rcur = r;
#pragma unroll
                for (int i = 0; i < D; ++i) mean[i] = pw.mean[r * 8 + i];
            }
            terms_transition<D>(kt, TermParamsRegion{pw, r}, init ? 0.0 : tpb[t + 1] - tl, init, A, Q);
        } else {
#pragma unroll
            for (int e = 0; e < EF; ++e) A[e] = 0.0;
        }
        if (s >= 0) st_node<EF>(Ag, R, s, me, A);
        if (!has || s + 1 >= len) continue;
        // (Q, b) of node t + 1; the initial mean is zero (SDEKernel.initial_mean, which PiecewiseKernel does not override)
        bool zero = true;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double o = 0.0;
            if (!init) {
                o = mean[i];
#pragma unroll
                for (int k = 0; k < D; ++k) o = __builtin_fma(-A[i * D + k], mean[k], o);
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
