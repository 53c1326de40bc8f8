// ---- kernel score of the PANEL's sparse-CVI bound through the conditionals of its B N data points (mfgm_panel_cond_score) -----------
// DESIGN.md section 27.  The reverse mode of mfgm_sparse_score.h (cond_score_lane / cond_score_term, unchanged) for the points of B
// series that share one kernel and one inducing grid: the forms touch the posterior in one place, pair_cotangent, and the panel's
// reads the pair (state m - 1, state m) of chain b out of the PACKED x (VEC), Sig (SYM), Sub (FULL) of the B-chain lane-per-segment
// plan -- chain b, node t at lane b P + t / R, step t mod R, element e of a node 64 doubles after element e - 1 -- where the
// single-chain kernel reads natural [M, d] arrays.  The sums run in the single-chain kernel's order, so a series gives the bits it
// gives there.
//
// One lane per (series, point) over the flattened B N points, 64 lanes per workgroup; series boundaries fall anywhere in a wavefront.
// The interval comes from idx[b, i] (clamped to 0 .. M); neighbouring lanes are neighbouring points of one series and mostly read the
// same packed addresses.  The lanes of a wavefront are summed by the fixed shuffle tree of cond_score_lane, the wavefronts by
// k_score_sum in index order: the score is summed over the series, no floating-point atomics, two launches agree bit for bit.
#pragma once
#include "mfgm_panel.h"
#include "mfgm_sparse_score.h"

namespace mfgm {

struct PanelScoreArgs {
    PanelArgs sp;            // idx, w, prior_mean, prior_cov are read; seg and c are not
    const double* gap_lo;    // [B, N] t - z-  (the caller pads the ends)
    const double* gap_hi;    // [B, N] z+ - t
    const double* a;         // [B, N] d ve / d fmu   (0 for an absent point)
    const double* b;         // [B, N] d ve / d fvar
    const double* x;         // packed VEC
    const double* Sig;       // packed SYM
    const double* Sub;       // packed FULL, Sigma_{t+1,t} at t
    double* part;            // [kScorePlanes][nblk]
    int* info;
    double jitter;
    int nblk;
};

// What cond_score_term reads of its argument struct, for one lane: the packed positions of the two states of the point's pair.
struct PanelScoreLane {
    PanelArgs sp;
    double jitter;
    const double* x;
    const double* Sig;
    const double* Sub;
    size_t n_lo, n_hi;       // packed node of state m - 1 / state m (clamped where the prior stands in: the address is then not read)
    int q_lo, q_hi;          // their lane within the wave tile
};

// pair_cotangent of mfgm_sparse_score.h on the packed moments: the same sums in the same order
template <int N>
MFGM_DEV void pair_cotangent(const PanelScoreLane& A, int m, bool hi, int O, const double* __restrict__ w, double av, double bv,
                             double (&wb)[N]) {
    const int d = A.sp.d, M = A.sp.M;
    const bool lo_prior = (m == 0), hi_prior = (m == M);
    const bool prior = hi ? hi_prior : lo_prior;
    const size_t node = hi ? A.n_hi : A.n_lo;
    const int q = hi ? A.q_hi : A.q_lo;
    const double* S = A.Sig + node * (size_t)(d * (d + 1) / 2) * 64 + q;      // lower triangle, element tix(i, j)
    const double* mean = A.x + node * (size_t)d * 64 + q;
    const double* C = (lo_prior || hi_prior) ? nullptr : A.Sub + A.n_lo * (size_t)(d * d) * 64 + A.q_lo;      // Cov(x_hi, x_lo)
    const double* wsame = w + (hi ? d : 0);
    const double* wother = w + (hi ? 0 : d);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int r = O + i;
        double t = 0.0;
        for (int j = 0; j < d; ++j) t = __builtin_fma(prior ? A.sp.prior_cov[r * d + j] : S[six(r, j) * 64], wsame[j], t);
        if (C) {
            for (int j = 0; j < d; ++j) t = __builtin_fma(hi ? C[(r * d + j) * 64] : C[(j * d + r) * 64], wother[j], t);
        }
        wb[i] = __builtin_fma(av, prior ? A.sp.prior_mean[r] : mean[r * 64], 2.0 * bv * t);
    }
}

template <int NMAX>
static __global__ __launch_bounds__(64) void k_panel_cond_score(PanelScoreArgs U, LevelDesc lv, KernelTermsDev kt) {
    const size_t gi = (size_t)blockIdx.x * 64 + threadIdx.x, total = (size_t)U.sp.B * U.sp.N;
    const bool active = gi < total;
    const size_t k = active ? gi : total - 1;      // idle lanes of the last wavefront repeat the last point and add nothing
    const int b = (int)(k / U.sp.N), M = U.sp.M;
    const int m = min(max(U.sp.idx[k], 0), M);
    PanelScoreLane A;
    A.sp = U.sp;
    A.jitter = U.jitter;
    A.x = U.x; A.Sig = U.Sig; A.Sub = U.Sub;
    // the packed positions of the nodes m - 1 and m of chain b, as k_panel_predict finds them
    const int t_lo = (m == 0) ? 0 : m - 1, t_hi = (m == M) ? M - 1 : m;
    const int p_lo = t_lo / lv.R, p_hi = t_hi / lv.R;
    const size_t l_lo = (size_t)b * lv.P + p_lo, l_hi = (size_t)b * lv.P + p_hi;
    A.n_lo = (l_lo >> 6) * lv.R + (t_lo - p_lo * lv.R);
    A.n_hi = (l_hi >> 6) * lv.R + (t_hi - p_hi * lv.R);
    A.q_lo = (int)(l_lo & 63);
    A.q_hi = (int)(l_hi & 63);
    const double* w = U.sp.w + k * (size_t)(2 * U.sp.d);
    const int bad = cond_score_lane<NMAX>(A, kt, m, w, U.gap_lo[k], U.gap_hi[k], U.a[k], U.b[k], active, U.part, U.nblk);
    // as in k_kernel_ssm: every writer of this word in the launch writes 1
    if (bad && *U.info == 0) *U.info = 1;
}

}  // namespace mfgm
