// Seeded draws from a factorised Gauss-Markov precision (lane-per-segment plans, d <= 8): with the natural-order block Cholesky
// factor Lambda = L L^T of a form-0 factorisation and y = L^{-1} r,
//
//        x = L^{-T} (y + eps),     x_t = L_tt^{-T} (y_t + eps_t - G_t^T x_{t+1}),   G_t = L_{t+1,t},   x_T = 0,
//
// eps[n, b, t, :] = z[i = n, k = b T + t, :] of the normal stream with tag s (include/mfgm.h, mfgm_philox.h).  The backward recursion
// is affine in x_{t+1} and is parallelised exactly over the level-0 segments of the packed layout (mfgm_layout.h), as the VDP Lagrange
// sweep and mfgm_bidiag.h do:
//
//   map     one lane per (chain, segment) walks its segment from the last node down and composes x_{pR} = Phi_p x_{(p+1)R} + c_p^n.
//           Phi_p is the same for every sample (sample group 0 writes it); the offsets of K samples ride in the lane's registers and
//           blockIdx.y spreads the sample groups.
//   scan    one wavefront per (chain, sample): lane j composes the maps of ceil(P / 64) consecutive segments, the 64 composed maps are
//           chained from the top through shuffles, and each lane replays its segments, writing xin_p = x_{(p+1)R} of every segment.
//   replay  the map's lanes walk their segments again from xin_p, regenerate eps from the counter (nothing stores the noise) and
//           write x in the natural [S, B, T, d] layout.
//
// Scratch (the caller's, never the plan's workspace): Phi [D*D][Lpad], c [S][D][Lpad], xin [S][D][Lpad] -- element-major, so the
// map and replay lanes of a wavefront touch 512 contiguous bytes per element.
#pragma once
#include "mfgm_layout.h"
#include "mfgm_math.h"
#include "mfgm_philox.h"

namespace mfgm {

// samples carried per lane: the largest K for which neither the map (Phi, K offsets, one node of L, G, y) nor the replay kernel of
// that d spills (-Rpass-analysis=kernel-resource-usage)
constexpr int sample_k(int D) { return D <= 2 ? 16 : (D <= 6 ? 8 : 4); }

template <int D>
MFGM_DEV void smp_noise(unsigned long long seed, unsigned tag, unsigned n, unsigned k, double (&z)[D + (D & 1)]) {
#pragma unroll
    for (int j = 0; j < (D + 1) / 2; ++j) sim_normal_pair(seed, tag, n, k, (unsigned)j, z[2 * j], z[2 * j + 1]);
}

// one node of the factor: L_tt (packed lower triangle), 1 / diag L_tt, G_t = L_{t+1,t} (zero at the last node of a chain), y_t
template <int D>
struct SmpNode {
    double L[D * (D + 1) / 2], inv[D], G[D * D], y[D];
};

template <int D>
MFGM_DEV void smp_load(const double* __restrict__ Lg, const double* __restrict__ Gg, const double* __restrict__ yg, int R, int s,
                       int tile, int l, bool coupled, SmpNode<D>& nd) {
    constexpr int ET = D * (D + 1) / 2, EF = D * D;
    const double* pL = Lg + ((size_t)tile * R + s) * (size_t)(ET * 64) + l;
    const double* pG = Gg + ((size_t)tile * R + s) * (size_t)(EF * 64) + l;
    const double* py = yg + ((size_t)tile * R + s) * (size_t)(D * 64) + l;
#pragma unroll
    for (int e = 0; e < ET; ++e) nd.L[e] = pL[e * 64];
#pragma unroll
    for (int e = 0; e < EF; ++e) nd.G[e] = coupled ? pG[e * 64] : 0.0;
#pragma unroll
    for (int e = 0; e < D; ++e) nd.y[e] = py[e * 64];
#pragma unroll
    for (int i = 0; i < D; ++i) nd.inv[i] = rcp_nr(nd.L[tix(i, i)]);
}

// v <- L_tt^{-T} (w - G_t^T v):  w[i] - sum_j G[j, i] v[j], then back substitution with the transposed lower triangle
template <int D>
MFGM_DEV void smp_step(const SmpNode<D>& nd, const double (&w)[D], double (&v)[D]) {
    double z[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double acc = w[i];
#pragma unroll
        for (int j = 0; j < D; ++j) acc = __builtin_fma(-nd.G[j * D + i], v[j], acc);
        z[i] = acc;
    }
#pragma unroll
    for (int i = D - 1; i >= 0; --i) {
        double acc = z[i];
#pragma unroll
        for (int j = i + 1; j < D; ++j) acc = __builtin_fma(-nd.L[tix(j, i)], z[j], acc);
        z[i] = acc * nd.inv[i];
    }
#pragma unroll
    for (int i = 0; i < D; ++i) v[i] = z[i];
}

struct SmpArgs {
    LevelDesc lv;
    int B, T, S;
    unsigned long long seed;
    unsigned tag;
    const double *L, *G, *y;
    double *Phi, *c, *xin, *x;
    size_t xpk;          // replay with PK: doubles per sample of the packed VEC output (x then holds S packed arrays, unpacked afterwards)
};

// MAP = true: segment maps (Phi from sample group 0, c for the group's samples);  MAP = false: replay from xin, writing x (PK: in the
// packed VEC layout, one array per sample)
template <int D, int K, bool MAP, bool PK = false>
__global__ __launch_bounds__(64) void k_sample_seg(SmpArgs a) {
    const int lane = blockIdx.x * 64 + threadIdx.x;
    if (lane >= a.lv.L) return;
    const int P = a.lv.P, R = a.lv.R, Lpad = a.lv.Lpad, T = a.T;
    const int b = lane / P, p = lane - b * P, tile = blockIdx.x, l = threadIdx.x;
    const int n0 = blockIdx.y * K, ns = min(K, a.S - n0);
    const bool want_phi = MAP && blockIdx.y == 0;
    double v[K][D];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int i = 0; i < D; ++i) v[k][i] = (!MAP && k < ns) ? a.xin[((size_t)(n0 + k) * D + i) * Lpad + lane] : 0.0;
    double phi[MAP ? D : 1][MAP ? D : 1];             // column m of Phi in phi[m]
    if constexpr (MAP) {
#pragma unroll
        for (int m = 0; m < D; ++m)
#pragma unroll
            for (int i = 0; i < D; ++i) phi[m][i] = (i == m) ? 1.0 : 0.0;
    }
    const int s_hi = min(R, T - p * R) - 1;
    for (int s = s_hi; s >= 0; --s) {
        const int t = p * R + s;
        SmpNode<D> nd;
        smp_load<D>(a.L, a.G, a.y, R, s, tile, l, t + 1 < T, nd);
        const unsigned kk = (unsigned)((size_t)b * T + t);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (k < ns) {
                double z[D + (D & 1)], w[D];
                smp_noise<D>(a.seed, a.tag, (unsigned)(n0 + k), kk, z);
#pragma unroll
                for (int i = 0; i < D; ++i) w[i] = nd.y[i] + z[i];
                smp_step<D>(nd, w, v[k]);
                if constexpr (!MAP && PK) {
                    double* o = a.x + (size_t)(n0 + k) * a.xpk + ((size_t)tile * R + s) * (size_t)(D * 64) + l;
#pragma unroll
                    for (int i = 0; i < D; ++i) o[i * 64] = v[k][i];
                } else if constexpr (!MAP) {
                    double* o = a.x + (((size_t)(n0 + k) * a.B + b) * T + t) * D;
#pragma unroll
                    for (int i = 0; i < D; ++i) o[i] = v[k][i];
                }
            }
        }
        if constexpr (MAP) {
            if (want_phi) {
                const double zero[D] = {};
#pragma unroll
                for (int m = 0; m < D; ++m) smp_step<D>(nd, zero, phi[m]);
            }
        }
    }
    if constexpr (MAP) {
        if (want_phi) {
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int m = 0; m < D; ++m) a.Phi[(size_t)(i * D + m) * Lpad + lane] = phi[m][i];
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (k < ns)
#pragma unroll
                for (int i = 0; i < D; ++i) a.c[((size_t)(n0 + k) * D + i) * Lpad + lane] = v[k][i];
    }
}

// xin of every segment of chain blockIdx.x, sample blockIdx.y:  xin_{P-1} = 0,  xin_{p-1} = Phi_p xin_p + c_p
template <int D>
__global__ __launch_bounds__(64) void k_sample_scan(SmpArgs a) {
    const int b = blockIdx.x, n = blockIdx.y, j = threadIdx.x;
    const int P = a.lv.P, Lpad = a.lv.Lpad;
    const int m = (P + 63) / 64, p_lo = min(P, j * m), p_hi = min(P, p_lo + m);
    const double* cn = a.c + (size_t)n * D * Lpad;
    double* xn = a.xin + (size_t)n * D * Lpad;
    // x_{p_lo R} = A x_{p_hi R} + u
    double A[D][D], u[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        u[i] = 0.0;
#pragma unroll
        for (int q = 0; q < D; ++q) A[i][q] = (i == q) ? 1.0 : 0.0;
    }
    for (int p = p_hi - 1; p >= p_lo; --p) {
        const int lane = b * P + p;
        double F[D][D], A2[D][D], u2[D];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int q = 0; q < D; ++q) F[i][q] = a.Phi[(size_t)(i * D + q) * Lpad + lane];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double acc = cn[(size_t)i * Lpad + lane];
#pragma unroll
            for (int q = 0; q < D; ++q) acc = __builtin_fma(F[i][q], u[q], acc);
            u2[i] = acc;
#pragma unroll
            for (int r = 0; r < D; ++r) {
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < D; ++q) s = __builtin_fma(F[i][q], A[q][r], s);
                A2[i][r] = s;
            }
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            u[i] = u2[i];
#pragma unroll
            for (int r = 0; r < D; ++r) A[i][r] = A2[i][r];
        }
    }
    // chain the 64 composed maps from the top: lane q's block is entered with the value that leaves the blocks above it
    double v[D], mine[D];
#pragma unroll
    for (int i = 0; i < D; ++i) v[i] = mine[i] = 0.0;
    for (int q = 63; q >= 0; --q) {
        if (j == q) {
#pragma unroll
            for (int i = 0; i < D; ++i) mine[i] = v[i];
        }
        double w[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double acc = u[i];
#pragma unroll
            for (int r = 0; r < D; ++r) acc = __builtin_fma(A[i][r], v[r], acc);
            w[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) v[i] = __shfl(w[i], q, 64);
    }
    for (int p = p_hi - 1; p >= p_lo; --p) {
        const int lane = b * P + p;
        double w[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            xn[(size_t)i * Lpad + lane] = mine[i];
            double acc = cn[(size_t)i * Lpad + lane];
#pragma unroll
            for (int q = 0; q < D; ++q) acc = __builtin_fma(a.Phi[(size_t)(i * D + q) * Lpad + lane], mine[q], acc);
            w[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) mine[i] = w[i];
    }
}

}  // namespace mfgm
