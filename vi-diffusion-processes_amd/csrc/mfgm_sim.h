// Simulation of the SDE priors (markovflow/sde/sde_utils.py:36-96): the counter-based normal stream of include/mfgm.h (Philox4x32-10 +
// Box-Muller) and the Euler-Maruyama recursion, one lane per path with the state in registers.
//
// Arithmetic is written with FMA contraction off: the torch route of sde_utils.euler_maruyama evaluates the same recursion one rounded
// torch op at a time, and with the same rounding sequence the two routes agree to the last bit for the drifts whose torch form has the
// same operation order (OU, the theta drifts, Van der Pol), and to a few ulps per step for the others.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mfgm.h"
#include "mfgm_math.h"
#include "mfgm_philox.h"

namespace mfgm {

constexpr int kSimD = 8;          // largest state dimension
constexpr int kSimLanes = 64;     // one wave per block, one lane per path
constexpr int kSimStageW = 64;    // largest staged row chunk (doubles per path per flush)

struct sim_chol {                 // lower Cholesky factor of q, packed lower triangle (row r at r (r + 1) / 2)
    double L[kSimD * (kSimD + 1) / 2];
};

// the d normals of step k of path i (stream 0)
template <int D>
MFGM_DEV void sim_step_noise(unsigned long long seed, unsigned i, unsigned k, double (&z)[D + (D & 1)]) {
#pragma unroll
    for (int j = 0; j < (D + 1) / 2; ++j) sim_normal_pair(seed, 0u, i, k, (unsigned)j, z[2 * j], z[2 * j + 1]);
}

// ---- drift-only evaluators (the torch forms of vi-diffusion-processes_amd/sde.py, operation for operation) --------------------------
//   10 Van der Pol, d = 2:        f = tau (a ((x1 - x1^3 / 3) - x2), x1 / a)        theta = (a, tau)
//   11 ReLU network per dimension: f = sum_k relu(W1_k x + b1_k) W2_k + b2          theta = (W1 [nh], b1 [nh], W2 [nh], b2)
//   12 cubic per dimension:        f = x (c1 - c3 x^2)                               theta = (c1, c3) = drift_cubic()
//   13 / 14 / 15 per dimension:    theta tanh x / sin(x - theta) / sqrt(theta |x|)   theta = (theta, -)
template <int D, int KIND>
MFGM_DEV void sim_drift(const mfgm_quad_drift& q, const double (&x)[D], double (&f)[D]) {
#pragma clang fp contract(off)
    if constexpr (KIND == 10) {
        const double a = q.theta[0], tau = q.theta[1], x1 = x[0], x2 = x[1];
        f[0] = tau * (a * ((x1 - x1 * x1 * x1 / 3.0) - x2));
        f[1] = tau * (x1 / a);
    } else if constexpr (KIND == 11) {
        const int nh = q.nh;
        const double *W1 = q.theta, *b1 = q.theta + nh, *W2 = q.theta + 2 * nh, b2 = q.theta[3 * nh];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double acc = 0.0;
            for (int k = 0; k < nh; ++k) {
                const double z = x[i] * W1[k] + b1[k];
                acc = acc + (z > 0.0 ? z : 0.0) * W2[k];
            }
            f[i] = acc + b2;
        }
    } else {
        const double c1 = q.theta[0], c3 = q.theta[1];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double xi = x[i];
            if constexpr (KIND == 12) f[i] = xi * (c1 - c3 * (xi * xi));
            else if constexpr (KIND == 13) f[i] = c1 * tanh(xi);
            else if constexpr (KIND == 14) f[i] = sin(xi - c1);
            else f[i] = sqrt(c1 * fabs(xi));
        }
    }
}

// ---- Euler-Maruyama: one lane per path -------------------------------------------------------------------------------------------
// Output rows are written in the reference's [B, N, d] layout.  With S > 0 every lane stages S consecutive rows (S d doubles, contiguous
// in global memory) in LDS, and a flush writes the wave's 64 chunks back cooperatively: consecutive lanes store consecutive doubles of
// one path's chunk, so a store instruction touches a few cache lines instead of the 64 a per-lane row store touches.  S = 0 stores every
// row straight from the lane (the A/B baseline).  The noise of step k + 1 (Philox blocks and Box-Muller) does not depend on x and is
// computed at the top of step k, where the scheduler can issue it under the drift chain of step k.
MFGM_DEV void sim_flush(const double* stage, int R, int w, int path0, int B, size_t row, size_t col0, double* __restrict__ X) {
    __syncthreads();
    for (int f = threadIdx.x; f < kSimLanes * w; f += kSimLanes) {
        const int p = f / w, l = f - p * w;
        if (path0 + p < B) X[(size_t)(path0 + p) * row + col0 + l] = stage[p * R + l];
    }
    __syncthreads();
}

template <int D, int KIND>
__global__ __launch_bounds__(kSimLanes) void k_euler_maruyama(mfgm_quad_drift q, sim_chol lc, int B, int N, const double* __restrict__ x0,
                                                              const double* __restrict__ tg, unsigned long long seed, int S,
                                                              double* __restrict__ X) {
#pragma clang fp contract(off)
    extern __shared__ double stage[];            // [64][R], R = S D rounded up to odd (conflict-free row writes)
    const int lane = threadIdx.x, path0 = blockIdx.x * kSimLanes, i = path0 + lane;
    const bool live = i < B;
    const size_t row = (size_t)N * D;
    const int W = S * D, R = W | 1;
    double* mine = stage + lane * R;
    double x[D];
#pragma unroll
    for (int e = 0; e < D; ++e) x[e] = live ? x0[(size_t)i * D + e] : 0.0;

    int n0 = 0;                                  // first row of the chunk being staged
    auto put = [&](int n) {
        if (S == 0) {
            if (live) {
#pragma unroll
                for (int e = 0; e < D; ++e) X[(size_t)i * row + (size_t)n * D + e] = x[e];
            }
            return;
        }
        const int slot = n - n0;
#pragma unroll
        for (int e = 0; e < D; ++e) mine[slot * D + e] = x[e];
        if (slot == S - 1 || n == N - 1) {
            sim_flush(stage, R, (slot + 1) * D, path0, B, row, (size_t)n0 * D, X);
            n0 += S;
        }
    };
    put(0);

    double zc[D + (D & 1)], zn[D + (D & 1)];
    if (N > 1) sim_step_noise<D>(seed, (unsigned)i, 0u, zc);
    double tprev = 0.0;
    for (int k = 0; k < N - 1; ++k) {
        sim_step_noise<D>(seed, (unsigned)i, (unsigned)(k + 1), zn);     // next step's noise (unused after the last step)
        const double t = tg[k], dt = t - tprev, sq = sqrt(dt);
        tprev = t;
        double f[D];
        sim_drift<D, KIND>(q, x, f);
#pragma unroll
        for (int r = 0; r < D; ++r) {
            const double* Lr = lc.L + r * (r + 1) / 2;
            double acc = zc[0] * Lr[0];
#pragma unroll
            for (int j = 1; j <= r; ++j) acc = acc + zc[j] * Lr[j];
            x[r] = (x[r] + f[r] * dt) + sq * acc;
        }
        put(k + 1);
#pragma unroll
        for (int e = 0; e < D + (D & 1); ++e) zc[e] = zn[e];
    }
}

// out [P, K, d]: one thread per (path, step, pair)
static __global__ void k_normal_fill(unsigned long long seed, unsigned s, int P, int K, int d, double* __restrict__ out) {
    const int np = (d + 1) / 2;
    const size_t total = (size_t)P * K * np;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(t % np);
        const size_t r = t / np;
        const int k = (int)(r % K), i = (int)(r / K);
        double z0, z1;
        sim_normal_pair(seed, s, (unsigned)i, (unsigned)k, (unsigned)j, z0, z1);
        double* o = out + ((size_t)i * K + k) * d + 2 * j;
        o[0] = z0;
        if (2 * j + 1 < d) o[1] = z1;
    }
}

}  // namespace mfgm
