// The counter-based normal stream of include/mfgm.h: Philox4x32-10 and Box-Muller.  Shared by the Euler-Maruyama kernels (mfgm_sim.h)
// and the posterior sampler (mfgm_sample.h), which read the same stream with different tags.
#pragma once
#include <hip/hip_runtime.h>

#include "mfgm_math.h"

namespace mfgm {

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) ---------------------------------------------------------------------------
MFGM_DEV uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const unsigned hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += W0;
        k1 += W1;
    }
    return c;
}

// ((hi << 21) | (lo >> 11)) is a 53-bit integer (exact in fp64); + 0.5 and * 2^-53 in fp64: a uniform in (0, 1]
MFGM_DEV double sim_u53(unsigned lo, unsigned hi) {
#pragma clang fp contract(off)
    const unsigned long long n = ((unsigned long long)hi << 21) | (unsigned long long)(lo >> 11);
    return ((double)n + 0.5) * 0x1p-53;
}

// normals 2j and 2j + 1 of step k of path i in stream s (Box-Muller on the pair (u1, u2) of counter (j, k, i, s))
MFGM_DEV void sim_normal_pair(unsigned long long seed, unsigned s, unsigned i, unsigned k, unsigned j, double& z0, double& z1) {
#pragma clang fp contract(off)
    const uint4 w = philox4x32_10(make_uint4(j, k, i, s), (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32));
    const double u1 = sim_u53(w.x, w.y), u2 = sim_u53(w.z, w.w);
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);           // sin / cos of 2 pi u2; 2 u2 is exact and the pi-scaled form needs no argument reduction
    z0 = r * cs;
    z1 = r * sn;
}

}  // namespace mfgm
