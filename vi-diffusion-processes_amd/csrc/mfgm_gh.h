// Gauss-Hermite rules of numpy.polynomial.hermite.hermgauss(H), H = 10 and 20, as node / weight tables.  Shared by the tensor-product
// quadrature of the SDE kernels (mfgm_quad.h) and the per-observation quadrature of the scalar likelihoods (mfgm_lik.h).
#pragma once
#include <hip/hip_runtime.h>

#include "mfgm_math.h"

namespace mfgm {

__device__ __constant__ const double kGH10x[5] = {0.3429013272237046, 1.0366108297895136, 1.7566836492998816, 2.5327316742327897,
                                                  3.4361591188377374};
__device__ __constant__ const double kGH10w[5] = {0.34464233493201907, 0.13548370298026777, 0.01911158050077031, 0.0007580709343122176,
                                                  4.310652630718299e-06};
__device__ __constant__ const double kGH20x[10] = {0.24534070830090124, 0.7374737285453944, 1.234076215395323, 1.7385377121165861,
                                                   2.2549740020892757, 2.7888060584281305, 3.3478545673832163, 3.944764040115625,
                                                   4.603682449550744, 5.387480890011233};
__device__ __constant__ const double kGH20w[10] = {0.2607930634495549, 0.16173933398399998, 0.0615063720639769, 0.013997837447101022,
                                                   0.00183010313108049, 0.00012882627996192928, 4.402121090230851e-06,
                                                   6.127490259982928e-08, 2.4820623623151755e-10, 1.2578006724379234e-13};
// node k (0 .. H-1, ascending) and weight (w / sqrt(pi)) of numpy.polynomial.hermite.hermgauss(H); the rule is symmetric
MFGM_DEV void gh_node(int H, int k, double& xi, double& w) {
    const int half = H / 2, kk = (k < half) ? (half - 1 - k) : (k - half);
    const double xa = (H == 10) ? kGH10x[kk] : kGH20x[kk];
    w = (H == 10) ? kGH10w[kk] : kGH20w[kk];
    xi = (k < half) ? -xa : xa;
}

}  // namespace mfgm
