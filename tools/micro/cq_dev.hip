// Development harness: instantiates the level-0 cq kernels for d = 6 alone, so that `hipcc -S --cuda-device-only` on this file gives
// their ISA / register usage in seconds instead of the minutes the whole sweeps unit takes (tools/isa_regs.py reads the listing).
#include "../../vi-diffusion-processes_amd/csrc/mfgm_internal.h"
#include "../../vi-diffusion-processes_amd/csrc/mfgm_cq.h"
using namespace mfgm;
void inst(SweepArgs a, CqArgs q, SdeParams pr, double* fix) {
    hipLaunchKernelGGL((k_reduce_cq<6>), dim3(1), dim3(64), 0, 0, a, q);
    hipLaunchKernelGGL((k_reduce_cq_lean<6>), dim3(1), dim3(64), 0, 0, a, q);
    hipLaunchKernelGGL((k_forward_cq<6>), dim3(1), dim3(64), 0, 0, a, q);
    hipLaunchKernelGGL((k_forward_cq<6, 2>), dim3(1), dim3(64), 0, 0, a, q);
    hipLaunchKernelGGL((k_backward_kl_cq<6, 2>), dim3(1), dim3(64), 0, 0, a, pr, q);
    hipLaunchKernelGGL((k_forward_reduce_cq<6>), dim3(1), dim3(128), 0, 0, a, q);
    hipLaunchKernelGGL((k_backward_girsanov_cq<6>), dim3(1), dim3(64), 0, 0, a, pr, q, fix);
    hipLaunchKernelGGL((k_backward_kl_cq<6>), dim3(1), dim3(64), 0, 0, a, pr, q);
}
// k_forward_pair_cq at every size and cache policy the library dispatches it for
template <int D>
void inst_pair(SweepArgs a, CqArgs q) {
    hipLaunchKernelGGL((k_forward_pair_cq<D>), dim3(1), dim3(128), 0, 0, a, q, a, q);
    hipLaunchKernelGGL((k_forward_pair_cq<D, 1>), dim3(1), dim3(128), 0, 0, a, q, a, q);
}
// the reduce of mfgm_cq_factor_pair_heads: the shared part and the tail, at the headline size and the largest one
template <int D>
void inst_heads(SweepArgs a, CqArgs q, double* park) {
    hipLaunchKernelGGL((k_reduce_cq_interior<D>), dim3(1), dim3(64), 0, 0, a, q, park, 2);
    hipLaunchKernelGGL((k_reduce_cq_heads<D>), dim3(1, 2), dim3(64), 0, 0, a, q, a, q, park, 2);
}
void inst_heads_all(SweepArgs a, CqArgs q, double* park) { inst_heads<6>(a, q, park); inst_heads<8>(a, q, park); }
void inst_pairs(SweepArgs a, CqArgs q) {
    inst_pair<1>(a, q); inst_pair<2>(a, q); inst_pair<3>(a, q); inst_pair<4>(a, q); inst_pair<5>(a, q); inst_pair<6>(a, q);
}
// the thinned pair route (mfgm_cq_factor_pair_thin, mfgm_cq_selinv_kl_thin) at every size and cache policy the library dispatches it for
template <int D>
void inst_thin(SweepArgs a, CqArgs q, SdeParams pr) {
    hipLaunchKernelGGL((k_forward_pair_thin_cq<D>), dim3(1), dim3(128), 0, 0, a, q, a, q);
    hipLaunchKernelGGL((k_forward_pair_thin_cq<D, 1>), dim3(1), dim3(128), 0, 0, a, q, a, q);
    hipLaunchKernelGGL((k_backward_kl_thin_cq<D>), dim3(1), dim3(64), 0, 0, a, pr, q);
    hipLaunchKernelGGL((k_backward_kl_thin_cq<D, 2>), dim3(1), dim3(64), 0, 0, a, pr, q);
}
void inst_thin_all(SweepArgs a, CqArgs q, SdeParams pr) {
    inst_thin<1>(a, q, pr); inst_thin<2>(a, q, pr); inst_thin<3>(a, q, pr); inst_thin<4>(a, q, pr); inst_thin<5>(a, q, pr); inst_thin<6>(a, q, pr);
}
