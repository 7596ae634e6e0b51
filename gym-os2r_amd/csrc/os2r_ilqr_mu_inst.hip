// os2r_ilqr_mu_inst.hip — the os2rt_ilqr_backward_mu kernels (os2r_ilqr_mu.hpp) of one dtype, chains of 2..5 dofs; compiled once
// per OS2R_REAL into libos2r_steer.so.  They need no robot constants.
#include "os2r_ilqr_mu.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

template <>
int launch_ilqr_backward_mu<T>(int nq, const IlqrMuArgs<T>& p, hipStream_t s) {
  return by_chain_length(nq, [&](auto chain) {
    constexpr int NQ = decltype(chain)::value;
    const dim3 grid((unsigned)((p.base.M + kLqrEnvs - 1) / kLqrEnvs)), block(kLqrEnvs * (2 * NQ + 2));
    hipLaunchKernelGGL((ilqr_backward_mu_kernel<T, NQ>), grid, block, 0, s, p);
  });
}

}  // namespace os2r
