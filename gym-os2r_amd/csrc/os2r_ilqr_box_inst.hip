// os2r_ilqr_box_inst.hip — the os2rb_ilqr_backward_box kernels (os2r_ilqr_box.hpp) of one dtype, chains of 2..5 dofs; compiled once
// per OS2R_REAL into libos2r_box.so.  They need no robot constants.
#include "os2r_ilqr_box.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

template <>
int launch_ilqr_backward_box<T>(int nq, const IlqrBoxArgs<T>& p, hipStream_t s) {
  return by_chain_length(nq, [&](auto chain) {
    constexpr int NQ = decltype(chain)::value;
    const dim3 grid((unsigned)((p.base.M + kLqrEnvs - 1) / kLqrEnvs)), block(kLqrEnvs * (2 * NQ + 2));
    hipLaunchKernelGGL((ilqr_backward_box_kernel<T, NQ>), grid, block, 0, s, p);
  });
}

}  // namespace os2r
