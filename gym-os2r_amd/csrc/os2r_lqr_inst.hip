// os2r_lqr_inst.hip — the os2r_lqr_gains kernels (os2r_lqr.hpp) of one dtype, chains of 2..5 dofs; compiled once per OS2R_REAL.
// They need no robot constants: compiled-in, run-time and registered robots share them.
#include "os2r_lqr.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

template <>
int launch_lqr_gains<T>(int nq, const LqrArgs<T>& p, hipStream_t s) {
  return by_chain_length(nq, [&](auto chain) {
    constexpr int NQ = decltype(chain)::value;
    const dim3 grid((unsigned)((p.M + kLqrEnvs - 1) / kLqrEnvs)), block(kLqrEnvs * (2 * NQ + 2));
    hipLaunchKernelGGL((lqr_gains_kernel<T, NQ>), grid, block, 0, s, p);
  });
}

}  // namespace os2r
