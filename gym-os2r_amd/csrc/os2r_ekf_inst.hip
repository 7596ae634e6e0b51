// os2r_ekf_inst.hip — the os2re_ekf_update kernels (os2r_ekf.hpp) of one dtype, chains of 2..5 dofs; compiled once per OS2R_REAL
// into libos2r_ekf.so.  They need no robot constants.
#include "os2r_ekf.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

template <>
int launch_ekf_update<T>(int nq, const EkfArgs<T>& p, hipStream_t s) {
  return by_chain_length(nq, [&](auto chain) {
    constexpr int NQ = decltype(chain)::value;
    const dim3 grid((unsigned)((p.M + kEkfRobots - 1) / kEkfRobots)), block(kEkfRobots * 2 * NQ);
    hipLaunchKernelGGL((ekf_update_kernel<T, NQ>), grid, block, 0, s, p);
  });
}

}  // namespace os2r
