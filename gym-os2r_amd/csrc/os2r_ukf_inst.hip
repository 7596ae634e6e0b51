// os2r_ukf_inst.hip — the os2ru_ukf_points and os2ru_ukf_update kernels (os2r_ukf.hpp) of one dtype, chains of 2..5 dofs; compiled
// once per OS2R_REAL into libos2r_ukf.so.  They need no robot constants.
#include "os2r_ukf.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

template <>
int launch_ukf_points<T>(int nq, const UkfPointsArgs<T>& p, hipStream_t s) {
  return by_chain_length(nq, [&](auto chain) {
    constexpr int NQ = decltype(chain)::value;
    const dim3 grid((unsigned)((p.M + kUkfRobots - 1) / kUkfRobots)), block(kUkfRobots * 2 * NQ);
    hipLaunchKernelGGL((ukf_points_kernel<T, NQ>), grid, block, 0, s, p);
  });
}

template <>
int launch_ukf_update<T>(int nq, const UkfArgs<T>& p, hipStream_t s) {
  return by_chain_length(nq, [&](auto chain) {
    constexpr int NQ = decltype(chain)::value;
    const dim3 grid((unsigned)((p.M + kUkfRobots - 1) / kUkfRobots)), block(kUkfRobots * 2 * NQ);
    hipLaunchKernelGGL((ukf_update_kernel<T, NQ>), grid, block, 0, s, p);
  });
}

}  // namespace os2r
