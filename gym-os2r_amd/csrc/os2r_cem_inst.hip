// os2r_cem_inst.hip — the two os2rx_cem_update kernels (os2r_cem.hpp) of one dtype; compiled once per OS2R_REAL into
// libos2r_cem.so.  They need no robot constants and no chain length.
#include "os2r_cem.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

// the update of every knot, then -- behind it on the same stream -- the pooling that reads what it wrote into var_out
template <>
void launch_cem_update<T>(const CemArgs<T>& p, hipStream_t s) {
  const unsigned groups = (unsigned)((p.M + kCemRobots - 1) / kCemRobots);
  const dim3 block(kCemRobots * kCemChunks);
  hipLaunchKernelGGL((cem_update_kernel<T>), dim3(groups, (unsigned)p.K), block, 0, s, p);
  hipLaunchKernelGGL((cem_pool_kernel<T>), dim3(groups), block, 0, s, p);
}

}  // namespace os2r
