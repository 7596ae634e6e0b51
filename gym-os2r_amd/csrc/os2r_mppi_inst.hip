// os2r_mppi_inst.hip — the os2rm_mppi_update kernel (os2r_mppi.hpp) of one dtype; compiled once per OS2R_REAL into
// libos2r_mppi.so.  It needs no robot constants and no chain length.
#include "os2r_mppi.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

template <>
void launch_mppi_update<T>(const MppiArgs<T>& p, hipStream_t s) {
  const dim3 grid((unsigned)((p.M + kMppiRobots - 1) / kMppiRobots), (unsigned)p.K), block(kMppiRobots * kMppiChunks);
  hipLaunchKernelGGL((mppi_update_kernel<T>), grid, block, 0, s, p);
}

}  // namespace os2r
