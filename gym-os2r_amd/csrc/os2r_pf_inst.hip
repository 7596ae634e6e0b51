// os2r_pf_inst.hip — the os2rp_pf_update kernel (os2r_pf.hpp) of one dtype; compiled once per OS2R_REAL into libos2r_pf.so.
// It needs no robot constants and no chain length.
#include "os2r_pf.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

template <>
void launch_pf_update<T>(const PfArgs<T>& p, hipStream_t s) {
  const dim3 grid((unsigned)((p.M + kPfRobots - 1) / kPfRobots)), block(kPfRobots * kPfChunks);
  hipLaunchKernelGGL((pf_update_kernel<T>), grid, block, 0, s, p);
}

}  // namespace os2r
