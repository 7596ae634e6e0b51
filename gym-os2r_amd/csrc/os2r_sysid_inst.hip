// os2r_sysid_inst.hip — the five kernels of os2ri_perturb and os2ri_update (os2r_sysid.hpp) of one dtype; compiled once per
// OS2R_REAL into libos2r_sysid.so.  They need no robot constants and no chain length.
#include "os2r_sysid.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

// a thread per row and lane of the packed parameters
template <>
void launch_sysid_perturb<T>(const SysidArgs<T>& p, hipStream_t s) {
  const long long entries = (long long)p.F * (2 * p.P + 1) * p.M;
  hipLaunchKernelGGL((sysid_perturb_kernel<T>), dim3((unsigned)((entries + kSysidBlock - 1) / kSysidBlock)), dim3(kSysidBlock), 0, s, p);
}

// the sums of every segment; then the totals of every set, which read sums and counts as the first launch wrote them; then the
// verdict and the step of every set, which reads the totals
template <>
void launch_sysid_update<T>(const SysidArgs<T>& p, hipStream_t s) {
  const int pairs = (p.P + 1) / 2, rows = p.P * (p.P + 1) / 2 + p.P + 2;
  hipLaunchKernelGGL((sysid_segment_kernel<T>), dim3((unsigned)((p.M + kSysidLanes - 1) / kSysidLanes)), dim3(pairs * kSysidLanes), 0, s, p);
  if (p.M / p.sets > kPgChunks)
    hipLaunchKernelGGL((sysid_sum_kernel<T>), dim3((unsigned)p.sets, rows), dim3(kPgChunks), 0, s, p);
  else
    hipLaunchKernelGGL((sysid_sum_few_kernel<T>), dim3((unsigned)((p.sets + kSysidBlock - 1) / kSysidBlock), rows), dim3(kSysidBlock), 0, s, p);
  hipLaunchKernelGGL((sysid_step_kernel<T>), dim3((unsigned)p.sets), dim3(kSysidLanes), 0, s, p);
}

}  // namespace os2r
