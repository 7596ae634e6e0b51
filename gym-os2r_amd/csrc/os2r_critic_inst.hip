// os2r_critic_inst.hip — the six kernels of os2rv_gae and os2rv_value_fit (os2r_critic.hpp) of one dtype; compiled once per
// OS2R_REAL into libos2r_critic.so.  They need no robot constants and no chain length.
#include "os2r_critic.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

// the values of all K N steps, then -- behind them on the same stream -- the scan of every lane, which reads them
template <>
void launch_gae<T>(const GaeArgs<T>& p, hipStream_t s) {
  const unsigned lane_groups = (unsigned)((p.N + kCrBlock - 1) / kCrBlock);
  hipLaunchKernelGGL((critic_value_kernel<T>), dim3(lane_groups, (unsigned)p.K), dim3(kCrBlock), 0, s, p);
  hipLaunchKernelGGL((critic_scan_kernel<T>), dim3((unsigned)((p.N + kCrScanBlock - 1) / kCrScanBlock)), dim3(kCrScanBlock), 0, s, p);
}

// the moments of every lane, their sums over the samples of every policy (a wave per total above 64 samples, a thread per total
// up to 64), the solve of every policy: each reads what the one before it wrote
template <>
void launch_value_fit<T>(const FitArgs<T>& p, hipStream_t s) {
  const int n = p.D + 1;
  const unsigned entries = (unsigned)(n * (n + 1) / 2 + n + kCrIntegerSums);
  const unsigned lane_groups = (unsigned)((p.N * kCrThreads + kCrBlock - 1) / kCrBlock);
  hipLaunchKernelGGL((critic_moment_kernel<T>), dim3(lane_groups), dim3(kCrBlock), 0, s, p);
  if (p.S > kPgChunks)
    hipLaunchKernelGGL((critic_sum_kernel<T>), dim3((unsigned)p.P, entries), dim3(kPgChunks), 0, s, p);
  else
    hipLaunchKernelGGL((critic_sum_few_kernel<T>), dim3((unsigned)((p.P + kPgBlock - 1) / kPgBlock), entries), dim3(kPgBlock), 0, s, p);
  hipLaunchKernelGGL((critic_solve_kernel<T>), dim3((unsigned)((p.P + kCrSolveBlock - 1) / kCrSolveBlock)), dim3(kCrSolveBlock), 0, s, p);
}

}  // namespace os2r
