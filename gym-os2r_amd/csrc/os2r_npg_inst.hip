// os2r_npg_inst.hip — the four os2rn_natural_step kernels (os2r_npg.hpp) of one dtype; compiled once per OS2R_REAL into
// libos2r_npg.so.  They need no robot constants and no chain length.
#include "os2r_npg.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

// the Fisher moments of every lane, their sums over the samples of every policy (a wave per total above 64 samples, a thread per
// total up to 64), the solve and the scaling of every policy: each reads what the one before it wrote
template <>
void launch_natural_step<T>(const NpgArgs<T>& p, hipStream_t s) {
  const int n = p.D + 1;
  const unsigned entries = (unsigned)(n * (n + 1) + kNpgIntegerSums);
  const unsigned lane_groups = (unsigned)((p.N * kCrThreads + kCrBlock - 1) / kCrBlock);
  hipLaunchKernelGGL((npg_moment_kernel<T>), dim3(lane_groups), dim3(kCrBlock), 0, s, p);
  if (p.S > kPgChunks)
    hipLaunchKernelGGL((npg_sum_kernel<T>), dim3((unsigned)p.P, entries), dim3(kPgChunks), 0, s, p);
  else
    hipLaunchKernelGGL((npg_sum_few_kernel<T>), dim3((unsigned)((p.P + kPgBlock - 1) / kPgBlock), entries), dim3(kPgBlock), 0, s, p);
  hipLaunchKernelGGL((npg_solve_kernel<T>), dim3((unsigned)((p.P + kNpgSolvePolicies - 1) / kNpgSolvePolicies)), dim3(kNpgSolveBlock), 0, s, p);
}

}  // namespace os2r
