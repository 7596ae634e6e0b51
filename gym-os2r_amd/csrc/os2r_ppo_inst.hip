// os2r_ppo_inst.hip — the three os2ro_ppo_gradient kernels (os2r_ppo.hpp) of one dtype; compiled once per OS2R_REAL into
// libos2r_ppo.so.  They need no robot constants and no chain length.
#include "os2r_ppo.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

// the sums of every lane, then -- behind them on the same stream -- the sums over the samples of every policy, which read what
// the first launch wrote into lane_grad, lane_lsig, lane_stat and lane_count: a wave per total above 64 samples, a thread per
// total up to 64
template <>
void launch_ppo_gradient<T>(const PpoArgs<T>& p, hipStream_t s) {
  const unsigned entries = (unsigned)(2 * (p.D + 1) + 2 + kPpoStats + kPpoIntegerSums);
  const unsigned lane_groups = (unsigned)((p.N * kPgThreads + kPgBlock - 1) / kPgBlock);
  hipLaunchKernelGGL((ppo_lane_kernel<T>), dim3(lane_groups), dim3(kPgBlock), 0, s, p);
  if (p.S > kPgChunks)
    hipLaunchKernelGGL((ppo_sum_kernel<T>), dim3((unsigned)p.P, entries), dim3(kPgChunks), 0, s, p);
  else
    hipLaunchKernelGGL((ppo_sum_few_kernel<T>), dim3((unsigned)((p.P + kPgBlock - 1) / kPgBlock), entries), dim3(kPgBlock), 0, s, p);
}

}  // namespace os2r
