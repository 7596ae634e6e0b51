// os2r_norm_inst.hip — the four kernels of os2rz_obs_stats, os2rz_fold and os2rz_unfold (os2r_norm.hpp) of one dtype; compiled
// once per OS2R_REAL into libos2r_norm.so.  They need no robot constants and no chain length.
#include "os2r_norm.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

// the sums of every (lane, component); then the sums of every (policy, component) and its merge (four waves each above 64 samples, a
// thread each up to 64), which reads what the first wrote
template <>
void launch_obs_stats<T>(const StatsArgs<T>& p, hipStream_t s) {
  const long long per = p.lanes_per_block;
  hipLaunchKernelGGL((norm_lane_kernel<T>), dim3((unsigned)((p.N + per - 1) / per)), dim3(kNormBlock), 0, s, p);
  if (p.S > kPgChunks)
    hipLaunchKernelGGL((norm_sum_kernel<T>), dim3((unsigned)p.P, (unsigned)p.D), dim3(kNormSumWaves * kPgChunks), 0, s, p);
  else
    hipLaunchKernelGGL((norm_sum_few_kernel<T>), dim3((unsigned)((p.P + kNormBlock - 1) / kNormBlock), (unsigned)p.D), dim3(kNormBlock), 0, s, p);
}

template <>
void launch_norm_fold<T>(const FoldArgs<T>& p, hipStream_t s) {
  const long long threads = p.Q * p.rows;
  hipLaunchKernelGGL((norm_fold_kernel<T>), dim3((unsigned)((threads + kNormBlock - 1) / kNormBlock)), dim3(kNormBlock), 0, s, p);
}

}  // namespace os2r
