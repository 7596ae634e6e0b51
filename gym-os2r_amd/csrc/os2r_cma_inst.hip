// os2r_cma_inst.hip — the four kernels of os2rk_cma_sample and os2rk_cma_update (os2r_cma.hpp) of one dtype; compiled once per
// OS2R_REAL into libos2r_cma.so.  They need no robot constants and no chain length.
#include "os2r_cma.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

// the factors, a wave per population; then the samples, which read factor and failed as the first launch wrote them
template <>
void launch_cma_sample<T>(const CmaArgs<T>& p, hipStream_t s) {
  const long long lanes = (long long)p.S * p.M;
  const int per_group = kCmaBlock / (p.D + 1);
  hipLaunchKernelGGL((cma_factor_kernel<T>), dim3((unsigned)p.M), dim3(kCmaChunks), 0, s, p);
  hipLaunchKernelGGL((cma_sample_kernel<T>), dim3((unsigned)((lanes + per_group - 1) / per_group)), dim3(kCmaBlock), 0, s, p);
}

// the ranks, count and status; then the sums and the new state, sixteen waves per population
template <>
void launch_cma_update<T>(const CmaArgs<T>& p, hipStream_t s) {
  const long long lanes = (long long)p.S * p.M;
  hipLaunchKernelGGL((cma_rank_kernel<T>), dim3((unsigned)((lanes + kCmaBlock - 1) / kCmaBlock)), dim3(kCmaBlock), 0, s, p);
  hipLaunchKernelGGL((cma_sum_kernel<T>), dim3((unsigned)p.M), dim3(kCmaSumBlock), 0, s, p);
}

}  // namespace os2r
