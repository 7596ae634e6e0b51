// os2r_es_inst.hip — the five kernels of os2ra_es_perturb and os2ra_es_update (os2r_es.hpp) of one dtype; compiled once per
// OS2R_REAL into libos2r_es.so.  They need no robot constants and no chain length.
#include "os2r_es.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

template <>
void launch_es_perturb<T>(const EsArgs<T>& p, hipStream_t s) {
  const long long threads = (long long)p.S * p.M * (p.D + 1);
  hipLaunchKernelGGL((es_perturb_kernel<T>), dim3((unsigned)((threads + kEsBlock - 1) / kEsBlock)), dim3(kEsBlock), 0, s, p);
}

// where top selects, the keys and the ranks (above 1 024 directions in spans, and a launch that decides); then the sums (sixteen
// waves per (population, Philox block) from 1 024 directions on, a wave above 64, a thread up to 64): each reads what the one
// before it wrote
template <>
void launch_es_update<T>(const EsArgs<T>& p, hipStream_t s) {
  const unsigned blocks = (unsigned)p.D + 1u;
  if (p.select) {
    const unsigned groups = (unsigned)(((long long)p.S * p.M + kEsBlock - 1) / kEsBlock);
    const unsigned spans = (unsigned)((p.S + kEsRankSpan - 1) / kEsRankSpan);
    hipLaunchKernelGGL((es_score_kernel<T>), dim3(groups), dim3(kEsBlock), 0, s, p);
    hipLaunchKernelGGL((es_rank_kernel<T>), dim3(groups, spans < 65535u ? spans : 65535u), dim3(kEsBlock), 0, s, p);
    if (spans > 1) hipLaunchKernelGGL((es_keep_kernel<T>), dim3(groups), dim3(kEsBlock), 0, s, p);
  }
  if (p.S >= kEsWide)
    hipLaunchKernelGGL((es_sum_wide_kernel<T>), dim3((unsigned)p.M, blocks), dim3(kEsWide), 0, s, p);
  else if (p.S > kEsChunks)
    hipLaunchKernelGGL((es_sum_kernel<T>), dim3((unsigned)p.M, blocks), dim3(kEsChunks), 0, s, p);
  else
    hipLaunchKernelGGL((es_sum_few_kernel<T>), dim3((unsigned)((p.M + kEsBlock - 1) / kEsBlock), blocks), dim3(kEsBlock), 0, s, p);
}

}  // namespace os2r
