// os2r_search_inst.hip — the os2rs_ilqr_line_search kernels (os2r_search.hpp) of one dtype, chains of 2..5 dofs; compiled once
// per OS2R_REAL into libos2r_search.so.  They need no robot constants.
#include "os2r_search.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

template <>
int launch_ilqr_line_search<T>(int nq, const SearchArgs<T>& p, hipStream_t s) {
  return by_chain_length(nq, [&](auto chain) {
    constexpr int NQ = decltype(chain)::value;
    const dim3 grid((unsigned)((p.M + kSearchTraj - 1) / kSearchTraj)), block(kSearchTraj * p.nalpha);
    hipLaunchKernelGGL((ilqr_line_search_kernel<T, NQ>), grid, block, 0, s, p);
  });
}

}  // namespace os2r
