// os2r_lqr_inst.hip — the os2r_lqr_gains kernels (os2r_lqr.hpp) of one dtype, chains of 2..5 dofs; compiled once per OS2R_REAL.
// They need no robot constants: compiled-in, run-time and registered robots share them.
#include "os2r_lqr.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

template <int NQ>
static void launch_lqr(const LqrArgs<T>& p, hipStream_t s) {
  const dim3 grid((unsigned)((p.M + kLqrEnvs - 1) / kLqrEnvs)), block(kLqrEnvs * (2 * NQ + 2));
  hipLaunchKernelGGL((lqr_gains_kernel<T, NQ>), grid, block, 0, s, p);
}

template <>
int launch_lqr_gains<T>(int nq, const LqrArgs<T>& p, hipStream_t s) {
  switch (nq) {
    case 2: launch_lqr<2>(p, s); return 0;
    case 3: launch_lqr<3>(p, s); return 0;
    case 4: launch_lqr<4>(p, s); return 0;
    case 5: launch_lqr<5>(p, s); return 0;
    default: return 1;
  }
}

}  // namespace os2r
