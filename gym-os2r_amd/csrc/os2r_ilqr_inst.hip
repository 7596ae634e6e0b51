// os2r_ilqr_inst.hip — the os2rc_ilqr_backward kernels (os2r_ilqr.hpp) of one dtype, chains of 2..5 dofs; compiled once per
// OS2R_REAL into libos2r_control.so.  They need no robot constants.
#include "os2r_ilqr.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif

namespace os2r {

using T = OS2R_REAL;

template <int NQ>
static void launch_ilqr(const IlqrArgs<T>& p, hipStream_t s) {
  const dim3 grid((unsigned)((p.M + kLqrEnvs - 1) / kLqrEnvs)), block(kLqrEnvs * (2 * NQ + 2));
  hipLaunchKernelGGL((ilqr_backward_kernel<T, NQ>), grid, block, 0, s, p);
}

template <>
int launch_ilqr_backward<T>(int nq, const IlqrArgs<T>& p, hipStream_t s) {
  switch (nq) {
    case 2: launch_ilqr<2>(p, s); return 0;
    case 3: launch_ilqr<3>(p, s); return 0;
    case 4: launch_ilqr<4>(p, s); return 0;
    case 5: launch_ilqr<5>(p, s); return 0;
    default: return 1;
  }
}

}  // namespace os2r
