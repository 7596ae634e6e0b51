// os2r_lin_inst.hip — one instantiation unit of the os2r_linearize kernels; compiled once per
// (OS2R_REAL, OS2R_UNIT) like os2r_inst.hip, whose objects it leaves as they are.
//
//   OS2R_UNIT = 0..3   static model of os2r_models_gen.hpp
//   OS2R_UNIT = 12..15 run-time model with 2..5 dofs
//
// A handle's Jacobians come from the substep instantiation its os2r_step runs (launch_step of os2r_inst.hip picks by the same
// rules): contact {on, off} x per-env parameters {on, off} x, for the compiled-in robots, the default sweep counts as
// compile-time bounds, and in fp64 the solver (exact finish / sweeps only).  Observation layouts and the counting variants
// do not enter: there is no epilogue.
#include "os2r_kernels.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif
#ifndef OS2R_UNIT
#error "OS2R_UNIT must be 0..3 (static model id) or 12..15 (run-time model, nq = unit - 10)"
#endif

namespace os2r {

using T = OS2R_REAL;

#define OS2R_LAUNCH_LIN(STD, SOLVER) \
  hipLaunchKernelGGL((linearize_kernel<T, MD, CONTACT, DR, STD, SOLVER>), grid, block, 0, s, p)

template <typename MD, bool CONTACT, bool DR>
static int launch_linearize(const LinArgs<T>& p, hipStream_t s) {
  const StepArgs<T>& a = p.s;
  const dim3 grid((unsigned)((a.N + kWave - 1) / kWave), (unsigned)p.ncols), block(kWave);
  if (MD::kStatic && is_std_solver<T>(a.pgs_iters, a.pgs_normal_iters, a.pgs_exact, MD::NQ)) {
    if constexpr (MD::kStatic) { OS2R_LAUNCH_LIN(true, std_solver(true, sizeof(T) == 8, StdSolver<T>::kExact)); }
  } else if constexpr (sizeof(T) == 8) {
    if (a.pgs_exact > 0) OS2R_LAUNCH_LIN(false, kSolverExact);
    else OS2R_LAUNCH_LIN(false, kSolverSweeps);
  } else {
    OS2R_LAUNCH_LIN(false, kSolverSweeps);
  }
  return 0;
}

template <typename R, int UNIT>
int linearize_unit(bool contact, bool dr, const LinArgs<R>& p, hipStream_t s);

#if OS2R_UNIT < 10
using MD = StModel<T, OS2R_UNIT>;
#else
using MD = RtModel<T, OS2R_UNIT - 10>;
#endif

template <>
int linearize_unit<T, OS2R_UNIT>(bool contact, bool dr, const LinArgs<T>& p, hipStream_t s) {
  if constexpr (MD::CMASK != 0u) {   // (a chain that cannot reach the ground has no contact variant)
    if (contact) return dr ? launch_linearize<MD, true, true>(p, s) : launch_linearize<MD, true, false>(p, s);
  }
  return dr ? launch_linearize<MD, false, true>(p, s) : launch_linearize<MD, false, false>(p, s);
}

}  // namespace os2r
