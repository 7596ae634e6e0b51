// os2r_jit_fused_unit.hip -- the kernels behind os2r_rollout, os2r_rollout_policy* and os2r_linearize specialised for ONE
// robot, built at run time into code objects of their own beside the step object of os2r_jit_unit.hip.
//
// gym_os2r_amd/jit.py compiles this file once per kind, with the flags and the generated table of the step object plus
//   -DOS2R_JIT_KIND=1   fused rollout:        os2r_jit_rollout_c1_d{0,1}
//   -DOS2R_JIT_KIND=2   fused policy rollout: os2r_jit_policy_c1_d{0,1}, and os2r_jit_policy_rec_c1_d{0,1} with the data symbol
//                       os2r_jit_policy_knots: the variants that record the knots (os2rr_rollout_policy_recorded)
//   -DOS2R_JIT_KIND=3   linearize:            os2r_jit_lin_c{C}_d{0,1} and ..._s, C = OS2R_JIT_CONTACT
// one kind per code object, so that the objects build side by side and the first use of a robot waits for the slowest of
// them, not for their sum.  Every kernel wraps a device template of os2r_kernels.hpp as it is: the arithmetic of a step is
// the code the robot's step kernels run.  The fused kinds exist where the compiled-in robots have them (launch_step of
// os2r_inst.hip): ground contact, the default solver settings; a contact-off build of kind 1 or 2 exports nothing.
#include "os2r_kernels.hpp"

#ifndef OS2R_REAL
#error "OS2R_REAL must be float or double"
#endif
#ifndef OS2R_JIT_TABLES
#error "OS2R_JIT_TABLES must name the generated table header"
#endif
#ifndef OS2R_JIT_CONTACT
#error "OS2R_JIT_CONTACT must be 0 or 1"
#endif
#if !defined(OS2R_JIT_KIND) || OS2R_JIT_KIND < 1 || OS2R_JIT_KIND > 3
#error "OS2R_JIT_KIND must be 1 (rollout), 2 (policy rollout) or 3 (linearize)"
#endif
#include OS2R_JIT_TABLES

namespace os2r {
using JitReal = OS2R_REAL;
using JitModel = StModel<JitReal, 100>;
// the solver of the robot's step kernels: NAME_s (default sweep counts compiled in) and NAME (counts read from the handle)
constexpr int kJitSolverStd = std_solver(true, sizeof(JitReal) == 8, StdSolver<JitReal>::kExact);
constexpr int kJitSolverAny = std_solver(false, sizeof(JitReal) == 8, StdSolver<JitReal>::kExact);
// the observation layout of the task the object was built for, announced in os2r_jit_layout as the step object does;
// without one the layout is read from the arguments
#ifdef OS2R_JIT_LAYOUT_DIM
using JitLayout = StLayout<OS2R_JIT_LAYOUT_KINDS, OS2R_JIT_LAYOUT_SRCS, OS2R_JIT_LAYOUT_DIM>;
#else
using JitLayout = RtLayout;
#endif
}  // namespace os2r

#if OS2R_JIT_KIND != 3 && OS2R_JIT_CONTACT
#ifdef OS2R_JIT_LAYOUT_DIM
extern "C" __device__ __attribute__((used)) const unsigned long long os2r_jit_layout[3] = {
    OS2R_JIT_LAYOUT_KINDS, OS2R_JIT_LAYOUT_SRCS, OS2R_JIT_LAYOUT_DIM};
#endif
#if OS2R_JIT_KIND == 1
#define OS2R_JIT_ROLLOUT_KERNEL(NAME, DR)                                                                              \
  extern "C" __global__ OS2R_STEP_KERNEL_ATTRS(OS2R_REAL) void NAME(const os2r::StepArgs<os2r::JitReal> A) {           \
    os2r::step_body<os2r::JitReal, os2r::JitModel, true, DR, true, os2r::JitLayout, false, os2r::kJitSolverStd, true>(A); \
  }
OS2R_JIT_ROLLOUT_KERNEL(os2r_jit_rollout_c1_d0, false)
OS2R_JIT_ROLLOUT_KERNEL(os2r_jit_rollout_c1_d1, true)
#else
// the one argument begins with the StepArgs: step_body reads the argument segment at offset 0
#define OS2R_JIT_POLICY_KERNEL(NAME, DR)                                                                               \
  extern "C" __global__ OS2R_STEP_KERNEL_ATTRS(OS2R_REAL) void NAME(const os2r::PolicyArgs<os2r::JitReal> P) {         \
    os2r::step_body<os2r::JitReal, os2r::JitModel, true, DR, true, os2r::JitLayout, false, os2r::kJitSolverStd, true,  \
                    true>(P.s);                                                                                        \
  }
// the _rec kernels read the sink of os2rr_rollout_policy_recorded (the fields appended to PolicyArgs): announced, because a kernel
// built without them would take the arguments and record nothing (os2r_register_model_kernels, include/os2r.h)
extern "C" __device__ __attribute__((used)) const unsigned int os2r_jit_policy_knots = 1u;
#define OS2R_JIT_POLICY_REC_KERNEL(NAME, DR)                                                                           \
  extern "C" __global__ OS2R_STEP_KERNEL_ATTRS(OS2R_REAL) void NAME(const os2r::PolicyArgs<os2r::JitReal> P) {         \
    os2r::step_body<os2r::JitReal, os2r::JitModel, true, DR, true, os2r::JitLayout, false, os2r::kJitSolverStd, true,  \
                    true, true>(P.s);                                                                                  \
  }
OS2R_JIT_POLICY_REC_KERNEL(os2r_jit_policy_rec_c1_d0, false)
OS2R_JIT_POLICY_REC_KERNEL(os2r_jit_policy_rec_c1_d1, true)
OS2R_JIT_POLICY_KERNEL(os2r_jit_policy_c1_d0, false)
OS2R_JIT_POLICY_KERNEL(os2r_jit_policy_c1_d1, true)
#endif
#endif

#if OS2R_JIT_KIND == 3
// one kernel per substep instantiation of the step object: NAME_s beside os2r_jit_step_..._s (and ..._l), NAME beside the
// plain step kernel; launched with grid.y = the number of columns
#define OS2R_JIT_LIN_KERNEL(NAME, CONTACT, DR)                                                                         \
  extern "C" __global__ OS2R_STEP_KERNEL_ATTRS(OS2R_REAL) void NAME(const os2r::LinArgs<os2r::JitReal> P) {            \
    os2r::linearize_body<os2r::JitReal, os2r::JitModel, CONTACT, DR, false, os2r::kJitSolverAny>(P);                   \
  }                                                                                                                    \
  extern "C" __global__ OS2R_STEP_KERNEL_ATTRS(OS2R_REAL) void NAME##_s(const os2r::LinArgs<os2r::JitReal> P) {        \
    os2r::linearize_body<os2r::JitReal, os2r::JitModel, CONTACT, DR, true, os2r::kJitSolverStd>(P);                    \
  }
#if OS2R_JIT_CONTACT
OS2R_JIT_LIN_KERNEL(os2r_jit_lin_c1_d0, true, false)
OS2R_JIT_LIN_KERNEL(os2r_jit_lin_c1_d1, true, true)
#else
OS2R_JIT_LIN_KERNEL(os2r_jit_lin_c0_d0, false, false)
OS2R_JIT_LIN_KERNEL(os2r_jit_lin_c0_d1, false, true)
#endif
#endif
