// os2r_partials.hpp — what the two sampling kernels (os2r_mppi.hpp, os2r_pf.hpp) share: sums over the samples of 64 robots kept as
// eight partials, one per wave, in LDS as [8][64] (gfx950, device only).  Both contracts (include/os2r_mppi.h step 4,
// include/os2r_pf.h step 6) name the same operations in the same order, so both kernels call the same functions.
//
// Not here: the running maximum-with-count of pass 1 and its eight-way combine after the barrier, five lines each, which both
// kernels still spell out.  As a function either one changes the code of the loops around it (through references the running
// pair is promoted a round later than the kernel's other locals and the loop variables change places; by value the combine
// loses its branches), and the by-value form measured 0.4 to 0.6 % slower in the particle filter at M = 1, S = 1 024 while
// the MPPI kernel gained up to 9 % (profiles/refactor_bodies_ab.txt; profiles/refactor_bodies_isa.txt has the forms tried).
#pragma once
#include "os2r_bits.hpp"

namespace os2r {

constexpr int kPartials = 8;        // waves of one workgroup: one partial each (OS2RM_CHUNKS, OS2RP_CHUNKS)
constexpr int kPartialLanes = 64;   // robots of one workgroup: one lane each in every wave

__device__ __forceinline__ double exp_of(double x) { return ::exp(x); }
__device__ __forceinline__ float exp_of(float x) { return ::expf(x); }

// the total of the eight partials of robot t
template <typename T>
__device__ __forceinline__ T partials_tree(const T* p, int t) {
#pragma clang fp contract(off)
  static_assert(kPartials == 8, "partials_tree is written for eight partials");
  constexpr int E = kPartialLanes;
  return ((p[0 * E + t] + p[1 * E + t]) + (p[2 * E + t] + p[3 * E + t])) + ((p[4 * E + t] + p[5 * E + t]) + (p[6 * E + t] + p[7 * E + t]));
}

}  // namespace os2r
