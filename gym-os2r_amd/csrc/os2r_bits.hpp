// os2r_bits.hpp — the bits of a floating-point value, and the class tests made of them (gfx950, device only).
//
// The libraries are built with -fno-honor-nans -fno-honor-infinities, so a value is found finite, NaN or negative by its bit
// pattern, and the word that holds the bits passes through an empty asm on the INTEGER: what comes out has no floating-point
// history, so the tests below are compiled as written.  Hiding the floating-point value alone is not enough: the compiler
// recognises the mask-and-compare on the bits of a float that passed through an asm as a float -- lqr_finite of os2r_lqr.hpp -- as
// a class test of that float and, told that there are neither NaNs nor infinities, folds it to true (the first build of the MPPI
// kernel counted every lane valid; DESIGN.md section 4 has what the assembly holds in place of lqr_finite).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace os2r {

// the whole value
__device__ __forceinline__ unsigned steer_bits(float x) {
  unsigned b = (unsigned)__float_as_int(x);
  asm volatile("" : "+v"(b));
  return b;
}
__device__ __forceinline__ unsigned long long steer_bits(double x) {
  unsigned long long b = (unsigned long long)__double_as_longlong(x);
  asm volatile("" : "+v"(b));
  return b;
}
__device__ __forceinline__ bool steer_finite(float x) { return (steer_bits(x) >> 23 & 0xffu) != 0xffu; }
__device__ __forceinline__ bool steer_finite(double x) { return (steer_bits(x) >> 52 & 0x7ffull) != 0x7ffull; }
__device__ __forceinline__ bool steer_nan(float x) { return (steer_bits(x) & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ bool steer_nan(double x) { return (steer_bits(x) & 0x7fffffffffffffffull) > 0x7ff0000000000000ull; }
// negative, or not finite: by the sign bit of a value that is no zero
__device__ __forceinline__ bool steer_invalid(float x) {
  const unsigned b = steer_bits(x);
  return (b >> 23 & 0xffu) == 0xffu || (b >> 31 != 0u && (b & 0x7fffffffu) != 0u);
}
__device__ __forceinline__ bool steer_invalid(double x) {
  const unsigned long long b = steer_bits(x);
  return (b >> 52 & 0x7ffull) == 0x7ffull || (b >> 63 != 0ull && (b & 0x7fffffffffffffffull) != 0ull);
}
__device__ __forceinline__ double steer_abs(double x) { return __longlong_as_double(__double_as_longlong(x) & 0x7fffffffffffffffll); }
__device__ __forceinline__ float steer_abs(float x) { return __int_as_float(__float_as_int(x) & 0x7fffffff); }

// the word that holds the exponent alone: of a double only the high half passes through the asm (the sampling kernels, which test
// one value per sample in their inner loops)
__device__ __forceinline__ unsigned hi_opaque_bits(unsigned b) { asm volatile("" : "+v"(b)); return b; }
__device__ __forceinline__ bool hi_finite(double x) { return (hi_opaque_bits((unsigned)__double2hiint(x)) >> 20 & 0x7ffu) != 0x7ffu; }
__device__ __forceinline__ bool hi_finite(float x) { return (hi_opaque_bits((unsigned)__float_as_int(x)) >> 23 & 0xffu) != 0xffu; }

}  // namespace os2r
