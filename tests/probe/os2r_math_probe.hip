// os2r_math_probe.hip — test-only: the device math primitives of the step kernels, one thread per argument (gfx950).
//
// Built by tests/math_probe.py with the flags of the library (jit.FLAGS), so every primitive is compiled under the same
// no-NaN / no-infinity / no-signed-zero semantics as in the kernels.  The project's own headers are included, not copies.
// Never linked into, or loaded by, anything under gym-os2r_amd/.
//
// Every kernel is straight-line element-wise code on a workgroup of 256 (four full waves; only the tail is partial), reads
// the arguments it is given and writes out[f * n + i] for function f of argument i.
#include "../../gym-os2r_amd/csrc/os2r_kernels.hpp"
#include "../../gym-os2r_amd/csrc/os2r_partials.hpp"
#include "../../gym-os2r_amd/csrc/os2r_bits.hpp"

namespace {

using namespace os2r;
constexpr int kBlock = 256;

// 1. sin/cos: out = [fast s, fast c, lib s, lib c, selected s, selected c][n]; the selection is the lane's own, under a
// divergent branch, as in substep step 1
template <typename T>
__global__ void __launch_bounds__(kBlock) k_sincos(const T* __restrict__ x, T* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const T v = x[i];
  T s, c;
  sincos_fast(v, s, c);
  out[0 * n + i] = s; out[1 * n + i] = c;
  sincos_lib(v, s, c);
  out[2 * n + i] = s; out[3 * n + i] = c;
  if (sincos_in_range(v)) sincos_fast(v, s, c);
  else sincos_lib(v, s, c);
  out[4 * n + i] = s; out[5 * n + i] = c;
}

// 2. out = [rcp_t, rcp_group<3>, rcp_group<5>, rsqrt_t, sqrt_t][n].  In a group argument i sits in slot i mod N next to its
// cyclic neighbours of the argument array; rsqrt_t and sqrt_t take |x|.
template <int N, typename T>
__device__ __forceinline__ T group_of(const T* __restrict__ x, long long i, long long n) {
  T a[N], r[N];
  const int slot = (int)(i % N);
#pragma unroll
  for (int j = 0; j < N; ++j) a[j] = x[(i + n + j - slot) % n];
  rcp_group<N>(a, r);
  T o = r[0];
#pragma unroll
  for (int j = 1; j < N; ++j) o = j == slot ? r[j] : o;
  return o;
}
template <typename T>
__global__ void __launch_bounds__(kBlock) k_recip(const T* __restrict__ x, T* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const T v = x[i], a = steer_abs(v);
  out[0 * n + i] = rcp_t(v);
  out[1 * n + i] = group_of<3>(x, i, n);
  out[2 * n + i] = group_of<5>(x, i, n);
  out[3 * n + i] = rsqrt_t(a);
  out[4 * n + i] = sqrt_t(a);
}

// 3. out = [tanh_t, wrap_pi][n]
template <typename T>
__global__ void __launch_bounds__(kBlock) k_tanh(const T* __restrict__ x, T* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = tanh_t(x[i]);
}
template <typename T>
__global__ void __launch_bounds__(kBlock) k_wrap(const T* __restrict__ x, T* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = wrap_pi(x[i]);
}

// 4. class tests on bit patterns: cls = [finite_t, hi_finite, steer_finite, steer_nan, steer_invalid][n] bytes, mag = the bits
// of steer_abs
template <typename T, typename B>
__global__ void __launch_bounds__(kBlock) k_class(const B* __restrict__ bits, uint8_t* __restrict__ cls, B* __restrict__ mag, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  T v;
  const B b = bits[i];
  __builtin_memcpy(&v, &b, sizeof(T));
  cls[0 * n + i] = finite_t(v) ? 1 : 0;
  cls[1 * n + i] = hi_finite(v) ? 1 : 0;
  cls[2 * n + i] = steer_finite(v) ? 1 : 0;
  cls[3 * n + i] = steer_nan(v) ? 1 : 0;
  cls[4 * n + i] = steer_invalid(v) ? 1 : 0;
  const T a = steer_abs(v);
  B m;
  __builtin_memcpy(&m, &a, sizeof(T));
  mag[i] = m;
}

// 5. tup = [seed lo, seed hi, env, stream, ctr, blk][n] words; out = [z0, z1, u0, u1][n]
__global__ void __launch_bounds__(kBlock) k_normal(const uint32_t* __restrict__ tup, double* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const unsigned long long seed = (unsigned long long)tup[0 * n + i] | ((unsigned long long)tup[1 * n + i] << 32);
  const uint32_t env = tup[2 * n + i], stream = tup[3 * n + i], ctr = tup[4 * n + i], blk = tup[5 * n + i];
  double z0, z1, u0, u1;
  normal2(seed, env, stream, ctr, blk, z0, z1);
  uniform2(seed, env, stream, ctr, blk, u0, u1);
  out[0 * n + i] = z0; out[1 * n + i] = z1; out[2 * n + i] = u0; out[3 * n + i] = u1;
}
// the word path of uniform2 and the Box-Muller of normal2 on crafted words: w = [a, b, c, d][n]; out = [u53(a, b), u53(c, d),
// r = sqrt(-2 log(1 - u0)), r cos(2 pi u1), r sin(2 pi u1)][n]
__global__ void __launch_bounds__(kBlock) k_words(const uint32_t* __restrict__ w, double* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double u0 = u53(w[0 * n + i], w[1 * n + i]), u1 = u53(w[2 * n + i], w[3 * n + i]);
  const double r = sqrt(-2.0 * log(1.0 - u0));
  const double th = 6.283185307179586476925286766559 * u1;
  out[0 * n + i] = u0; out[1 * n + i] = u1; out[2 * n + i] = r; out[3 * n + i] = r * cos(th); out[4 * n + i] = r * sin(th);
}

inline unsigned blocks(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }
inline int done() { return (int)hipGetLastError(); }

}  // namespace

#define PROBE_CHECK(n) if ((n) <= 0 || (n) > (1ll << 22)) return (int)hipErrorInvalidValue

extern "C" {
int probe_sincos_f64(const double* x, double* out, long long n, hipStream_t st) { PROBE_CHECK(n); k_sincos<double><<<blocks(n), kBlock, 0, st>>>(x, out, n); return done(); }
int probe_sincos_f32(const float* x, float* out, long long n, hipStream_t st) { PROBE_CHECK(n); k_sincos<float><<<blocks(n), kBlock, 0, st>>>(x, out, n); return done(); }
int probe_recip_f64(const double* x, double* out, long long n, hipStream_t st) { PROBE_CHECK(n); k_recip<double><<<blocks(n), kBlock, 0, st>>>(x, out, n); return done(); }
int probe_recip_f32(const float* x, float* out, long long n, hipStream_t st) { PROBE_CHECK(n); k_recip<float><<<blocks(n), kBlock, 0, st>>>(x, out, n); return done(); }
int probe_tanh_f64(const double* x, double* out, long long n, hipStream_t st) { PROBE_CHECK(n); k_tanh<double><<<blocks(n), kBlock, 0, st>>>(x, out, n); return done(); }
int probe_tanh_f32(const float* x, float* out, long long n, hipStream_t st) { PROBE_CHECK(n); k_tanh<float><<<blocks(n), kBlock, 0, st>>>(x, out, n); return done(); }
int probe_wrap_f64(const double* x, double* out, long long n, hipStream_t st) { PROBE_CHECK(n); k_wrap<double><<<blocks(n), kBlock, 0, st>>>(x, out, n); return done(); }
int probe_wrap_f32(const float* x, float* out, long long n, hipStream_t st) { PROBE_CHECK(n); k_wrap<float><<<blocks(n), kBlock, 0, st>>>(x, out, n); return done(); }
int probe_class_f64(const unsigned long long* bits, uint8_t* cls, unsigned long long* mag, long long n, hipStream_t st) {
  PROBE_CHECK(n); k_class<double, unsigned long long><<<blocks(n), kBlock, 0, st>>>(bits, cls, mag, n); return done();
}
int probe_class_f32(const uint32_t* bits, uint8_t* cls, uint32_t* mag, long long n, hipStream_t st) {
  PROBE_CHECK(n); k_class<float, uint32_t><<<blocks(n), kBlock, 0, st>>>(bits, cls, mag, n); return done();
}
int probe_normal(const uint32_t* tup, double* out, long long n, hipStream_t st) { PROBE_CHECK(n); k_normal<<<blocks(n), kBlock, 0, st>>>(tup, out, n); return done(); }
int probe_words(const uint32_t* w, double* out, long long n, hipStream_t st) { PROBE_CHECK(n); k_words<<<blocks(n), kBlock, 0, st>>>(w, out, n); return done(); }
}
