// os2r_lqr.hpp — os2r_lqr_gains: the backward Riccati recursion of many small LQR problems in one launch (gfx950).
//
// One environment per n + 2 lanes, n = 2 nq.  A workgroup is kLqrEnvs = 32 environments x (n + 2) columns, thread
// (column c, environment e) = c * 32 + e: the 32 lanes of one column read 32 consecutive elements of the environment-fastest
// arrays of os2r_linearize (256 B in fp64), and a wave holds two whole columns, so what differs between the column lanes
// (c < n, column c of A_k) and the input lanes (c = n + b, column b of B_k) is wave-uniform.  The arrays are addressed as one
// n x (n + 2) matrix [A_k | B_k]; lane c keeps its column v in registers.  Per knot, with P, A, B, G, K in LDS ([.][.][e],
// conflict-free: a half-wave reads 32 consecutive words, both half-waves of a b64 read are served apart):
//   top      the input lanes publish their column of B_k
//   barrier  (P' of the knot before and B_k are visible)
//   phase 1  every lane: pv = P v (column c of [PA | PB]), g_r = sum_l B[l][r] pv[l] -- for a column lane G[r][c], for the input
//            lane b the b-th column of B^T P B, so that S = R + that --; the column lanes publish their column of A_k.  The next
//            knot's column is requested before phase 1 and waits in registers.
//   barrier  (G, B^T P B and A_k are visible; nobody reads P any more)
//   phase 2  column lane j: S, det, the verdict, K[.][j] (two IEEE divisions) and P'[i][j], i <= j, written to both triangles
// and, when the weight table is asked for, a third barrier after which input lane b forms row b of the knot's weight set.
// No lane indexes a register array at run time, nothing goes to scratch (tests/test_lqr_gains_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r.h: the handle's dtype, no contraction, every sum of products
// ((x0 y0 + x1 y1) + x2 y2) + ... with the index ascending.  tests/test_gpu_lqr_gains.py restates it in numpy, bit for bit.
#pragma once
#include "os2r_device.hpp"

namespace os2r {

constexpr int kLqrEnvs = 32;                   // environments of one workgroup
constexpr int kLqrMaxN = 2 * OS2R_MAX_DOF;

// The chain length as a compile-time constant: f(std::integral_constant<int, NQ>()) for nq = NQ in 2..5 and 0, or 1 if there is
// no kernel for this nq.  The launches of os2r_lqr_inst.hip, os2r_ilqr_inst.hip and os2r_search_inst.hip go through it.
template <typename F>
int by_chain_length(int nq, F&& f) {
  switch (nq) {
    case 2: f(std::integral_constant<int, 2>()); return 0;
    case 3: f(std::integral_constant<int, 3>()); return 0;
    case 4: f(std::integral_constant<int, 4>()); return 0;
    case 5: f(std::integral_constant<int, 5>()); return 0;
    default: return 1;
  }
}

template <typename T>
struct LqrArgs {
  const T* __restrict__ a;         // [n][n][L], L = nknots * ntraj, lane of (knot k, trajectory m) = k * ntraj + m
  const T* __restrict__ b;         // [n][2][L]
  const T* p_final;                // [n][n][M] or null (Q); upper triangle read; p_out may alias it
  T* p_out;                        // [n][n][M] or null
  T* __restrict__ gain;            // [K][2][n][M] or null
  uint8_t* __restrict__ flag;      // [K][M] or null
  const T* __restrict__ actions;   // [L][2], with weights
  const T* __restrict__ obs;       // [L][D], with weights
  T* __restrict__ weights;         // [K][2][D+1][M] or null
  long long M;
  int K, sweeps, D;
  int slot_col[OS2R_MAX_OBS];      // state column a raw observation slot shows, -1: the slot carries no gain
  T r00, r01, r11;
  T q[kLqrMaxN * kLqrMaxN];        // [n][n] row-major, rounded to T by the host
};

// -x by its sign bit: what numpy's negation does to a zero too (the library is built with -fno-signed-zeros)
__device__ __forceinline__ double lqr_neg(double x) { return __longlong_as_double(__double_as_longlong(x) ^ (long long)0x8000000000000000ull); }
__device__ __forceinline__ float lqr_neg(float x) { return __int_as_float(__float_as_int(x) ^ (int)0x80000000u); }
// finite, by the bit pattern of a value the compiler knows nothing about (it is told that there are no NaNs)
__device__ __forceinline__ bool lqr_finite(double x) {
  return ((unsigned long long)__double_as_longlong(opaque(x)) >> 52 & 0x7ffull) != 0x7ffull;
}
__device__ __forceinline__ bool lqr_finite(float x) { return ((unsigned)__float_as_int(opaque(x)) >> 23 & 0xffu) != 0xffu; }

template <typename T, int NQ>
__global__ __launch_bounds__(kLqrEnvs * (2 * NQ + 2)) void lqr_gains_kernel(const LqrArgs<T> P) {
#pragma clang fp contract(off)
  constexpr int n = 2 * NQ, E = kLqrEnvs;
  __shared__ T sP[n * n * E], sA[n * n * E], sB[n * 2 * E], sG[2 * (n + 2) * E], sK[2 * n * E], sQ[n * n];
  const int e = threadIdx.x % E, c = threadIdx.x / E;   // c is uniform over a half-wave, c < n over a wave (n is even)
  const bool col_lane = c < n;
  const long long M = P.M, m_raw = (long long)blockIdx.x * E + e;
  const bool valid = m_raw < M;
  const long long m = valid ? m_raw : M - 1;            // tail lanes shadow the last trajectory, their stores are masked
  const int K = P.K;
  const long long L = (long long)K * M;
  // the lane's column of [A | B]: element l at src[l * stride + k * M]
  const T* src = col_lane ? P.a + (long long)c * L + m : P.b + (long long)(c - n) * L + m;
  const long long stride = (col_lane ? n : 2) * L;

  {  // Q for everybody (read with a lane index: from the argument segment as memory, not from a copy of the struct)
    const OS2R_CONST LqrArgs<T>* ka = (const OS2R_CONST LqrArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();
    if ((int)threadIdx.x < n * n) sQ[threadIdx.x] = ka->q[threadIdx.x];
  }
  __syncthreads();
  if (col_lane) {
#pragma unroll
    for (int i = 0; i < n; ++i)
      if (i <= c) {
        const T p = P.p_final ? P.p_final[(long long)(i * n + c) * M + m] : sQ[i * n + c];
        sP[(i * n + c) * E + e] = p;
        sP[(c * n + i) * E + e] = p;
      }
  }

  const long long total = (long long)P.sweeps * K;
  int k = K - 1;
  T v[n], vn[n];
#pragma unroll
  for (int l = 0; l < n; ++l) vn[l] = v[l] = src[l * stride + (long long)k * M];

  for (long long it = 0; it < total; ++it) {
    const bool last_sweep = it >= total - K;
    if (!col_lane) {
#pragma unroll
      for (int l = 0; l < n; ++l) sB[(l * 2 + (c - n)) * E + e] = v[l];
    }
    __syncthreads();
    // the next knot's column, in flight during this knot (one knot swept repeatedly keeps its column)
    const int kn = k == 0 ? K - 1 : k - 1;
    if (K > 1 && it + 1 < total) {
#pragma unroll
      for (int l = 0; l < n; ++l) vn[l] = src[l * stride + (long long)kn * M];
    }
    // phase 1
    T pv[n];
#pragma unroll
    for (int i = 0; i < n; ++i) {
      T acc = sP[(i * n + 0) * E + e] * v[0];
#pragma unroll
      for (int l = 1; l < n; ++l) acc = acc + sP[(i * n + l) * E + e] * v[l];
      pv[i] = acc;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      T acc = sB[(0 * 2 + r) * E + e] * pv[0];
#pragma unroll
      for (int l = 1; l < n; ++l) acc = acc + sB[(l * 2 + r) * E + e] * pv[l];
      sG[(r * (n + 2) + c) * E + e] = acc;
    }
    if (col_lane) {
#pragma unroll
      for (int l = 0; l < n; ++l) sA[(l * n + c) * E + e] = v[l];
    }
    __syncthreads();
    // phase 2
    if (col_lane) {
      const T s00 = P.r00 + sG[(0 * (n + 2) + n) * E + e];
      const T s01 = P.r01 + sG[(0 * (n + 2) + n + 1) * E + e];
      const T s11 = P.r11 + sG[(1 * (n + 2) + n + 1) * E + e];
      const T det = s00 * s11 - s01 * s01;
      const bool ok = lqr_finite(det) && s00 > T(0) && det > T(0);
      const T g0 = sG[(0 * (n + 2) + c) * E + e], g1 = sG[(1 * (n + 2) + c) * E + e];
      T k0 = (s11 * g0 - s01 * g1) / det;
      T k1 = (s00 * g1 - s01 * g0) / det;
      k0 = ok ? k0 : T(0);
      k1 = ok ? k1 : T(0);
      if (last_sweep && valid) {
        if (P.gain) {
          P.gain[(((long long)k * 2 + 0) * n + c) * M + m] = k0;
          P.gain[(((long long)k * 2 + 1) * n + c) * M + m] = k1;
        }
        if (P.flag && c == 0) P.flag[(long long)k * M + m] = ok ? 0 : 1;
      }
      if (P.weights) {
        sK[(0 * n + c) * E + e] = k0;
        sK[(1 * n + c) * E + e] = k1;
      }
#pragma unroll
      for (int i = 0; i < n; ++i)
        if (i <= c) {
          T acc = sA[(0 * n + i) * E + e] * pv[0];
#pragma unroll
          for (int l = 1; l < n; ++l) acc = acc + sA[(l * n + i) * E + e] * pv[l];
          const T gk = sG[(0 * (n + 2) + i) * E + e] * k0 + sG[(1 * (n + 2) + i) * E + e] * k1;
          const T p = (sQ[i * n + c] + acc) - gk;
          sP[(i * n + c) * E + e] = p;
          sP[(c * n + i) * E + e] = p;
        }
    }
    if (P.weights && last_sweep) {   // (a kernel argument and the loop counter: every wave takes the barrier or none)
      __syncthreads();
      if (!col_lane) {
        // row j = c - n of the knot's set: a = a0 - K (x - x_k) on the raw observation slots
        const int j = c - n, D = P.D;
        const long long lane = (long long)k * M + m;
        T* w = P.weights + (((long long)k * 2 + j) * (D + 1)) * M + m;
        T acc = T(0);
        bool first = true;
#pragma unroll
        for (int d = 0; d < OS2R_MAX_OBS; ++d)
          if (d < D) {
            const int sc = P.slot_col[d];
            T wd = T(0);
            if (sc >= 0) {
              wd = lqr_neg(sK[(j * n + sc) * E + e]);
              const T t = wd * P.obs[lane * D + d];
              acc = first ? t : acc + t;
              first = false;
            }
            if (valid) w[(long long)d * M] = wd;
          }
        T a0 = P.actions[2 * lane + j];
        a0 = a0 < T(-1) ? T(-1) : (a0 > T(1) ? T(1) : a0);
        if (valid) w[(long long)D * M] = a0 - acc;
      }
    }
#pragma unroll
    for (int l = 0; l < n; ++l) v[l] = vn[l];
    k = kn;
  }

  if (P.p_out) {
    __syncthreads();
    if (col_lane && valid) {
#pragma unroll
      for (int i = 0; i < n; ++i) P.p_out[(long long)(i * n + c) * M + m] = sP[(i * n + c) * E + e];
    }
  }
}

// the launch (os2r_lqr_inst.hip, once per dtype): 1 if there is no kernel for this nq
template <typename T>
int launch_lqr_gains(int nq, const LqrArgs<T>& args, hipStream_t stream);

}  // namespace os2r
