// os2r_mppi.hpp — os2rm_mppi_update: the MPPI update of many robots in one launch (gfx950).
//
// The grid is (ceil(M / 64), K output slots).  A workgroup is kMppiRobots = 64 robots x OS2RM_CHUNKS = 8 waves: wave c owns
// partial c of every sum over the samples (include/os2r_mppi.h, step 4), its lane t robot blockIdx.x * 64 + t, so thread
// (partial c, robot t) = c * 64 + t, what differs between partials is wave-uniform, and every load of returns and actions is
// contiguous across the lanes of a wave (lane s M + m: the robot index is the fastest).
//   pass 1   wave c walks its samples s = c, c + 8, ... for the maximum of the finite returns and their number
//   barrier  [8][64] maxima and counts are in LDS; every lane combines the eight of its robot (a maximum has no order)
//   pass 2   wave c walks its samples again: w = exp((r - rmax) beta), and the partials of wsum, Q and A of the source slot
//            min(k + shift, K - 1) together; the workgroups of slot 0 also form A of slot 0 (the action to apply) and write w
//   barrier  [8][64] partials are in LDS; every lane applies the fixed tree ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))
//   writes   wave 0 writes nominal_out[k] (and, in slot 0, applied, ess and count); the S bias entries of the robot's lanes in
//            slot k of the table are shared among the eight waves as the samples were, contiguous across a wave
// The weights are formed again by the workgroup of every output slot: S exp per robot and slot, against a second launch and
// an [S][M] array written and read back (DESIGN.md section 4 has the count).  The workgroup of slot k reads its source slot
// itself, so no workgroup waits for another -- and nominal_out must not be nominal_in.  With OS2RM_TAIL_ZERO the workgroups of
// the uncovered slots k > 0 form nothing and write zeros.
// Tail lanes shadow the last robot, their stores are masked.  No lane indexes a register array at run time, nothing goes to
// scratch (tests/test_mppi_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_mppi.h: the layout's dtype, no contraction, each partial in ascending order.
// tests/test_mppi_host.py restates it in numpy; tests/test_gpu_mppi.py compares bit for bit.
#pragma once
#include "os2r_partials.hpp"
#include "../../include/os2r_mppi.h"

namespace os2r {

constexpr int kMppiRobots = 64;             // robots of one workgroup: one lane each in every wave
constexpr int kMppiChunks = OS2RM_CHUNKS;   // waves of one workgroup: one partial each

template <typename T>
struct MppiArgs {
  const T* __restrict__ returns;      // [N], N = S * M, lane j = s * M + m
  const T* __restrict__ actions;      // [K][N][2], aligned to a pair
  const T* __restrict__ nominal_in;   // [K][M][2]
  T* __restrict__ nominal_out;        // [K][M][2]
  T* __restrict__ applied;            // [M][2] or null
  T* __restrict__ table;              // [K][2][D+1][N] or null: only [.][.][D][.] is written
  T* __restrict__ weights;            // [S][M] or null
  T* __restrict__ ess;                // [M] or null
  int* __restrict__ count;            // [M] or null
  long long M;
  int K, S, D, shift, tail_zero;
  T beta;                             // rounded to T by the host
};

// one action: both motors in one load
template <typename T>
struct alignas(2 * sizeof(T)) MppiPair {
  T x, y;
};

template <typename T>
__device__ __forceinline__ T mppi_clamp(T a) { return a < T(-1) ? T(-1) : (a > T(1) ? T(1) : a); }

template <typename T>
__global__ __launch_bounds__(kMppiRobots * kMppiChunks) void mppi_update_kernel(const MppiArgs<T> P) {
#pragma clang fp contract(off)
  static_assert(kMppiChunks == kPartials && kMppiRobots == kPartialLanes, "the partials of os2r_partials.hpp");
  constexpr int E = kMppiRobots, C = kMppiChunks;
  __shared__ T sMax[C * E], sW[C * E], sQ[C * E], sA[4 * C * E];
  __shared__ int sCnt[C * E];
  const int t = threadIdx.x % E, c = threadIdx.x / E;   // c, the partial, is uniform over a wave
  const long long M = P.M, m_raw = (long long)blockIdx.x * E + t;
  const bool valid = m_raw < M;
  const long long m = valid ? m_raw : M - 1;            // tail lanes shadow the last robot, their stores are masked
  const int K = P.K, S = P.S, k = (int)blockIdx.y;
  const long long N = (long long)S * M;
  const bool first = k == 0;                            // uniform over the workgroup, like everything about k
  const bool zeroed = P.tail_zero && k + P.shift >= K;
  const int ks = k + P.shift < K ? k + P.shift : K - 1; // the source slot
  // where slot k of the table holds the bias of motor 0 for lane 0; motor 1 is (D + 1) * N further
  T* const bias = P.table ? P.table + (((long long)k * 2 * (P.D + 1)) + P.D) * N : nullptr;
  const long long bias_step = (long long)(P.D + 1) * N;

  if (zeroed && !first) {                               // an uncovered slot: no sum is needed
    if (valid) {
      if (c == 0) {
        P.nominal_out[((long long)k * M + m) * 2] = T(0);
        P.nominal_out[((long long)k * M + m) * 2 + 1] = T(0);
      }
      if (bias)
        for (int s = c; s < S; s += C) {
          bias[(long long)s * M + m] = T(0);
          bias[bias_step + (long long)s * M + m] = T(0);
        }
    }
    return;
  }

  // pass 1: the maximum of the valid returns of partial c, and their number (steps 1 and 2)
  {
    T mx = T(0);
    int cnt = 0;
    for (int s = c; s < S; s += C) {
      const T r = P.returns[(long long)s * M + m];
      const bool ok = hi_finite(r);                     // (by its exponent bits: os2r_bits.hpp says why)
      const T rv = ok ? r : T(0);
      const bool take = ok && (cnt == 0 || rv > mx);
      mx = take ? rv : mx;
      cnt += ok ? 1 : 0;
    }
    sMax[c * E + t] = mx;
    sCnt[c * E + t] = cnt;
  }
  __syncthreads();
  T rmax = T(0);
  int count = 0;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    const T vi = sMax[i * E + t];
    const int ci = sCnt[i * E + t];
    const bool take = ci > 0 && (count == 0 || vi > rmax);
    rmax = take ? vi : rmax;
    count += ci;
  }

  // pass 2: the weights and the partials of wsum, Q, A of the source slot and, in slot 0, A of slot 0 (steps 3 and 4)
  {
    const T beta = P.beta;
    T pw = T(0), pq = T(0), pa0 = T(0), pa1 = T(0), pb0 = T(0), pb1 = T(0);
    const MppiPair<T>* const src = (const MppiPair<T>*)P.actions + (long long)ks * N;
    const MppiPair<T>* const now = (const MppiPair<T>*)P.actions;
    for (int s = c; s < S; s += C) {
      const long long lane = (long long)s * M + m;
      const T r = P.returns[lane];
      const MppiPair<T> a = src[lane];
      const bool ok = hi_finite(r);
      const T rv = ok ? r : rmax;
      const T e = exp_of((rv - rmax) * beta);
      const T w = ok ? e : T(0);
      pw = pw + w;
      pq = pq + w * w;
      pa0 = pa0 + w * a.x;
      pa1 = pa1 + w * a.y;
      if (first) {
        const MppiPair<T> b = now[lane];
        pb0 = pb0 + w * b.x;
        pb1 = pb1 + w * b.y;
        if (P.weights && valid) P.weights[lane] = w;
      }
    }
    sW[c * E + t] = pw;
    sQ[c * E + t] = pq;
    sA[(0 * C + c) * E + t] = pa0;
    sA[(1 * C + c) * E + t] = pa1;
    sA[(2 * C + c) * E + t] = pb0;
    sA[(3 * C + c) * E + t] = pb1;
  }
  __syncthreads();

  // steps 5 and 8: the value of slot k, the same in every wave
  const T wsum = partials_tree<T>(sW, t);
  T out0 = T(0), out1 = T(0);
  if (!zeroed) {
    if (count > 0) {
      out0 = mppi_clamp(partials_tree<T>(sA + 0 * C * E, t) / wsum);
      out1 = mppi_clamp(partials_tree<T>(sA + 1 * C * E, t) / wsum);
    } else {
      out0 = P.nominal_in[((long long)ks * M + m) * 2];
      out1 = P.nominal_in[((long long)ks * M + m) * 2 + 1];
    }
  }
  if (!valid) return;
  if (c == 0) {
    P.nominal_out[((long long)k * M + m) * 2] = out0;
    P.nominal_out[((long long)k * M + m) * 2 + 1] = out1;
    if (first) {                                        // steps 6 and 7
      if (P.applied) {
        T ap0, ap1;
        if (count > 0) {
          ap0 = mppi_clamp(partials_tree<T>(sA + 2 * C * E, t) / wsum);
          ap1 = mppi_clamp(partials_tree<T>(sA + 3 * C * E, t) / wsum);
        } else {
          ap0 = P.nominal_in[m * 2];
          ap1 = P.nominal_in[m * 2 + 1];
        }
        P.applied[m * 2] = ap0;
        P.applied[m * 2 + 1] = ap1;
      }
      if (P.ess) {
        const T q = partials_tree<T>(sQ, t);
        P.ess[m] = count > 0 ? (wsum * wsum) / q : T(0);
      }
      if (P.count) P.count[m] = count;
    }
  }
  // step 9: the bias entries of the robot's lanes in slot k
  if (bias)
    for (int s = c; s < S; s += C) {
      bias[(long long)s * M + m] = out0;
      bias[bias_step + (long long)s * M + m] = out1;
    }
}

// the launch (os2r_mppi_inst.hip, once per dtype)
template <typename T>
void launch_mppi_update(const MppiArgs<T>& args, hipStream_t stream);

}  // namespace os2r
