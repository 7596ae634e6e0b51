// os2r_cem.hpp — os2rx_cem_update: the cross-entropy update of many robots in two stream-ordered launches (gfx950).
//
// cem_update_kernel, grid (ceil(M / 64), K knots).  A workgroup is kCemRobots = 64 robots x OS2RX_CHUNKS = 8 waves, the arrangement
// of mppi_update_kernel: wave c owns partial c of every sum over the samples (include/os2r_cem.h, step 3), its lane t robot
// blockIdx.x * 64 + t, so what differs between partials is wave-uniform and every load of returns and actions is contiguous
// across the lanes of a wave (lane s M + m: the robot index is the fastest).  The workgroup is indexed by the knot it FORMS, not
// by the slot it writes: the pooled variance needs all K knots, those a shift drops too.
//   count    wave c counts the finite returns among its samples s = c, c + 8, ...; [8][64] counts through LDS, e = min(E, count)
//   select   the e-th largest return of the robot, by a radix select on an order-preserving integer key of the return: two bits
//            a round from the top, wave c counts the lanes still in the race whose digit is 3, 2 or 1, [3][8][64] counts go
//            through LDS, every lane adds the eight of its robot and takes the digit that holds the e-th; what is left of e is
//            the place among the lanes that EQUAL the threshold, and the same rounds on the inverted sample index find the sample
//            at which the ties are cut.  One barrier a round: the counts alternate between two buffers, so a wave that runs a
//            round ahead writes the buffer nobody reads.  16 rounds for fp32, 32 for fp64, ceil(log4 S) for the ties
//   sums     wave c walks its samples for the partials of A (the elites' actions at knot k), barrier, the fixed tree, mu_e;
//            again for the partials of V (the squares of d = a - mu_e), barrier, the tree, var
//   writes   wave 0 writes var_out[k] and nominal_out of every slot that reads knot k: slot k - shift, and from knot K - 1 the
//            tail slots the shift uncovers; the S bias entries of the robot's lanes in those slots of the table are shared among
//            the eight waves as the samples were.  The workgroups of knot 0 also write applied, elite, threshold and count
// The elite set is found again by the workgroup of every knot, as MPPI's weights are (DESIGN.md section 4 has the count).
//
// cem_pool_kernel, grid ceil(M / 64), the same workgroup: the lanes of wave 0 count nothing alone -- the eight waves count the
// valid lanes as above --, then lane t of wave 0 adds var_out[0..K-1] of its robot in ascending order, forms sd and sigma_out
// (steps 9 and 10; it alone reads sigma_in and writes sigma_out of its robot, so the two may be one array), hands both values
// over in LDS, and the eight waves share the 2 S entries of lane_sigma.
//
// Tail lanes shadow the last robot, their stores are masked.  No lane indexes a register array at run time, nothing goes to
// scratch (tests/test_cem_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_cem.h: the layout's dtype, no contraction, each partial in ascending order.
// tests/test_cem_host.py restates it in numpy; tests/test_gpu_cem.py compares bit for bit.
#pragma once
#include "os2r_partials.hpp"
#include "../../include/os2r_cem.h"

namespace os2r {

constexpr int kCemRobots = 64;             // robots of one workgroup: one lane each in every wave
constexpr int kCemChunks = OS2RX_CHUNKS;   // waves of one workgroup: one partial each

template <typename T>
struct CemArgs {
  const T* __restrict__ returns;      // [N], N = S * M, lane j = s * M + m
  const T* __restrict__ actions;      // [K][N][2], aligned to a pair
  const T* __restrict__ nominal_in;   // [K][M][2]
  const T* sigma_in;                  // [2][M]; may be sigma_out
  T* __restrict__ nominal_out;        // [K][M][2]
  T* var_out;                         // [K][M][2]: written by the first launch, read by the second
  T* sigma_out;                       // [2][M]
  T* __restrict__ applied;            // [M][2] or null
  T* __restrict__ table;              // [K][2][D+1][N] or null: only [.][.][D][.] is written
  T* __restrict__ lane_sigma;         // [2][N] or null
  int* __restrict__ elite;            // [S][M] or null
  T* __restrict__ threshold;          // [M] or null
  int* __restrict__ count;            // [M] or null
  long long M;
  int K, S, E, D, shift, tail_zero;
  T gain, sigma_gain, sigma_min, sigma_max;   // rounded to T by the host
};

// one action: both motors in one load
template <typename T>
struct alignas(2 * sizeof(T)) CemPair {
  T x, y;
};

template <typename T>
__device__ __forceinline__ T cem_clamp(T a, T lo, T hi) { return a < lo ? lo : (a > hi ? hi : a); }

// one correctly rounded IEEE square root (os2r_ukf.hpp: the builtin gets the fix-up sequence in fp32 too)
__device__ __forceinline__ float cem_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double cem_sqrt(double x) { return __builtin_sqrt(x); }

// The order-preserving key of a return: an unsigned integer that compares as the value does, -0 and +0 equal.  Made of the bit
// pattern (os2r_bits.hpp says why); of a value that is not finite it is not used.
__device__ __forceinline__ unsigned cem_key(float r) {
  const unsigned b = steer_bits(r), z = b == 0x80000000u ? 0u : b;
  return (z >> 31) ? ~z : (z | 0x80000000u);
}
__device__ __forceinline__ unsigned long long cem_key(double r) {
  const unsigned long long b = steer_bits(r), z = b == 0x8000000000000000ull ? 0ull : b;
  return (z >> 63) ? ~z : (z | 0x8000000000000000ull);
}
__device__ __forceinline__ float cem_unkey(unsigned k) { return __int_as_float((int)((k >> 31) ? (k ^ 0x80000000u) : ~k)); }
__device__ __forceinline__ double cem_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

// The eight counts of robot t, added (an integer sum has no order).
__device__ __forceinline__ int cem_total(const int* p, int t) {
  int n = 0;
#pragma unroll
  for (int i = 0; i < kCemChunks; ++i) n += p[i * kCemRobots + t];
  return n;
}

// The radix select both orders go through: of the samples s = c, c + 8, ... of robot m for which key_of(return, s, key) holds, the
// need-th largest key (need >= 1 counts from the largest), two bits a round from bit `top` down to bit 0; need leaves as the
// place among the samples whose key IS the result.  `sel` is [2][3][8][64] ints, `buf` the half the next round writes (every
// use of sel alternates it, so one barrier a round is enough).  With need > the samples in the race the result is not used.
template <typename U, typename T, typename Key>
__device__ __forceinline__ U cem_select(const T* __restrict__ returns, long long M, long long m, Key key_of, int top, int S, int c, int t,
                                        int& need, int* sel, int& buf) {
  constexpr int E = kCemRobots, C = kCemChunks;
  U prefix = 0, mask = 0;
  for (int b = top - 2; b >= 0; b -= 2) {               // b: the lower bit of the round's digit
    int c1 = 0, c2 = 0, c3 = 0;
    auto tally = [&](T r, int s) {
      U key;
      const bool in = key_of(r, s, key);
      const bool race = in && (key & mask) == prefix;
      const unsigned d = (unsigned)(key >> b) & 3u;
      c1 += race && d == 1u ? 1 : 0;
      c2 += race && d == 2u ? 1 : 0;
      c3 += race && d == 3u ? 1 : 0;
    };
    int s = c;
    for (; s + 3 * C < S; s += 4 * C) {                 // four loads of a round are in flight together
      const T r0 = returns[(long long)s * M + m], r1 = returns[(long long)(s + C) * M + m];
      const T r2 = returns[(long long)(s + 2 * C) * M + m], r3 = returns[(long long)(s + 3 * C) * M + m];
      tally(r0, s);
      tally(r1, s + C);
      tally(r2, s + 2 * C);
      tally(r3, s + 3 * C);
    }
    for (; s < S; s += C) tally(returns[(long long)s * M + m], s);
    int* const cnt = sel + buf * 3 * C * E;
    cnt[(0 * C + c) * E + t] = c1;
    cnt[(1 * C + c) * E + t] = c2;
    cnt[(2 * C + c) * E + t] = c3;
    __syncthreads();
    const int n1 = cem_total(cnt + 0 * C * E, t), n2 = cem_total(cnt + 1 * C * E, t), n3 = cem_total(cnt + 2 * C * E, t);
    buf ^= 1;
    unsigned digit;
    if (n3 >= need) {
      digit = 3u;
    } else if (n3 + n2 >= need) {
      digit = 2u;
      need -= n3;
    } else if (n3 + n2 + n1 >= need) {
      digit = 1u;
      need -= n3 + n2;
    } else {
      digit = 0u;
      need -= n3 + n2 + n1;
    }
    prefix |= (U)digit << b;
    mask |= (U)3u << b;
  }
  return prefix;
}

// The valid lanes of robot m, counted by the eight waves (step 1); every lane leaves with the count of its robot.
template <typename T>
__device__ __forceinline__ int cem_count(const T* __restrict__ returns, long long M, long long m, int S, int c, int t, int* sel,
                                         int& buf) {
  constexpr int E = kCemRobots, C = kCemChunks;
  int cnt = 0;
  for (int s = c; s < S; s += C) cnt += hi_finite(returns[(long long)s * M + m]) ? 1 : 0;   // (by its exponent bits: os2r_bits.hpp)
  int* const p = sel + buf * 3 * C * E;
  p[c * E + t] = cnt;
  __syncthreads();
  buf ^= 1;
  return cem_total(p, t);
}

template <typename T>
__global__ __launch_bounds__(kCemRobots * kCemChunks) void cem_update_kernel(const CemArgs<T> P) {
#pragma clang fp contract(off)
  static_assert(kCemChunks == kPartials && kCemRobots == kPartialLanes, "the partials of os2r_partials.hpp");
  constexpr int E = kCemRobots, C = kCemChunks;
  using U = decltype(cem_key(T(0)));
  __shared__ int sSel[2 * 3 * C * E];
  __shared__ T sA[2 * C * E], sV[2 * C * E];
  const int t = threadIdx.x % E, c = threadIdx.x / E;   // c, the partial, is uniform over a wave
  const long long M = P.M, m_raw = (long long)blockIdx.x * E + t;
  const bool valid = m_raw < M;
  const long long m = valid ? m_raw : M - 1;            // tail lanes shadow the last robot, their stores are masked
  const int K = P.K, S = P.S, k = (int)blockIdx.y;      // k: the knot this workgroup forms, uniform over it
  const long long N = (long long)S * M;
  const bool first = k == 0;
  const T* const ret = P.returns;
  int buf = 0;

  // steps 1 and 2: the count, the threshold key and the sample at which its ties are cut
  const int count = cem_count<T>(ret, M, m, S, c, t, sSel, buf);
  const int e = count < P.E ? count : P.E;
  int need = e;
  const U thr = cem_select<U>(ret, M, m, [&](T r, int s, U& key) {
    key = cem_key(r);
    return hi_finite(r);
  }, 8 * (int)sizeof(U), S, c, t, need, sSel, buf);
  int index_bits = 0;
  while (index_bits < 32 && (1ll << index_bits) < (long long)S) index_bits += 2;     // an even number of bits that holds S - 1
  const unsigned index_full = index_bits >= 32 ? 0xffffffffu : (1u << index_bits) - 1u;
  const unsigned cut_inv = cem_select<unsigned>(ret, M, m, [&](T r, int s, unsigned& key) {
    key = index_full - (unsigned)s;                     // the lower sample has the larger key
    return hi_finite(r) && cem_key(r) == thr;
  }, index_bits, S, c, t, need, sSel, buf);
  const int cut = (int)(index_full - cut_inv);          // the last sample among the ties that is an elite
  auto is_elite = [&](T r, int s) {
    const U key = cem_key(r);
    return hi_finite(r) && (key > thr || (key == thr && s <= cut));
  };

  // steps 3 and 4: the partials of A, the tree, mu_e; the partials of V, the tree, var
  const CemPair<T>* const act = (const CemPair<T>*)P.actions + (long long)k * N;
  {
    T pa0 = T(0), pa1 = T(0);
    for (int s = c; s < S; s += C) {
      const long long lane = (long long)s * M + m;
      const T r = ret[lane];
      const CemPair<T> a = act[lane];
      const bool el = is_elite(r, s);
      pa0 = el ? pa0 + a.x : pa0;
      pa1 = el ? pa1 + a.y : pa1;
      if (first && P.elite && valid) P.elite[lane] = el ? 1 : 0;
    }
    sA[(0 * C + c) * E + t] = pa0;
    sA[(1 * C + c) * E + t] = pa1;
  }
  __syncthreads();
  const T te = (T)e;
  const T mu0 = partials_tree<T>(sA + 0 * C * E, t) / te, mu1 = partials_tree<T>(sA + 1 * C * E, t) / te;
  {
    T pv0 = T(0), pv1 = T(0);
    for (int s = c; s < S; s += C) {
      const long long lane = (long long)s * M + m;
      const T r = ret[lane];
      const CemPair<T> a = act[lane];
      const bool el = is_elite(r, s);
      const T d0 = a.x - mu0, d1 = a.y - mu1;
      pv0 = el ? pv0 + d0 * d0 : pv0;
      pv1 = el ? pv1 + d1 * d1 : pv1;
    }
    sV[(0 * C + c) * E + t] = pv0;
    sV[(1 * C + c) * E + t] = pv1;
  }
  __syncthreads();
  if (!valid) return;                                   // (behind the last barrier)

  // step 5: the mean of knot k, the same in every wave
  const T nom0 = P.nominal_in[((long long)k * M + m) * 2], nom1 = P.nominal_in[((long long)k * M + m) * 2 + 1];
  T mean0 = nom0, mean1 = nom1, var0 = T(0), var1 = T(0);
  if (count > 0) {
    var0 = partials_tree<T>(sV + 0 * C * E, t) / te;
    var1 = partials_tree<T>(sV + 1 * C * E, t) / te;
    if (P.gain == T(1)) {
      mean0 = cem_clamp(mu0, T(-1), T(1));
      mean1 = cem_clamp(mu1, T(-1), T(1));
    } else {
      mean0 = cem_clamp(nom0 + P.gain * (mu0 - nom0), T(-1), T(1));
      mean1 = cem_clamp(nom1 + P.gain * (mu1 - nom1), T(-1), T(1));
    }
  }
  if (c == 0) {
    P.var_out[((long long)k * M + m) * 2] = var0;
    P.var_out[((long long)k * M + m) * 2 + 1] = var1;
    if (first) {                                        // step 7, and what the selection found
      if (P.applied) {
        P.applied[m * 2] = mean0;
        P.applied[m * 2 + 1] = mean1;
      }
      if (P.threshold) P.threshold[m] = count > 0 ? cem_unkey(thr) : T(0);
      if (P.count) P.count[m] = count;
    }
  }

  // steps 6 and 8: every slot that reads knot k, and the bias entries of the robot's lanes in it
  const long long bias_step = (long long)(P.D + 1) * N;
  auto write_slot = [&](int slot, T v0, T v1) {
    if (c == 0) {
      P.nominal_out[((long long)slot * M + m) * 2] = v0;
      P.nominal_out[((long long)slot * M + m) * 2 + 1] = v1;
    }
    if (P.table) {
      // where slot `slot` of the table holds the bias of motor 0 for lane 0; motor 1 is (D + 1) * N further
      T* const bias = P.table + (((long long)slot * 2 * (P.D + 1)) + P.D) * N;
      for (int s = c; s < S; s += C) {
        bias[(long long)s * M + m] = v0;
        bias[bias_step + (long long)s * M + m] = v1;
      }
    }
  };
  if (k >= P.shift) write_slot(k - P.shift, mean0, mean1);
  if (k == K - 1) {                                     // the slots the shift uncovers: held, or zeros
    const T h0 = P.tail_zero ? T(0) : mean0, h1 = P.tail_zero ? T(0) : mean1;
    for (int slot = K - P.shift; slot < K; ++slot) write_slot(slot, h0, h1);
  }
}

template <typename T>
__global__ __launch_bounds__(kCemRobots * kCemChunks) void cem_pool_kernel(const CemArgs<T> P) {
#pragma clang fp contract(off)
  constexpr int E = kCemRobots, C = kCemChunks;
  __shared__ int sSel[3 * C * E];
  __shared__ T sSig[2 * E];
  const int t = threadIdx.x % E, c = threadIdx.x / E;
  const long long M = P.M, m_raw = (long long)blockIdx.x * E + t;
  const bool valid = m_raw < M;
  const long long m = valid ? m_raw : M - 1;
  const int K = P.K, S = P.S;
  const long long N = (long long)S * M;
  int buf = 0;
  const int count = cem_count<T>(P.returns, M, m, S, c, t, sSel, buf);
  if (c == 0) {
    // steps 9 and 10: this lane alone reads sigma_in and writes sigma_out of robot m (a shadow reads only)
    T acc0 = T(0), acc1 = T(0);
    for (int k = 0; k < K; ++k) {
      acc0 = acc0 + P.var_out[((long long)k * M + m) * 2];
      acc1 = acc1 + P.var_out[((long long)k * M + m) * 2 + 1];
    }
    const T tk = (T)K;
    const T sd0 = cem_sqrt(acc0 / tk), sd1 = cem_sqrt(acc1 / tk);
    const T in0 = P.sigma_in[m], in1 = P.sigma_in[M + m];
    T out0 = in0, out1 = in1;
    if (count > 0) {
      const T g0 = P.sigma_gain == T(1) ? sd0 : in0 + P.sigma_gain * (sd0 - in0);
      const T g1 = P.sigma_gain == T(1) ? sd1 : in1 + P.sigma_gain * (sd1 - in1);
      out0 = cem_clamp(g0, P.sigma_min, P.sigma_max);
      out1 = cem_clamp(g1, P.sigma_min, P.sigma_max);
    }
    if (valid) {
      P.sigma_out[m] = out0;
      P.sigma_out[M + m] = out1;
    }
    sSig[t] = out0;
    sSig[E + t] = out1;
  }
  if (!P.lane_sigma) return;                            // uniform over the grid
  __syncthreads();
  if (!valid) return;
  // step 11: the robot's lanes, shared among the waves as the samples were
  const T s0 = sSig[t], s1 = sSig[E + t];
  for (int s = c; s < S; s += C) {
    P.lane_sigma[(long long)s * M + m] = s0;
    P.lane_sigma[N + (long long)s * M + m] = s1;
  }
}

// the two launches (os2r_cem_inst.hip, once per dtype)
template <typename T>
void launch_cem_update(const CemArgs<T>& args, hipStream_t stream);

}  // namespace os2r
