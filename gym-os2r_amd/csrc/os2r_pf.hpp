// os2r_pf.hpp — os2rp_pf_update: the particle-filter update of many robots in one launch (gfx950).
//
// The grid is ceil(M / 64) workgroups.  A workgroup is kPfRobots = 64 robots x OS2RP_CHUNKS = 8 waves, as in os2r_mppi.hpp: wave c
// owns partial c of every sum over the particles (include/os2r_pf.h, step 6), its lane t robot blockIdx.x * 64 + t, so thread
// (partial c, robot t) = c * 64 + t, what differs between partials is wave-uniform, and every load of obs and logw and every
// store of index is contiguous across the lanes of a wave (lane s M + m: the robot index is the fastest).
//   pass 1   wave c walks its particles s = c, c + 8, ...: l_s from the D entries of the observation, the maximum of the finite
//            ones and their number
//   barrier  [8][64] maxima and counts are in LDS; every lane combines the eight of its robot (a maximum has no order)
//   pass 2   wave c walks its particles again: l_s again, w = exp(l_s - lmax), the partials of wsum, Q and E together; it writes
//            logw_out = l_s - lmax (step 10: final for a robot that does not resample) and w where wanted
//   barrier  [8][64] partials are in LDS; every lane applies the fixed tree and decides whether its robot resamples (step 9), the
//            same in every wave: a ballot of one wave says whether any robot of the workgroup does
//   writes   wave 0 writes est, ess, count and resampled; the keep index -1 of a robot that does not resample is shared among
//            the eight waves as the particles were
//   resampling, only in a workgroup with a robot that resamples:
//     pass 3   wave c turns its own entries of logw_out back into weights, w = exp(logw_out) (the same function on the same
//              bits as in pass 2), in place
//     barrier  the weights of every particle are in logw_out_dev
//     prefix   wave 0, one lane per robot, walks s = 0 .. S-1 once: c_s = c_(s-1) + w_s, written over w_s, and the last positive
//              weight.  s is uniform, so the loads do not depend on what a lane has summed: sixteen are made ahead of the
//              adds; step and the last particle go to the other waves through LDS
//     barrier  the cumulative weights of every particle are in logw_out_dev
//     slots    the merge walk of step 11, told from the particles' side: particle s is the ancestor of the slots n with
//              c_(s-1) <= t_n < c_s, the slots k(c_(s-1)) .. k(c_s) - 1 where k(c) is the number of slots with t_n < c (t_n does
//              not decrease with n); the last particle with a positive weight also takes what is left, up to S.  Wave c
//              does its own particles s = c, c + 8, ..., four at a time: two loads each, k of both -- a guess from c / step
//              corrected by comparing with the t_n of the contract themselves, so the guess decides the speed and never the
//              result -- and one store per slot.  Every slot is written once
//     barrier  every cumulative weight has been read
//     zeros    logw_out = 0, shared among the eight waves
// Where the weights live between the passes: in logw_out_dev, behind a barrier -- S exp more per resampling robot, against an
// [S][64] array in LDS (which S would size) or a third read of the observations (DESIGN.md section 4 has the count).  A load
// that follows a store waits for it (both count on vmcnt and return out of order), so pass 3, the prefix and the slots each
// read a batch before they write one.
// Tail lanes shadow the last robot, their stores are masked and they take no part in the resampling passes.  No lane indexes a
// register array at run time (the loops over the observation entries are unrolled to OS2R_MAX_OBS, an entry i >= D selected
// away), nothing goes to scratch (tests/test_pf_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_pf.h: the layout's dtype, no contraction, each partial in ascending order.
// tests/test_pf_host.py restates it in numpy; tests/test_gpu_pf.py compares bit for bit.
#pragma once
#include "os2r_partials.hpp"
#include "../../include/os2r_pf.h"

namespace os2r {

constexpr int kPfRobots = 64;            // robots of one workgroup: one lane each in every wave
constexpr int kPfChunks = OS2RP_CHUNKS;  // waves of one workgroup: one partial each
constexpr int kPfObs = OS2R_MAX_OBS;     // the unrolled length of every loop over the observation entries

template <typename T>
struct PfArgs {
  const T* __restrict__ obs;      // [N][D], N = S * M, lane j = s * M + m
  const T* __restrict__ meas;     // [M][D]
  const T* __restrict__ prec;     // [D]
  const T* __restrict__ logw_in;  // [S][M] or null
  const T* __restrict__ u;        // [M] or null
  T* logw_out;                    // [S][M]; holds the weights between pass 3 and the walk
  int* __restrict__ index;        // [N]
  T* __restrict__ est;            // [M][D] or null
  T* __restrict__ weights;        // [S][M] or null
  T* __restrict__ ess;            // [M] or null
  int* __restrict__ count;        // [M] or null
  int* __restrict__ resampled;    // [M] or null
  long long M;
  int S, D;
  T ratio;                        // resample_ratio, rounded to T by the host
};

// A log-weight is found finite or not by its exponent bits (hi_finite: os2r_bits.hpp says why).  For the same reason -infinity is
// never a floating-point constant here: it is stored as its bits.
typedef long long __attribute__((may_alias)) pf_bits64;
typedef int __attribute__((may_alias)) pf_bits32;
// *p = ok ? x : -infinity, the choice made on the bits
__device__ __forceinline__ void pf_store_or_minus_inf(double* p, bool ok, double x) {
  *(pf_bits64*)p = ok ? __double_as_longlong(x) : (long long)0xfff0000000000000ull;
}
__device__ __forceinline__ void pf_store_or_minus_inf(float* p, bool ok, float x) {
  *(pf_bits32*)p = ok ? __float_as_int(x) : (int)0xff800000u;
}

// steps 1 and 2 for one lane: its observation into o, -> l.  pr, the precisions, are in LDS and read there for every particle, at
// an offset of 0 the compiler cannot see through: held in registers across the loop over the particles they are 24 SGPRs the
// fp64 kernel does not have (the first build spilled 94), and read as volatile each read waited for the one before it
template <typename T>
__device__ __forceinline__ T pf_log_weight(const PfArgs<T>& P, long long lane, const T (&y)[kPfObs], const T* pr, T (&o)[kPfObs]) {
#pragma clang fp contract(off)
  const T* const src = P.obs + lane * P.D;
  // every load is made, an entry i >= D from the last one: behind a branch on i < D each load waits for the one before it (the
  // first build took a memory round trip per entry).  Such an entry adds 0 to d2
  // (the twelve clamped offsets are formed here, from a D the compiler cannot see through: hoisted out of the loop over the
  // particles they are SGPRs the kernel does not have either)
  int last = P.D - 1;
  asm volatile("" : "+s"(last));
#pragma unroll
  for (int i = 0; i < kPfObs; ++i) o[i] = src[i < last ? i : last];
  // (and so is the load of the log-weight: without logw_in it reads an observation entry instead and the value is dropped)
  const T lw_read = *(P.logw_in ? P.logw_in + lane : src);
  const T lw = P.logw_in ? lw_read : T(0);
  int zero = 0;
  asm volatile("" : "+v"(zero));
  T d2 = T(0);
#pragma unroll
  for (int i = 0; i < kPfObs; ++i) {
    const T diff = o[i] - y[i];
    const T term = (diff * diff) * pr[i + zero];
    d2 = d2 + (i < P.D ? term : T(0));
  }
  return lw - T(0.5) * d2;
}

template <typename T>
__global__ __launch_bounds__(kPfRobots * kPfChunks) void pf_update_kernel(const PfArgs<T> P) {
#pragma clang fp contract(off)
  static_assert(kPfChunks == kPartials && kPfRobots == kPartialLanes, "the partials of os2r_partials.hpp");
  constexpr int E = kPfRobots, C = kPfChunks;
  __shared__ T sMax[C * E], sW[C * E], sQ[C * E], sE[kPfObs * C * E];
  __shared__ T sPrec[kPfObs];
  __shared__ int sCnt[C * E];
  const int t = threadIdx.x % E, c = threadIdx.x / E;   // c, the partial, is uniform over a wave
  if (threadIdx.x < kPfObs) sPrec[threadIdx.x] = (int)threadIdx.x < P.D ? P.prec[threadIdx.x] : T(0);
  const long long M = P.M, m_raw = (long long)blockIdx.x * E + t;
  const bool valid = m_raw < M;
  const long long m = valid ? m_raw : M - 1;            // tail lanes shadow the last robot, their stores are masked
  const int S = P.S, D = P.D;
  const bool want_est = P.est != nullptr;               // uniform over the grid

  T y[kPfObs], o[kPfObs];
#pragma unroll
  for (int i = 0; i < kPfObs; ++i) {
    y[i] = P.meas[m * D + (i < D ? i : D - 1)];   // (loaded without a branch, like the observations; an entry i >= D is not used)
    o[i] = T(0);
  }
  const T* const pr = sPrec;
  __syncthreads();

  // pass 1: the maximum of the valid log-weights of partial c, and their number (steps 1 to 4)
  {
    T mx = T(0);
    int cnt = 0;
    for (int s = c; s < S; s += C) {
      const T l = pf_log_weight<T>(P, (long long)s * M + m, y, pr, o);
      const bool ok = hi_finite(l);
      const T lv = ok ? l : T(0);
      const bool take = ok && (cnt == 0 || lv > mx);
      mx = take ? lv : mx;
      cnt += ok ? 1 : 0;
    }
    sMax[c * E + t] = mx;
    sCnt[c * E + t] = cnt;
  }
  __syncthreads();
  T lmax = T(0);
  int count = 0;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    const T vi = sMax[i * E + t];
    const int ci = sCnt[i * E + t];
    const bool take = ci > 0 && (count == 0 || vi > lmax);
    lmax = take ? vi : lmax;
    count += ci;
  }
  const bool lost = count == 0;

  // pass 2: the weights and the partials of wsum, Q and E (steps 5 and 6); logw_out as step 10 has it
  {
    T pw = T(0), pq = T(0), pe[kPfObs];
#pragma unroll
    for (int i = 0; i < kPfObs; ++i) pe[i] = T(0);
    for (int s = c; s < S; s += C) {
      const long long lane = (long long)s * M + m;
      const T l = pf_log_weight<T>(P, lane, y, pr, o);
      const bool ok = hi_finite(l);
      const T lv = ok ? l : lmax;
      const T arg = lv - lmax;
      const T e = exp_of(arg);
      const T w = ok ? e : T(0);
      pw = pw + w;
      pq = pq + w * w;
      if (want_est) {
#pragma unroll
        for (int i = 0; i < kPfObs; ++i)
          if (i < D) pe[i] = pe[i] + w * (ok ? o[i] : T(0));
      }
      if (valid) {
        pf_store_or_minus_inf(&P.logw_out[lane], ok || lost, arg);   // (a lost robot: arg = 0 in every lane)
        if (P.weights) P.weights[lane] = w;
      }
    }
    sW[c * E + t] = pw;
    sQ[c * E + t] = pq;
    if (want_est) {
#pragma unroll
      for (int i = 0; i < kPfObs; ++i)
        if (i < D) sE[(i * C + c) * E + t] = pe[i];
    }
  }
  __syncthreads();

  // steps 7 and 9, the same in every wave
  const T wsum = partials_tree<T>(sW, t);
  const T ess = lost ? T(0) : (wsum * wsum) / partials_tree<T>(sQ, t);
  const bool res = !lost && (ess < P.ratio * T(S) || count < S);
  const bool any_res = __builtin_amdgcn_ballot_w64(res) != 0;     // every wave holds the same 64 robots: uniform over the workgroup

  if (c == 0 && valid) {
    if (want_est)                                                   // step 8
      for (int i = 0; i < D; ++i) P.est[m * D + i] = lost ? P.meas[m * D + i] : partials_tree<T>(sE + i * C * E, t) / wsum;
    if (P.ess) P.ess[m] = ess;
    if (P.count) P.count[m] = count;
    if (P.resampled) P.resampled[m] = res ? 1 : 0;
  }
  if (valid && !res)                                                // step 10: keep
    for (int s = c; s < S; s += C) P.index[(long long)s * M + m] = -1;
  if (!any_res) return;

  // step 11.  pass 3: logw_out back into weights, every thread its own entries of pass 2
  if (valid && res) {
    T* const lw = P.logw_out + m;
    auto to_weight = [](T a) {
      const bool ok = hi_finite(a);
      const T e = exp_of(ok ? a : T(0));
      return ok ? e : T(0);
    };
    int s = c;
    for (; s + 3 * C < S; s += 4 * C) {                             // four loads ahead of the stores that follow them
      const long long j0 = (long long)s * M, j1 = (long long)(s + C) * M, j2 = (long long)(s + 2 * C) * M, j3 = (long long)(s + 3 * C) * M;
      const T a0 = lw[j0], a1 = lw[j1], a2 = lw[j2], a3 = lw[j3];
      const T e0 = to_weight(a0), e1 = to_weight(a1), e2 = to_weight(a2), e3 = to_weight(a3);
      lw[j0] = e0; lw[j1] = e1; lw[j2] = e2; lw[j3] = e3;
    }
    for (; s < S; s += C) lw[(long long)s * M] = to_weight(lw[(long long)s * M]);
  }
  __syncthreads();
  if (c == 0) {                                                     // the sequential prefix, in place
    T cs = T(0);
    int last = 0;
    if (res && valid) {
      T* const w = P.logw_out + m;                                  // w_s = w[s * M]
      auto take = [&](int s, T ws) {
        cs = cs + ws;
        last = ws > T(0) ? s : last;
        w[(long long)s * M] = cs;
      };
      int s = 0;
      for (; s + 16 <= S; s += 16) {                                // sixteen loads ahead of the stores that follow them
        const T* const g = w + (long long)s * M;
        const T a0 = g[0], a1 = g[M], a2 = g[2 * M], a3 = g[3 * M], a4 = g[4 * M], a5 = g[5 * M], a6 = g[6 * M], a7 = g[7 * M];
        const T a8 = g[8 * M], a9 = g[9 * M], a10 = g[10 * M], a11 = g[11 * M], a12 = g[12 * M], a13 = g[13 * M], a14 = g[14 * M], a15 = g[15 * M];
        take(s + 0, a0); take(s + 1, a1); take(s + 2, a2); take(s + 3, a3); take(s + 4, a4); take(s + 5, a5); take(s + 6, a6); take(s + 7, a7);
        take(s + 8, a8); take(s + 9, a9); take(s + 10, a10); take(s + 11, a11); take(s + 12, a12); take(s + 13, a13); take(s + 14, a14);
        take(s + 15, a15);
      }
      for (; s < S; ++s) take(s, w[(long long)s * M]);
    }
    sW[t] = cs / T(S);                                              // step
    sCnt[t] = last;
  }
  __syncthreads();
  if (res && valid) {
    const T step = sW[t], inv = T(1) / step;
    const int last = sCnt[t];
    T u = P.u ? P.u[m] : T(0.5);
    u = hi_finite(u) && u >= T(0) && u < T(1) ? u : T(0.5);
    // k(x): the number of slots n < S with t_n < x
    auto slots_below = [&](T x) {
      const T guess = x * inv - u;
      int k = guess <= T(0) ? 0 : (guess >= T(S) ? S : (int)guess);
      while (k < S && (T(k) + u) * step < x) ++k;
      while (k > 0 && !((T(k - 1) + u) * step < x)) --k;
      return k;
    };
    // c_i, for any i: read inside the array (where i is outside it the value is not used)
    auto cum = [&](int i) { return P.logw_out[(long long)(i < 0 ? 0 : (i < S ? i : S - 1)) * M + m]; };
    // the slots of particle s, from c_(s-1) and c_s; none behind the last particle
    auto emit = [&](int s, T below, T at) {
      if (s > last) return;
      const int lo = s == 0 ? 0 : slots_below(below);
      const int hi = s == last ? S : slots_below(at);
      for (int n = lo; n < hi; ++n) P.index[(long long)n * M + m] = (int)((long long)s * M + m);
    };
    for (int s = c; s <= last; s += 4 * C) {                        // the eight loads of four particles ahead of their stores
      const T b0 = cum(s - 1), a0 = cum(s), b1 = cum(s + C - 1), a1 = cum(s + C);
      const T b2 = cum(s + 2 * C - 1), a2 = cum(s + 2 * C), b3 = cum(s + 3 * C - 1), a3 = cum(s + 3 * C);
      emit(s, b0, a0);
      emit(s + C, b1, a1);
      emit(s + 2 * C, b2, a2);
      emit(s + 3 * C, b3, a3);
    }
  }
  __syncthreads();
  if (valid && res)
    for (int s = c; s < S; s += C) P.logw_out[(long long)s * M + m] = T(0);
}

// the launch (os2r_pf_inst.hip, once per dtype)
template <typename T>
void launch_pf_update(const PfArgs<T>& args, hipStream_t stream);

}  // namespace os2r
