// os2r_norm.hpp — os2rz_obs_stats, os2rz_fold and os2rz_unfold: running observation whitening of many linear policies (gfx950),
// four kernels; the sum over more than 64 samples of a policy is the body of os2r_pg.hpp as it is, the one over up to 64 is written
// here (norm_push says why).
//
// os2rz_obs_stats, two launches:
//   norm_lane_kernel, grid ceil(N / (256 / D)).  obs is [K][N][D]: a matrix of K rows and N D columns, and column l D + d holds
//     what lane l saw of component d.  A thread owns one column: the loads of a wave are one contiguous span per step, and the two
//     sums of a (lane, component) are chains of the thread's own, so no sum is exchanged.  The order of the additions is the
//     contract's, k ascending; the order of the loads is not: kNormSteps steps' loads depend on no accumulator and are issued
//     before the first is used, which is what hides the chain of 2 K dependent operations where there are few lanes.  A
//     workgroup holds 256 / D whole lanes (at D = 10 six of its 256 threads idle), so that a lane's D verdicts meet in LDS: the
//     thread of component 0 writes the lane's len and whether all 2 D sums are finite
//   norm_sum_kernel (S > 64), grid (P, D), four waves each: pg_wave_sum over the rows d and D + d of lane_sum and the two rows of
//     lane_count, a wave a sum; norm_sum_few_kernel (S <= 64), grid (ceil(P / 256), D), one thread each: the same partials and tree, formed as
//     the samples arrive.  Then the merge of (policy, component) by the one thread that holds the totals.  The integer sums are
//     formed by all D waves (or threads) of a policy -- D times two loads per sample against a launch and a scratch array less
// os2rz_fold and os2rz_unfold, one launch: norm_fold_kernel, grid ceil(Q rows / 256), a thread per (set, row) that walks the
//   row's D entries once: the bias is a chain over them.  With the policy index fastest neighbouring threads read neighbouring
//   sets; without it a thread reads its row's D + 1 contiguous values.
// No lane indexes a register array at run time, nothing goes to scratch (tests/test_norm_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_norm.h: the layout's dtype, no contraction, every chain in the order given
// there.  tests/test_norm_host.py restates it in numpy; tests/test_gpu_norm.py compares bit for bit.
#pragma once
#include "os2r_pg.hpp"
#include "../../include/os2r_norm.h"

namespace os2r {

constexpr int kNormBlock = 256;                  // threads of a workgroup of every kernel but the wave sum
constexpr int kNormSteps = 16;                   // steps of one round of the lane kernel: their loads are in flight together
constexpr int kNormTail = 4;                     // ... and of the rounds behind the last full one
constexpr int kNormLevels = 6;                   // of the adjacent-pair tree
constexpr int kNormSumWaves = 4;                 // waves of a workgroup of the wave sum: A, B, the steps and the valid lanes
static_assert(OS2RZ_CHUNKS == kPgChunks && (1 << kNormLevels) == kPgChunks && OS2R_MAX_OBS <= kNormBlock, "the partials are the score-function library's");

template <typename T>
struct StatsArgs {
  const T* __restrict__ obs;          // [K][N][D]
  const T* __restrict__ obs0;         // [N][D] or null
  const int* __restrict__ length;     // [N] or null
  const long long* __restrict__ count_in;   // [P], or null with mean_in and m2_in: every policy empty
  const T* __restrict__ mean_in;      // [P][D]
  const T* __restrict__ m2_in;        // [P][D]
  long long* __restrict__ count_out;  // [P]
  T* __restrict__ mean_out;           // [P][D]
  T* __restrict__ m2_out;             // [P][D]
  int* __restrict__ steps;            // [P] or null
  int* __restrict__ valid;            // [P] or null
  T* lane_sum;                        // [2 D][N]: written by the first launch, read by the second
  int* lane_count;                    // [2][N]: len, valid; as lane_sum
  long long P, N;
  int K, S, D, lanes_per_block;       // 256 / D
};

template <typename T>
struct FoldArgs {
  const long long* __restrict__ count;      // [P], or null with mean and m2: every policy empty
  const T* __restrict__ mean;         // [P][D]
  const T* __restrict__ m2;           // [P][D]
  const T* __restrict__ in;           // theta (fold) or the gradient (unfold)
  T* __restrict__ out;
  long long P, Q;                     // Q sets, set q under the statistics of policy q % P
  int rows, D, fastest, unfold;
  T floor;                            // rounded to T by the host
};

__device__ __forceinline__ int norm_len(const int* __restrict__ length, long long l, int K) {
  const int len = length ? length[l] : K;
  return len < 0 ? 0 : (len > K ? K : len);
}

// step 1: the pivot of (policy, component), the same in both launches
template <typename T>
__device__ __forceinline__ T norm_pivot(const StatsArgs<T>& A, long long p, int d) {
  if (A.count_in && A.count_in[p] > 0) return A.mean_in[p * A.D + d];
  if (norm_len(A.length, p, A.K) <= 0) return T(0);     // lane p is sample 0 of policy p
  const T x0 = A.obs0 ? A.obs0[p * A.D + d] : A.obs[p * A.D + d];
  return steer_finite(x0) ? x0 : T(0);
}

template <typename T>
__global__ __launch_bounds__(kNormBlock) void norm_lane_kernel(const StatsArgs<T> A) {
#pragma clang fp contract(off)
  __shared__ int sFine[kNormBlock];
  const int t = threadIdx.x, D = A.D, K = A.K;
  const int local = t / D, d = t - local * D;
  const long long N = A.N, l = (long long)blockIdx.x * A.lanes_per_block + local;
  const bool owns = local < A.lanes_per_block && l < N;
  T a = T(0), b = T(0);
  int len = 0;
  if (owns) {
    len = norm_len(A.length, l, K);
    const T c = norm_pivot<T>(A, l % A.P, d);
    const long long col = l * D + d, ND = N * D;
    auto apply = [&](T x) {
      const T dk = x - c;
      a = a + dk;
      b = b + dk * dk;
    };
    int n = len;                                        // the rows 0 .. n - 1 of obs, behind obs0 where it is given
    if (A.obs0 && len > 0) {
      apply(A.obs0[col]);
      n = len - 1;
    }
    const T* const src = A.obs + col;
    int k = 0;
    for (; k + kNormSteps <= n; k += kNormSteps) {
      T x[kNormSteps];
#pragma unroll
      for (int i = 0; i < kNormSteps; ++i) x[i] = src[(long long)(k + i) * ND];
#pragma unroll
      for (int i = 0; i < kNormSteps; ++i) apply(x[i]);
    }
    for (; k + kNormTail <= n; k += kNormTail) {
      T x[kNormTail];
#pragma unroll
      for (int i = 0; i < kNormTail; ++i) x[i] = src[(long long)(k + i) * ND];
#pragma unroll
      for (int i = 0; i < kNormTail; ++i) apply(x[i]);
    }
    for (; k < n; ++k) apply(src[(long long)k * ND]);
    A.lane_sum[(long long)d * N + l] = a;
    A.lane_sum[(long long)(D + d) * N + l] = b;
  }
  sFine[t] = (steer_finite(a) && steer_finite(b)) ? 1 : 0;    // (a thread that owns no column holds zeros)
  __syncthreads();                                      // every thread of the workgroup reaches it
  if (owns && d == 0) {
    int fine = 1;
    for (int i = 0; i < D; ++i) fine &= sFine[t + i];
    A.lane_count[l] = len;
    A.lane_count[N + l] = fine;
  }
}

// step 4, by the one thread that holds the totals of component d of policy p
template <typename T>
__device__ __forceinline__ void norm_merge(const StatsArgs<T>& A, long long p, int d, T At, T Bt, int nb, int nv) {
#pragma clang fp contract(off)
  const long long held = A.count_in ? A.count_in[p] : 0, na = held > 0 ? held : 0;
  const long long at = p * A.D + d;
  T mean = na > 0 ? A.mean_in[at] : T(0), m2 = na > 0 ? A.m2_in[at] : T(0);
  long long count = na;
  if (nb > 0) {
    const T nbT = (T)nb;
    const T off = At / nbT;
    const T prod = At * off;
    const T diff = Bt - prod;
    const T m2b = diff < T(0) ? T(0) : diff;
    if (na == 0) {
      const T c = norm_pivot<T>(A, p, d);
      mean = c + off;
      m2 = m2b;
      count = nb;
    } else {
      const T naT = (T)na, ntT = (T)(na + nb);
      const T w = nbT / ntT;
      const T shift = off * w;
      const T both = m2 + m2b;
      const T sq = off * off;
      const T scale = naT * w;
      const T cross = sq * scale;
      mean = mean + shift;
      m2 = both + cross;
      count = na + nb;
    }
  }
  A.mean_out[at] = mean;
  A.m2_out[at] = m2;
  if (d == 0) {
    A.count_out[p] = count;
    if (A.steps) A.steps[p] = nb;
    if (A.valid) A.valid[p] = nv;
  }
}

// A partial is a chain of S / 64 dependent additions, and at one policy there are only D workgroups: the four sums of a (policy,
// component) are a wave each, side by side, and meet in LDS (one after the other in one wave, (1, 65536, 50) took 0.29 ms, of
// which the lane launch is 0.05).
template <typename T>
__global__ __launch_bounds__(kNormSumWaves * kPgChunks) void norm_sum_kernel(const StatsArgs<T> A) {
#pragma clang fp contract(off)
  __shared__ T sB;
  __shared__ int sCount[2];
  const long long p = blockIdx.x, N = A.N;
  const int d = (int)blockIdx.y, wave = threadIdx.x / kPgChunks, c = threadIdx.x % kPgChunks;
  const int* const fine = A.lane_count + N;
  T At = T(0);
  if (wave == 0) {                                      // (uniform over a wave, here and below)
    At = pg_wave_sum<T>(A.lane_sum + (long long)d * N, fine, A.P, p, A.S, c);
  } else if (wave == 1) {
    const T Bt = pg_wave_sum<T>(A.lane_sum + (long long)(A.D + d) * N, fine, A.P, p, A.S, c);
    if (c == 0) sB = Bt;
  } else if (wave == 2) {
    const int nb = pg_wave_sum<int>(A.lane_count, fine, A.P, p, A.S, c);
    if (c == 0) sCount[0] = nb;
  } else {
    int nv = 0;
    if (d == 0 && A.valid) nv = pg_wave_sum<int>(fine, fine, A.P, p, A.S, c);
    if (c == 0) sCount[1] = nv;
  }
  __syncthreads();
  if (threadIdx.x == 0) norm_merge<T>(A, p, d, At, sB, sCount[0], sCount[1]);
}

// S <= 64: partial c is the term of sample c, or 0.  pg_few_sum holds the 64 partials of ONE sum in registers, which is right for a
// thread that forms one total; the merge needs two totals in one thread, and two or three of those bodies side by side came to
// 390 registers and 134 spilled SGPRs in fp64.  So, as in os2r_es.hpp, the same tree is formed as the partials arrive: level b
// holds the sum of a finished block of 2^b partials until its right neighbour is finished; `c` is uniform, the levels are indexed
// at compile time, and after the push of c = 63 the total is returned.  The integer sums have no order.
template <typename U>
__device__ __forceinline__ U norm_push(U (&level)[kNormLevels], U v, int c) {
#pragma clang fp contract(off)
  bool carry = true;
#pragma unroll
  for (int b = 0; b < kNormLevels; ++b) {
    const bool bit = ((c >> b) & 1) != 0;
    const U merged = level[b] + v;
    level[b] = (carry && !bit) ? v : level[b];
    v = (carry && bit) ? merged : v;
    carry = carry && bit;
  }
  return v;
}

template <typename T>
__global__ __launch_bounds__(kNormBlock) void norm_sum_few_kernel(const StatsArgs<T> A) {
#pragma clang fp contract(off)
  const long long p = (long long)blockIdx.x * kNormBlock + threadIdx.x, N = A.N;
  if (p >= A.P) return;
  const int d = (int)blockIdx.y, S = A.S;
  const int* const fine = A.lane_count + N;
  const T* const sum_a = A.lane_sum + (long long)d * N;
  const T* const sum_b = A.lane_sum + (long long)(A.D + d) * N;
  T la[kNormLevels], lb[kNormLevels];
#pragma unroll
  for (int b = 0; b < kNormLevels; ++b) la[b] = lb[b] = T(0);
  T At = T(0), Bt = T(0);
  int nb = 0, nv = 0;
#pragma unroll 4
  for (int c = 0; c < kPgChunks; ++c) {                  // (the loads of four samples depend on no partial and go out together)
    T a = T(0), b = T(0);
    if (c < S) {                                        // uniform
      const long long l = (long long)c * A.P + p;
      const int f = fine[l], n = A.lane_count[l];
      const T xa = sum_a[l], xb = sum_b[l];
      a = f != 0 ? xa : T(0);
      b = f != 0 ? xb : T(0);
      nb += f != 0 ? n : 0;
      nv += f != 0 ? 1 : 0;
    }
    At = norm_push<T>(la, a, c);
    Bt = norm_push<T>(lb, b, c);
  }
  norm_merge<T>(A, p, d, At, Bt, nb, nv);
}

// one correctly rounded IEEE square root (the builtin gets the fix-up sequence in fp32)
__device__ __forceinline__ float norm_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double norm_sqrt(double x) { return __builtin_sqrt(x); }

template <typename T>
__global__ __launch_bounds__(kNormBlock) void norm_fold_kernel(const FoldArgs<T> A) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * kNormBlock + threadIdx.x, Q = A.Q;
  if (t >= Q * A.rows) return;
  const int D = A.D, n = D + 1;
  // entry i of row j of set q stands at first + i * step
  const long long q = A.fastest ? t % Q : t / A.rows;
  const int j = (int)(A.fastest ? t / Q : t % A.rows);
  const long long first = A.fastest ? (long long)j * n * Q + q : (q * A.rows + j) * n, step = A.fastest ? Q : 1;
  const long long p = q % A.P;
  const long long count = A.count ? A.count[p] : 0;
  if (count < 2) {                                      // the identity: copied through
    for (int i = 0; i < n; ++i) A.out[first + i * step] = A.in[first + i * step];
    return;
  }
  const T cT = (T)count, last = A.in[first + D * step];
  T s = T(0);
  for (int d = 0; d < D; ++d) {
    const T mu = A.mean[p * D + d];
    const T v = A.m2[p * D + d] / cT;
    T sd = norm_sqrt(v);
    sd = sd < A.floor ? A.floor : sd;
    const T r = T(1) / sd;
    const T x = A.in[first + d * step];
    if (A.unfold) {
      const T prod = last * mu;
      const T diff = x - prod;
      A.out[first + d * step] = diff * r;
    } else {
      const T W = x * r;
      const T prod = W * mu;
      s = d == 0 ? prod : s + prod;
      A.out[first + d * step] = W;
    }
  }
  A.out[first + D * step] = A.unfold ? last : last - s;
}

// the launches of the three calls (os2r_norm_inst.hip, once per dtype)
template <typename T>
void launch_obs_stats(const StatsArgs<T>& args, hipStream_t stream);
template <typename T>
void launch_norm_fold(const FoldArgs<T>& args, hipStream_t stream);

}  // namespace os2r
