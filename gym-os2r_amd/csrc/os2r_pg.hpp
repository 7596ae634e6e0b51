// os2r_pg.hpp — os2rg_policy_gradient: the score-function gradient of many linear-Gaussian policies in two stream-ordered
// launches (gfx950).
//
// policy_gradient_lane_kernel, grid ceil(8 N / 256).  Each of a lane's 2 (D + 1) + 2 sums is a chain of its own over the steps
// (include/os2r_pg.h, steps 1 to 4), so a lane is shared among kPgThreads = 8 neighbouring threads: thread 8 l + 4 j + h owns row j
// (the motor) and, of its columns, group h -- columns 3 h .. 3 h + 2 below D; the thread of group 0 also owns the row's bias sum, its
// V and its clip count.  At N = 8 192 that is 1 024 waves where a thread per lane would be 128.  What the eight share (the reward-
// to-go chain, psi, the quotient eps / sigma) every one of them forms for itself: a few operations against eight times the waves.
// The walk runs from len - 1 down to 0, four steps to a round: the loads of a round depend on no accumulator, so all of them
// are issued before the first is used.  obs is [K][N][D] with D fastest: the eight read the lane's D values, the wave one
// contiguous span per step.  A lane is valid iff every one of its threads found its sums finite: three xor shuffles inside the
// wave (the eight never straddle one).  The thread (j, h) = (0, 0) writes rtg where k < len, the thread (1, 3) the zeros behind it.
//
// The second launch sums over the samples of every policy (step 5) and reads nothing but what the first wrote: lane_grad,
// lane_lsig and lane_count, whose fourth row is the lane's verdict.  One entry of one policy -- an element of grad or lsig_grad,
// or one of the four integer sums -- is one chain of 64 partials and a tree:
//   policy_gradient_sum_kernel (S > 64), grid (P, entries), one wave each: lane c of the wave is partial c and adds its samples
//     s = c, c + 64, ... in ascending order; the xor butterfly over 1, 2, 4, .. 32 leaves the adjacent-pair tree in lane 0.  With
//     P = 1 the 64 lanes read 64 neighbouring values a round
//   policy_gradient_sum_few_kernel (S <= 64), grid (ceil(P / 256), entries), one thread each: partial c is the term of sample c
//     (or 0), all 64 are loaded at once -- the threads of a wave read neighbouring policies -- and the tree is formed in registers
// No lane indexes a register array at run time, nothing goes to scratch (tests/test_pg_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_pg.h: the layout's dtype, no contraction, every chain in the order given there.
// tests/test_pg_host.py restates it in numpy; tests/test_gpu_pg.py compares bit for bit.
#pragma once
#include "os2r_bits.hpp"
#include "../../include/os2r_pg.h"

namespace os2r {

// Four column groups and four steps to a round, of the five pairs measured (profiles/pg_rate.txt): at one policy, 8 192 samples
// and 500 steps in fp64 2 x 4 took 0.284 ms, 4 x 4 0.227 ms, 4 x 8 0.208 ms -- but 4 x 8 and 4 x 12 need 260 and 372 registers, one
// wave to a SIMD, and lost up to a factor two wherever there are lanes enough to fill the chip.
constexpr int kPgGroups = 4;                     // column groups of one row: a thread each
constexpr int kPgSteps = 4;                      // steps of one round: their loads are in flight together
constexpr int kPgThreads = 2 * kPgGroups;           // threads of one lane: 2 rows x the column groups
constexpr int kPgCols = OS2R_MAX_OBS / kPgGroups;   // columns of one thread
constexpr int kPgBlock = 256;                    // threads of a workgroup of the lane kernel and of the few-samples sum
constexpr int kPgChunks = OS2RG_CHUNKS;          // partials of a sum over the samples: the lanes of one wave
constexpr int kPgIntegerSums = 4;                // steps, clip_0, clip_1, valid: the rows of lane_count
static_assert(kPgChunks == 64, "a partial is a lane of a wave");
static_assert(kPgGroups * kPgCols == OS2R_MAX_OBS && 64 % kPgThreads == 0, "the groups hold every column, a wave whole lanes");

template <typename T>
struct PgArgs {
  const T* __restrict__ obs;          // [K][N][D]
  const T* __restrict__ obs0;         // [N][D] or null
  const T* __restrict__ noise;        // [K][N][2]
  const T* __restrict__ action;       // [K][N][2]; not read with tanh
  const T* __restrict__ sigma;        // [2], or [2][N] with sigma_per_lane
  const int* __restrict__ length;     // [N] or null
  const T* __restrict__ adv;          // [N], or null with reward
  const T* __restrict__ reward;       // [K][N], or null with adv
  const unsigned char* __restrict__ done;   // [K][N], with reward
  const T* __restrict__ baseline;     // [K][P] or null
  T* grad;                            // [2][D+1][P]
  T* lane_grad;                       // [2][D+1][N]: written by the first launch, read by the second
  T* lsig_grad;                       // [2][P] or null
  T* lane_lsig;                       // [2][N] or null, as lane_grad
  int* steps;                         // [P] or null
  int* clipped;                       // [2][P] or null
  int* valid;                         // [P] or null
  T* __restrict__ rtg;                // [K][N] or null
  int* lane_count;                    // [4][N]: len, clip_0, clip_1, valid; as lane_grad
  long long P, N;
  int K, S, D, tanh, sigma_per_lane;
  T gamma;                            // rounded to T by the host
};

// |a| < 1 and s > 0 on the bit patterns (os2r_bits.hpp says why): the magnitude's bits compare as the magnitude does, and a NaN's
// lie above those of every number; the bits of a positive number or +inf lie in 1 .. the bits of +inf
__device__ __forceinline__ bool pg_below_one(float a) { return (steer_bits(a) & 0x7fffffffu) < 0x3f800000u; }
__device__ __forceinline__ bool pg_below_one(double a) { return (steer_bits(a) & 0x7fffffffffffffffull) < 0x3ff0000000000000ull; }
__device__ __forceinline__ bool pg_positive(float s) { return steer_bits(s) - 1u < 0x7f800000u; }
__device__ __forceinline__ bool pg_positive(double s) { return steer_bits(s) - 1ull < 0x7ff0000000000000ull; }

// what one thread reads of one step
template <typename T>
struct PgStep {
  T x[kPgCols];
  T eps, a, r, b;
  unsigned done;
  long long at;     // k N + l
};

template <typename T>
__global__ __launch_bounds__(kPgBlock) void policy_gradient_lane_kernel(const PgArgs<T> A) {
#pragma clang fp contract(off)
  const long long gid = (long long)blockIdx.x * kPgBlock + threadIdx.x;
  const long long N = A.N, l = gid / kPgThreads;
  if (l >= N) return;                                   // (whole lanes: 256 and 8 N are multiples of 8)
  const int h = (int)(gid % kPgGroups), j = (int)(gid / kPgGroups) & 1;
  const int K = A.K, D = A.D, d0 = h * kPgCols;
  const long long p = l % A.P;
  const bool rewards = A.reward != nullptr, tanh = A.tanh != 0;
  int len = A.length ? A.length[l] : K;
  len = len < 0 ? 0 : (len > K ? K : len);
  const T sig = A.sigma[A.sigma_per_lane ? (long long)j * N + l : (long long)j];
  const bool sig_open = pg_positive(sig);
  const T adv = rewards ? T(0) : A.adv[l];
  const T gamma = A.gamma;
  T* const rtg = (j == 0 && h == 0) ? A.rtg : nullptr;

  auto load = [&](int k) {
    PgStep<T> s;
    s.at = (long long)k * N + l;
    const T* const x = A.obs0 ? (k ? A.obs + ((long long)(k - 1) * N + l) * D : A.obs0 + l * D) : A.obs + s.at * D;
#pragma unroll
    for (int i = 0; i < kPgCols; ++i) s.x[i] = d0 + i < D ? x[d0 + i] : T(0);
    s.eps = A.noise[s.at * 2 + j];
    s.a = tanh ? T(0) : A.action[s.at * 2 + j];
    s.r = rewards ? A.reward[s.at] : T(0);
    s.done = rewards ? (unsigned)A.done[s.at] : 0u;
    s.b = A.baseline ? A.baseline[(long long)k * A.P + p] : T(0);
    return s;
  };

  T acc[kPgCols];
#pragma unroll
  for (int i = 0; i < kPgCols; ++i) acc[i] = T(0);
  T bias = T(0), V = T(0), G = T(0);
  int clip = 0;
  auto apply = [&](const PgStep<T>& s) {
    T psi = adv;
    if (rewards) {                                      // step 1
      G = s.done != 0u ? s.r : s.r + gamma * G;
      psi = A.baseline ? G - s.b : G;
      if (rtg) rtg[s.at] = G;
    }
    const bool a_open = tanh || pg_below_one(s.a);      // step 2
    clip += a_open ? 0 : 1;
    if (sig_open && a_open) {                           // step 3 (every thread forms bias and V; those of group 0 are tested and stored)
      const T e = s.eps / sig;
      const T c = psi * e;
#pragma unroll
      for (int i = 0; i < kPgCols; ++i) acc[i] = acc[i] + c * s.x[i];
      bias = bias + c;
      V = V + psi * (s.eps * s.eps - T(1));
    }
  };
  int k = len - 1;
  for (; k >= kPgSteps - 1; k -= kPgSteps) {
    PgStep<T> s[kPgSteps];
#pragma unroll
    for (int i = 0; i < kPgSteps; ++i) s[i] = load(k - i);
#pragma unroll
    for (int i = 0; i < kPgSteps; ++i) apply(s[i]);
  }
  for (; k >= 0; --k) apply(load(k));
  if (A.rtg && j == 1 && h == kPgGroups - 1)
    for (int z = len; z < K; ++z) A.rtg[(long long)z * N + l] = T(0);

  // step 4: the columns this thread owns (a column at or above D saw zeros only, and is not asked), with group 0 the row's bias and V
  int fine = 1;
#pragma unroll
  for (int i = 0; i < kPgCols; ++i) fine &= (d0 + i >= D || steer_finite(acc[i])) ? 1 : 0;
  if (h == 0) fine &= (steer_finite(bias) && steer_finite(V)) ? 1 : 0;
#pragma unroll
  for (int m = 1; m < kPgThreads; m *= 2) fine &= __shfl_xor(fine, m);

  T* const row = A.lane_grad + (long long)j * (D + 1) * N + l;
#pragma unroll
  for (int i = 0; i < kPgCols; ++i)
    if (d0 + i < D) row[(long long)(d0 + i) * N] = acc[i];
  if (h == 0) {
    row[(long long)D * N] = bias;
    if (A.lane_lsig) A.lane_lsig[(long long)j * N + l] = V;
    A.lane_count[(long long)(1 + j) * N + l] = clip;
    if (j == 0) {
      A.lane_count[l] = len;
      A.lane_count[3 * N + l] = fine;
    }
  }
}

// Entry e of the sums of step 5 -> where its per-lane terms stand and where the policies' totals go: the 2 (D + 1) elements of
// grad, the two of lsig_grad, then steps, clipped[0], clipped[1] and valid.  False: the total is not wanted.
template <typename T>
struct PgEntry {
  const T* terms;
  T* totals;
  const int* counts;
  int* count_totals;
};

template <typename T>
__device__ __forceinline__ bool pg_entry(const PgArgs<T>& A, int e, PgEntry<T>& out) {
  const int F = 2 * (A.D + 1);
  out.terms = nullptr; out.totals = nullptr; out.counts = nullptr; out.count_totals = nullptr;
  if (e < F) {
    out.terms = A.lane_grad + (long long)e * A.N;
    out.totals = A.grad + (long long)e * A.P;
    return true;
  }
  if (e < F + 2) {
    if (!A.lsig_grad) return false;
    out.terms = A.lane_lsig + (long long)(e - F) * A.N;
    out.totals = A.lsig_grad + (long long)(e - F) * A.P;
    return true;
  }
  const int row = e - (F + 2);                          // of lane_count
  int* const totals = row == 0 ? A.steps : (row == 3 ? A.valid : (A.clipped ? A.clipped + (long long)(row - 1) * A.P : nullptr));
  if (!totals) return false;
  out.counts = A.lane_count + (long long)row * A.N;
  out.count_totals = totals;
  return true;
}

// partial c of policy p: the terms of its valid samples s = c, c + 64, ... in ascending order onto 0; then the tree, in lane 0
template <typename U>
__device__ __forceinline__ U pg_wave_sum(const U* __restrict__ terms, const int* __restrict__ fine, long long P, long long p, int S, int c) {
  U acc = U(0);
#pragma unroll 4
  for (int s = c; s < S; s += kPgChunks) {
    const long long l = (long long)s * P + p;
    const U x = terms[l];
    acc = fine[l] != 0 ? acc + x : acc;
  }
#pragma unroll
  for (int m = 1; m < kPgChunks; m *= 2) acc = acc + __shfl_xor(acc, m);
  return acc;
}

template <typename T>
__global__ __launch_bounds__(kPgChunks) void policy_gradient_sum_kernel(const PgArgs<T> A) {
#pragma clang fp contract(off)
  PgEntry<T> E;
  if (!pg_entry(A, (int)blockIdx.y, E)) return;         // uniform over the workgroup
  const long long p = blockIdx.x;
  const int c = threadIdx.x;
  const int* const fine = A.lane_count + 3 * A.N;
  if (E.terms) {
    const T total = pg_wave_sum<T>(E.terms, fine, A.P, p, A.S, c);
    if (c == 0) E.totals[p] = total;
  } else {
    const int total = pg_wave_sum<int>(E.counts, fine, A.P, p, A.S, c);
    if (c == 0) E.count_totals[p] = total;
  }
}

// S <= 64: partial c is the term of sample c, or 0; the tree in registers
template <typename U>
__device__ __forceinline__ U pg_few_sum(const U* __restrict__ terms, const int* __restrict__ fine, long long P, long long p, int S) {
  U v[kPgChunks];
#pragma unroll
  for (int c = 0; c < kPgChunks; ++c) {
    v[c] = U(0);
    if (c < S) {                                        // uniform
      const long long l = (long long)c * P + p;
      const U x = terms[l];
      v[c] = fine[l] != 0 ? x : U(0);
    }
  }
#pragma unroll
  for (int w = 1; w < kPgChunks; w *= 2)
#pragma unroll
    for (int i = 0; i < kPgChunks; i += 2 * w) v[i] = v[i] + v[i + w];
  return v[0];
}

template <typename T>
__global__ __launch_bounds__(kPgBlock) void policy_gradient_sum_few_kernel(const PgArgs<T> A) {
#pragma clang fp contract(off)
  PgEntry<T> E;
  if (!pg_entry(A, (int)blockIdx.y, E)) return;
  const long long p = (long long)blockIdx.x * kPgBlock + threadIdx.x;
  if (p >= A.P) return;
  const int* const fine = A.lane_count + 3 * A.N;
  if (E.terms)
    E.totals[p] = pg_few_sum<T>(E.terms, fine, A.P, p, A.S);
  else
    E.count_totals[p] = pg_few_sum<int>(E.counts, fine, A.P, p, A.S);
}

// the two launches (os2r_pg_inst.hip, once per dtype)
template <typename T>
void launch_policy_gradient(const PgArgs<T>& args, hipStream_t stream);

}  // namespace os2r
