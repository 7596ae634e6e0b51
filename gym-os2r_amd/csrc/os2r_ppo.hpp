// os2r_ppo.hpp — os2ro_ppo_gradient: the gradient of the clipped surrogate of many linear-Gaussian policies in two stream-ordered
// launches (gfx950); the sums over the samples of a policy are the bodies of os2r_pg.hpp as they are.
//
// ppo_lane_kernel, grid ceil(8 N / 256).  The split of a lane is policy_gradient_lane_kernel's: thread 8 l + 4 j + h owns row j
// (the motor) and, of its columns, group h -- columns 3 h .. 3 h + 2 below D; the thread of group 0 also owns the row's bias sum,
// its V and its clip count, the thread (0, 0) the lane's three stat sums and its gated count.  Before the walk every thread
// forms the weight difference of its three columns and of the bias, and r_j.  In a step the mean shift of row j is a dot
// product over the row's four threads: each forms q_h of its columns, an xor butterfly over the column-group bits (1, 2) leaves
// ((q_0 + q_1) + (q_2 + q_3)) in all four (an addition commutes, so both sides of an exchange hold the same bits); t_j and r'_j of
// the other row come over the row bit (4).  What follows -- h, rho, the gate, the stats -- every one of the eight forms for
// itself.  The shuffles stay among the eight threads of one lane: they share len, so they run the same trip count; neighbouring
// lanes of a wave do not.  The walk runs from len - 1 down to 0, kPpoSteps steps to a round, the loads of a round issued before
// the first is used.  The thread (0, 0) writes ratio where k < len, the thread (1, 3) the zeros behind it.
//
// The second launch sums over the samples of every policy (step 16 of include/os2r_ppo.h) and reads nothing but what the first
// wrote; ppo_sum_kernel (S > 64, a wave per total) and ppo_sum_few_kernel (S <= 64, a thread per total) are pg_wave_sum and
// pg_few_sum over this library's own entry table, with the lane's verdict in row 4 of lane_count.
// No lane indexes a register array at run time, nothing goes to LDS or scratch (tests/test_ppo_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_ppo.h: the layout's dtype, no contraction, every chain in the order given
// there; the comparisons of the gate are made on bit patterns (the libraries are built without NaNs and infinities in the
// compiler's mind: os2r_bits.hpp).  tests/test_ppo_host.py restates it in numpy; tests/test_gpu_ppo.py compares bit for bit.
#pragma once
#include "os2r_pg.hpp"
#include "../../include/os2r_ppo.h"

namespace os2r {

// Steps of one round, of the pairs measured (profiles/ppo_rate.txt): beside what policy_gradient_lane_kernel holds a thread
// keeps four weight differences, r, the new width, both bounds and three more chains.
constexpr int kPpoSteps = 4;
constexpr int kPpoIntegerSums = OS2RO_LANE_COUNTS;   // steps, clip_0, clip_1, gated, valid: the rows of lane_count
constexpr int kPpoStats = OS2RO_STATS;               // surr, dev, logr
static_assert(OS2RO_CHUNKS == kPgChunks && kPgGroups == 4 && kPgThreads == 8, "the sums and the split of a lane are os2r_pg.hpp's");

template <typename T>
struct PpoArgs {
  const T* __restrict__ obs;          // [K][N][D]
  const T* __restrict__ obs0;         // [N][D] or null
  const T* __restrict__ noise;        // [K][N][2]
  const T* __restrict__ action;       // [K][N][2]; not read with tanh
  const T* __restrict__ sigma;        // [2], or [2][N] with sigma_per_lane
  const T* __restrict__ sigma_new;    // [2][P] or null
  const T* __restrict__ weight;       // [2][D+1][P]
  const T* __restrict__ weight_old;   // [2][D+1][P]
  const int* __restrict__ length;     // [N] or null
  const T* __restrict__ adv;          // [K][N]
  T* grad;                            // [2][D+1][P]
  T* lane_grad;                       // [2][D+1][N]: written by the first launch, read by the second
  T* lsig_grad;                       // [2][P] or null
  T* lane_lsig;                       // [2][N] or null, as lane_grad
  T* stat;                            // [3][P] or null
  T* lane_stat;                       // [3][N], as lane_grad
  int* steps;                         // [P] or null
  int* clipped;                       // [2][P] or null
  int* gated;                         // [P] or null
  int* valid;                         // [P] or null
  T* __restrict__ ratio;              // [K][N] or null
  int* lane_count;                    // [5][N]: len, clip_0, clip_1, gated, valid; as lane_grad
  long long P, N;
  int K, S, D, tanh, sigma_per_lane;
  T lo, hi;                           // 1 - clip and 1 + clip, formed in double and rounded to T by the host
};

__device__ __forceinline__ double ppo_exp(double x) { return ::exp(x); }
__device__ __forceinline__ float ppo_exp(float x) { return ::expf(x); }

// a < 0 (a NaN and a zero are not), and the two comparisons of the gate against a bound b > 0 that is finite, all on the bit
// patterns: the bits of the non-negative numbers and +inf compare as the values do, a NaN's magnitude lies above that of inf
__device__ __forceinline__ bool ppo_negative(float a) { return steer_bits(a) - 0x80000001u < 0x7f800000u; }
__device__ __forceinline__ bool ppo_negative(double a) { return steer_bits(a) - 0x8000000000000001ull < 0x7ff0000000000000ull; }
__device__ __forceinline__ bool ppo_above(float a, float b) {
  const unsigned x = steer_bits(a);
  return x > steer_bits(b) && x <= 0x7f800000u;
}
__device__ __forceinline__ bool ppo_above(double a, double b) {
  const unsigned long long x = steer_bits(a);
  return x > steer_bits(b) && x <= 0x7ff0000000000000ull;
}
__device__ __forceinline__ bool ppo_below(float a, float b) {
  const unsigned x = steer_bits(a);
  return x < steer_bits(b) || (x >= 0x80000000u && x <= 0xff800000u);
}
__device__ __forceinline__ bool ppo_below(double a, double b) {
  const unsigned long long x = steer_bits(a);
  return x < steer_bits(b) || (x >= 0x8000000000000000ull && x <= 0xfff0000000000000ull);
}

// what one thread reads of one step
template <typename T>
struct PpoStep {
  T x[kPgCols];
  T eps, a, psi;
  long long at;     // k N + l
};

template <typename T>
__global__ __launch_bounds__(kPgBlock) void ppo_lane_kernel(const PpoArgs<T> A) {
#pragma clang fp contract(off)
  const long long gid = (long long)blockIdx.x * kPgBlock + threadIdx.x;
  const long long N = A.N, l = gid / kPgThreads;
  if (l >= N) return;                                   // (whole lanes: 256 and 8 N are multiples of 8)
  const int h = (int)(gid % kPgGroups), j = (int)(gid / kPgGroups) & 1;
  const int K = A.K, D = A.D, d0 = h * kPgCols;
  const long long P = A.P, p = l % P;
  const bool tanh = A.tanh != 0;
  int len = A.length ? A.length[l] : K;
  len = len < 0 ? 0 : (len > K ? K : len);
  const T sig = A.sigma[A.sigma_per_lane ? (long long)j * N + l : (long long)j];
  const T snew = A.sigma_new ? A.sigma_new[(long long)j * P + p] : sig;
  const T r = A.sigma_new ? sig / snew : T(1);
  const bool enabled = pg_positive(sig) && pg_positive(snew);
  const T lo = A.lo, hi = A.hi;
  const long long wrow = (long long)j * (D + 1) * P + p;
  T dW[kPgCols];
#pragma unroll
  for (int i = 0; i < kPgCols; ++i)
    dW[i] = d0 + i < D ? A.weight[wrow + (long long)(d0 + i) * P] - A.weight_old[wrow + (long long)(d0 + i) * P] : T(0);
  const T dWb = A.weight[wrow + (long long)D * P] - A.weight_old[wrow + (long long)D * P];
  T* const ratio = (j == 0 && h == 0) ? A.ratio : nullptr;

  auto load = [&](int k) {
    PpoStep<T> s;
    s.at = (long long)k * N + l;
    const T* const x = A.obs0 ? (k ? A.obs + ((long long)(k - 1) * N + l) * D : A.obs0 + l * D) : A.obs + s.at * D;
#pragma unroll
    for (int i = 0; i < kPgCols; ++i) s.x[i] = d0 + i < D ? x[d0 + i] : T(0);
    s.eps = A.noise[s.at * 2 + j];
    s.a = tanh ? T(0) : A.action[s.at * 2 + j];
    s.psi = A.adv[s.at];
    return s;
  };

  T acc[kPgCols];
#pragma unroll
  for (int i = 0; i < kPgCols; ++i) acc[i] = T(0);
  T bias = T(0), V = T(0), surr = T(0), dev = T(0), logr = T(0);
  int clip = 0, gated = 0;
  auto apply = [&](const PpoStep<T>& s) {
    const T psi = s.psi;
    const bool a_open = tanh || pg_below_one(s.a);      // step 2
    clip += a_open ? 0 : 1;
    const bool open = enabled && a_open;
    T q = T(0);                                         // step 3: q_h, then the row's four over the column-group bits
#pragma unroll
    for (int i = 0; i < kPgCols; ++i) q = q + dW[i] * s.x[i];
    q = q + __shfl_xor(q, 1);
    q = q + __shfl_xor(q, 2);
    const T dmu = q + dWb;
    const T z = (s.eps - dmu / sig) * r;                // steps 4 and 5
    const T zz = z * z;
    const T t = open ? s.eps * s.eps - zz : T(0);
    const T rp = open ? r : T(1);
    const T half = T(0.5) * (t + __shfl_xor(t, 4));     // steps 6 and 7
    const T rho = ppo_exp(half) * (rp * __shfl_xor(rp, 4));
    if (ratio) ratio[s.at] = rho;
    const bool up = pg_positive(psi) && ppo_above(rho, hi);      // step 10
    const bool down = ppo_negative(psi) && ppo_below(rho, lo);
    gated += (up || down) ? 1 : 0;
    surr = surr + (up ? psi * hi : (down ? psi * lo : rho * psi));   // steps 11 to 13
    dev = dev + (rho - T(1));
    logr = logr + half;
    if (open && !(up || down)) {                        // step 14 (every thread forms bias and V; those of group 0 are tested and stored)
      const T w = psi * rho;
      const T e = z / snew;
      const T c = w * e;
#pragma unroll
      for (int i = 0; i < kPgCols; ++i) acc[i] = acc[i] + c * s.x[i];
      bias = bias + c;
      V = V + w * (zz - T(1));
    }
  };
  int k = len - 1;
  for (; k >= kPpoSteps - 1; k -= kPpoSteps) {
    PpoStep<T> s[kPpoSteps];
#pragma unroll
    for (int i = 0; i < kPpoSteps; ++i) s[i] = load(k - i);
#pragma unroll
    for (int i = 0; i < kPpoSteps; ++i) apply(s[i]);
  }
  for (; k >= 0; --k) apply(load(k));
  if (A.ratio && j == 1 && h == kPgGroups - 1)
    for (int z = len; z < K; ++z) A.ratio[(long long)z * N + l] = T(0);

  // step 15: the columns this thread owns (a column at or above D saw zeros only, and is not asked), with group 0 the row's bias and
  // V, with the thread (0, 0) the three stats
  int fine = 1;
#pragma unroll
  for (int i = 0; i < kPgCols; ++i) fine &= (d0 + i >= D || steer_finite(acc[i])) ? 1 : 0;
  if (h == 0) fine &= (steer_finite(bias) && steer_finite(V)) ? 1 : 0;
  if (h == 0 && j == 0) fine &= (steer_finite(surr) && steer_finite(dev) && steer_finite(logr)) ? 1 : 0;
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
      A.lane_stat[l] = surr;
      A.lane_stat[N + l] = dev;
      A.lane_stat[2 * N + l] = logr;
      A.lane_count[l] = len;
      A.lane_count[3 * N + l] = gated;
      A.lane_count[4 * N + l] = fine;
    }
  }
}

// Entry e of the sums of step 16 -> where its per-lane terms stand and where the policies' totals go: the 2 (D + 1) elements of
// grad, the two of lsig_grad, the three of stat, then steps, clipped[0], clipped[1], gated and valid.  False: the total is not wanted.
template <typename T>
__device__ __forceinline__ bool ppo_entry(const PpoArgs<T>& A, int e, PgEntry<T>& out) {
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
  if (e < F + 2 + kPpoStats) {
    if (!A.stat) return false;
    out.terms = A.lane_stat + (long long)(e - (F + 2)) * A.N;
    out.totals = A.stat + (long long)(e - (F + 2)) * A.P;
    return true;
  }
  const int row = e - (F + 2 + kPpoStats);              // of lane_count
  int* const totals = row == 0 ? A.steps : (row == 3 ? A.gated : (row == 4 ? A.valid : (A.clipped ? A.clipped + (long long)(row - 1) * A.P : nullptr)));
  if (!totals) return false;
  out.counts = A.lane_count + (long long)row * A.N;
  out.count_totals = totals;
  return true;
}

template <typename T>
__global__ __launch_bounds__(kPgChunks) void ppo_sum_kernel(const PpoArgs<T> A) {
#pragma clang fp contract(off)
  PgEntry<T> E;
  if (!ppo_entry(A, (int)blockIdx.y, E)) return;        // uniform over the workgroup
  const long long p = blockIdx.x;
  const int c = threadIdx.x;
  const int* const fine = A.lane_count + (kPpoIntegerSums - 1) * A.N;
  if (E.terms) {
    const T total = pg_wave_sum<T>(E.terms, fine, A.P, p, A.S, c);
    if (c == 0) E.totals[p] = total;
  } else {
    const int total = pg_wave_sum<int>(E.counts, fine, A.P, p, A.S, c);
    if (c == 0) E.count_totals[p] = total;
  }
}

template <typename T>
__global__ __launch_bounds__(kPgBlock) void ppo_sum_few_kernel(const PpoArgs<T> A) {
#pragma clang fp contract(off)
  PgEntry<T> E;
  if (!ppo_entry(A, (int)blockIdx.y, E)) return;
  const long long p = (long long)blockIdx.x * kPgBlock + threadIdx.x;
  if (p >= A.P) return;
  const int* const fine = A.lane_count + (kPpoIntegerSums - 1) * A.N;
  if (E.terms)
    E.totals[p] = pg_few_sum<T>(E.terms, fine, A.P, p, A.S);
  else
    E.count_totals[p] = pg_few_sum<int>(E.counts, fine, A.P, p, A.S);
}

// the two launches (os2r_ppo_inst.hip, once per dtype)
template <typename T>
void launch_ppo_gradient(const PpoArgs<T>& args, hipStream_t stream);

}  // namespace os2r
