// os2r_es.hpp — os2ra_es_perturb and os2ra_es_update: antithetic perturbations and the ARS V1-t update of many linear policies
// (gfx950).  The directions are never read: every kernel that needs delta[m][s] forms it from the counter RNG of os2r_device.hpp
// (normal2, stream OS2RA_STREAM), in double, rounded once to T.
//
// es_perturb_kernel, grid ceil(S M (D + 1) / 256).  A thread owns one Philox block q of one (m, s): the entries 2 q and 2 q + 1 of
// the policy.  Thread t is block t % (D + 1) of direction-population t / (D + 1) = s M + m, so the threads of a wave write one
// contiguous span of the plus lanes, one of the minus lanes and one of delta; theta, weights and delta go as aligned pairs.
// es_score_kernel, grid ceil(S M / 256), runs only where top selects: per (s, m) the order-preserving integer key of the score
// max(r+, r-) of a valid direction, 0 for an invalid one (no key of a finite value is 0).
// es_rank_kernel, grid (ceil(S M / 256), ceil(S / 1024)), only where top selects: the thread of (s, m) counts the directions of
// population m whose key is larger, or equal at a lower s, and keeps its own iff the count is below top.  The loads are four
// in flight; the threads of a wave read neighbouring populations (or, with M = 1, all the same word).  Above 1 024 directions
// the count is shared among the rows of the grid, a span of 1 024 directions each: their counts meet in kept[i] by integer
// atomics (es_score_kernel left a 0 there) and es_keep_kernel, grid ceil(S M / 256), decides.  The contract fixes the set, not
// the method: a count needs no LDS and no barrier, and costs S^2 M comparisons (DESIGN.md section 4 has what that comes to).
// es_sum_kernel (64 < S < 1024), grid (M, D + 1), one wave each: lane c of the wave is partial c of every sum of the population
// and regenerates the Philox block of its own directions s = c, c + 64, ...; the xor butterfly over 1, 2, 4, .. 32 leaves the
// adjacent-pair tree in every lane.  Two walks: the counts, the sum of the returns and the two direction sums; then, with the
// mean, the squared deviations.  Every wave of a population forms sigma_R for itself (D + 1 times two loads per direction against
// one launch less and no exchange); the wave of block 0 writes sigma_r, count, used and, where no top selects, kept.
// es_sum_wide_kernel (S >= 1024), grid (M, D + 1), sixteen waves each: the terms of a partial's chain are formed by all sixteen
// and handed to wave 0 through LDS (see there); the one kernel with LDS, 36 864 / 20 480 bytes (fp64 / fp32).
// es_sum_few_kernel (S <= 64), grid (ceil(M / 256), D + 1), one thread each: partial c is the term of direction c (or 0) and the
// tree is formed as the partials arrive, on a stack of six levels in registers (policy_gradient_sum_few_kernel holds all 64 of
// one sum; here a thread has four sums and a Philox block in flight).
// No lane indexes a register array at run time, nothing goes to scratch (tests/test_es_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_es.h: the layout's dtype, no contraction, every chain in the order given there.
// tests/test_es_host.py restates it in numpy; tests/test_gpu_es.py compares bit for bit.
#pragma once
#include "os2r_bits.hpp"
#include "os2r_device.hpp"
#include "../../include/os2r_es.h"

namespace os2r {

constexpr uint32_t kStreamEsDirection = OS2RA_STREAM;   // beside the five of os2r_device.hpp
constexpr int kEsChunks = OS2RA_CHUNKS;                  // partials of a sum over the directions: the lanes of one wave
constexpr int kEsLevels = 6;                             // of the adjacent-pair tree
constexpr int kEsBlock = 256;                            // threads of a workgroup of every kernel but the wave sums
constexpr int kEsWide = 1024;                            // threads of a workgroup of the wide sum: the directions of one round
constexpr int kEsRankSpan = 1024;                        // directions one workgroup of the rank launch counts against
static_assert(kEsChunks == 64 && (1 << kEsLevels) == kEsChunks && kEsWide % kEsChunks == 0, "a partial is a lane of a wave");
static_assert(kStreamEsDirection > kStreamPolicyNoise, "a stream of its own");

template <typename T>
struct EsArgs {
  const T* __restrict__ returns;      // [2 S M]
  const T* __restrict__ theta;        // [M][E]
  T* __restrict__ weights;            // [2 S M][E]  (perturb)
  T* __restrict__ delta;              // [S M][E] or null  (perturb)
  T* __restrict__ theta_out;          // [M][E]
  T* __restrict__ sigma_r;            // [M]
  int* __restrict__ count;            // [M]
  int* __restrict__ used;             // [M]
  T* __restrict__ grad;               // [M][E] or null
  int* kept;                          // [S M]; with `select` written by the rank launch and read by the sum launch
  void* score;                        // [S M] keys of the size of T, with `select`
  unsigned long long seed;
  long long M;
  uint32_t pop_offset, generation;
  int S, D, top, select;
  T nu, step_size, sigma_floor;       // rounded to T by the host
};

// two adjacent entries of a policy, read and written at once
template <typename T>
struct alignas(2 * sizeof(T)) EsPair {
  T a, b;
};

// the Philox block q of direction s of population m: entries 2 q and 2 q + 1 of delta[m][s], rounded once to T
template <typename T>
__device__ __forceinline__ EsPair<T> es_direction(const EsArgs<T>& A, long long m, int s, int q) {
  double z0, z1;
  normal2(A.seed, A.pop_offset + (uint32_t)m, kStreamEsDirection, A.generation, 16u * (uint32_t)s + (uint32_t)q, z0, z1);
  return EsPair<T>{(T)z0, (T)z1};
}

template <typename T>
__global__ __launch_bounds__(kEsBlock) void es_perturb_kernel(const EsArgs<T> A) {
#pragma clang fp contract(off)
  const int n = A.D + 1;
  const long long SM = (long long)A.S * A.M;
  const long long t = (long long)blockIdx.x * kEsBlock + threadIdx.x;
  if (t >= SM * n) return;
  const int q = (int)(t % n);
  const long long sm = t / n, m = sm % A.M;
  const int s = (int)(sm / A.M);
  const EsPair<T> d = es_direction<T>(A, m, s, q);
  const EsPair<T> th = reinterpret_cast<const EsPair<T>*>(A.theta)[m * n + q];
  const T p0 = A.nu * d.a, p1 = A.nu * d.b;
  EsPair<T>* const w = reinterpret_cast<EsPair<T>*>(A.weights);
  w[sm * n + q] = EsPair<T>{th.a + p0, th.b + p1};
  w[(SM + sm) * n + q] = EsPair<T>{th.a - p0, th.b - p1};
  if (A.delta) reinterpret_cast<EsPair<T>*>(A.delta)[sm * n + q] = d;
}

// The order-preserving key of a finite score: an unsigned integer that compares as the value does, -0 and +0 equal, never 0.
// Made of the bit pattern (os2r_bits.hpp says why).
__device__ __forceinline__ unsigned es_key(float r) {
  const unsigned b = steer_bits(r), z = b == 0x80000000u ? 0u : b;
  return (z >> 31) ? ~z : (z | 0x80000000u);
}
__device__ __forceinline__ unsigned long long es_key(double r) {
  const unsigned long long b = steer_bits(r), z = b == 0x8000000000000000ull ? 0ull : b;
  return (z >> 63) ? ~z : (z | 0x8000000000000000ull);
}

template <typename T>
__device__ __forceinline__ bool es_valid(T rp, T rm) { return steer_finite(rp) && steer_finite(rm); }

template <typename T>
__global__ __launch_bounds__(kEsBlock) void es_score_kernel(const EsArgs<T> A) {
  using U = decltype(es_key(T(0)));
  const long long SM = (long long)A.S * A.M;
  const long long i = (long long)blockIdx.x * kEsBlock + threadIdx.x;
  if (i >= SM) return;
  const T rp = A.returns[i], rm = A.returns[SM + i];
  const U kp = es_key(rp), km = es_key(rm);
  static_cast<U*>(A.score)[i] = es_valid(rp, rm) ? (kp > km ? kp : km) : U(0);
  if (A.S > kEsRankSpan) A.kept[i] = 0;                 // the rank launch adds the spans' counts up here
}

// grid (ceil(S M / 256), ceil(S / kEsRankSpan)): the workgroups of row y count against the directions of span y.  With one span
// the thread decides; with more the counts of a direction's spans meet in kept[i] by integer atomics (an integer sum has no
// order), and es_keep_kernel decides.
template <typename T>
__global__ __launch_bounds__(kEsBlock) void es_rank_kernel(const EsArgs<T> A) {
  using U = decltype(es_key(T(0)));
  const long long M = A.M, SM = (long long)A.S * M;
  const long long i = (long long)blockIdx.x * kEsBlock + threadIdx.x;
  if (i >= SM) return;
  const long long m = i % M;
  const int S = A.S, mine = (int)(i / M);
  const bool alone = S <= kEsRankSpan;
  const U* const key = static_cast<const U*>(A.score) + m;
  const U own = key[(long long)mine * M];
  if (own == U(0)) {                                    // an invalid direction: not kept, and ahead of none that is valid
    if (alone) A.kept[i] = 0;
    return;
  }
  int ahead = 0;
  auto tally = [&](U k, int s) { ahead += (k > own || (k == own && s < mine)) ? 1 : 0; };
  for (long long lo = (long long)blockIdx.y * kEsRankSpan; lo < S; lo += (long long)gridDim.y * kEsRankSpan) {   // (a grid has 65 535 rows at the most)
    const int hi = S - lo < kEsRankSpan ? S : (int)lo + kEsRankSpan;
    int s = (int)lo;
    for (; s + 3 < hi; s += 4) {                        // four loads are in flight together
      const U k0 = key[(long long)s * M], k1 = key[(long long)(s + 1) * M], k2 = key[(long long)(s + 2) * M], k3 = key[(long long)(s + 3) * M];
      tally(k0, s);
      tally(k1, s + 1);
      tally(k2, s + 2);
      tally(k3, s + 3);
    }
    for (; s < hi; ++s) tally(key[(long long)s * M], s);
  }
  if (alone)
    A.kept[i] = ahead < A.top ? 1 : 0;
  else if (ahead != 0)
    atomicAdd(&A.kept[i], ahead);
}

// more than one span: the count in kept[i] -> kept or not
template <typename T>
__global__ __launch_bounds__(kEsBlock) void es_keep_kernel(const EsArgs<T> A) {
  using U = decltype(es_key(T(0)));
  const long long i = (long long)blockIdx.x * kEsBlock + threadIdx.x;
  if (i >= (long long)A.S * A.M) return;
  A.kept[i] = (static_cast<const U*>(A.score)[i] != U(0) && A.kept[i] < A.top) ? 1 : 0;
}

// What one direction adds to the sums of its population's first walk.
template <typename T>
struct EsTerms {
  T ret;        // the chain of the returns: acc + r+ and then + r-
  T g0, g1;     // the two direction sums of this Philox block
  int valid, kept;
};

// the two returns of direction s of population m, and whether the direction is kept
template <typename T>
struct EsReturns {
  T rp, rm;
  bool valid, kept;
};

template <typename T>
__device__ __forceinline__ EsReturns<T> es_returns(const EsArgs<T>& A, long long m, int s) {
  const long long SM = (long long)A.S * A.M, i = (long long)s * A.M + m;
  EsReturns<T> r;
  r.rp = A.returns[i];
  r.rm = A.returns[SM + i];
  r.valid = es_valid(r.rp, r.rm);
  r.kept = A.select ? A.kept[i] != 0 : r.valid;
  return r;
}

// direction s of population m onto the counts and the chain of the returns of the partial `acc` (the first walk; a return that
// is not finite never touches a chain); where no top selects the wave or thread of block 0 writes kept
template <typename T>
__device__ __forceinline__ EsReturns<T> es_first(const EsArgs<T>& A, long long m, int s, int q, EsTerms<T>& acc) {
#pragma clang fp contract(off)
  const EsReturns<T> r = es_returns<T>(A, m, s);
  acc.valid += r.valid ? 1 : 0;
  acc.kept += r.kept ? 1 : 0;
  if (r.kept) {
    acc.ret = acc.ret + r.rp;
    acc.ret = acc.ret + r.rm;
  }
  if (!A.select && q == 0) A.kept[(long long)s * A.M + m] = r.valid ? 1 : 0;
  return r;
}

// the two terms of a kept direction for the direction sums of Philox block q
template <typename T>
__device__ __forceinline__ EsPair<T> es_products(const EsArgs<T>& A, long long m, int s, int q, const EsReturns<T>& r) {
#pragma clang fp contract(off)
  const EsPair<T> d = es_direction<T>(A, m, s, q);
  const T diff = r.rp - r.rm;
  return EsPair<T>{diff * d.a, diff * d.b};
}

// ... both onto the partial `acc`
template <typename T>
__device__ __forceinline__ void es_first_whole(const EsArgs<T>& A, long long m, int s, int q, EsTerms<T>& acc) {
#pragma clang fp contract(off)
  const EsReturns<T> r = es_first<T>(A, m, s, q, acc);
  if (r.kept) {
    const EsPair<T> p = es_products<T>(A, m, s, q, r);
    acc.g0 = acc.g0 + p.a;
    acc.g1 = acc.g1 + p.b;
  }
}

// ... and onto the partial of the squared deviations (the second walk)
template <typename T>
__device__ __forceinline__ T es_second(const EsArgs<T>& A, long long m, int s, T mean, T acc) {
#pragma clang fp contract(off)
  const long long SM = (long long)A.S * A.M, i = (long long)s * A.M + m;
  const T rp = A.returns[i], rm = A.returns[SM + i];
  const bool kept = A.select ? A.kept[i] != 0 : es_valid(rp, rm);
  if (kept) {
    const T dp = rp - mean, dm = rm - mean;
    acc = acc + dp * dp;
    acc = acc + dm * dm;
  }
  return acc;
}

__device__ __forceinline__ float es_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double es_sqrt(double x) { return __builtin_sqrt(x); }

// Step 3 behind the trees, by the one thread that holds the totals of block q of population m.
template <typename T>
__device__ __forceinline__ void es_finish(const EsArgs<T>& A, long long m, int q, int count, int used, T var_total, T g0, T g1) {
#pragma clang fp contract(off)
  const int n = A.D + 1;
  const EsPair<T> th = reinterpret_cast<const EsPair<T>*>(A.theta)[m * n + q];
  EsPair<T> out = th, gr = EsPair<T>{T(0), T(0)};
  T sigma = T(0);
  if (used > 0) {
    const T n2 = (T)(2 * used), nb = (T)used;
    sigma = es_sqrt(var_total / n2);
    sigma = sigma < A.sigma_floor ? A.sigma_floor : sigma;
    const T den = nb * sigma;
    gr.a = g0 / den;
    gr.b = g1 / den;
    const T s0 = A.step_size * gr.a, s1 = A.step_size * gr.b;
    out.a = th.a + s0;
    out.b = th.b + s1;
  }
  reinterpret_cast<EsPair<T>*>(A.theta_out)[m * n + q] = out;
  if (A.grad) reinterpret_cast<EsPair<T>*>(A.grad)[m * n + q] = gr;
  if (q == 0) {
    A.sigma_r[m] = sigma;
    A.count[m] = count;
    A.used[m] = used;
  }
}

template <typename U>
__device__ __forceinline__ U es_butterfly(U acc) {
#pragma unroll
  for (int w = 1; w < kEsChunks; w *= 2) acc = acc + __shfl_xor(acc, w);
  return acc;
}

// the trees of a wave's 64 partials, the second walk and the finish: lane c holds partial c of the first walk in `acc`
template <typename T>
__device__ __forceinline__ void es_wave_finish(const EsArgs<T>& A, long long m, int q, int c, const EsTerms<T>& acc) {
#pragma clang fp contract(off)
  const int count = es_butterfly<int>(acc.valid), used = es_butterfly<int>(acc.kept);
  const T total = es_butterfly<T>(acc.ret), g0 = es_butterfly<T>(acc.g0), g1 = es_butterfly<T>(acc.g1);
  T var = T(0);
  if (used > 0) {                                       // uniform over the wave: every lane holds the same totals
    const T mean = total / (T)(2 * used);
    for (int s = c; s < A.S; s += kEsChunks) var = es_second<T>(A, m, s, mean, var);
    var = es_butterfly<T>(var);
  }
  if (c == 0) es_finish<T>(A, m, q, count, used, var, g0, g1);
}

template <typename T>
__global__ __launch_bounds__(kEsChunks) void es_sum_kernel(const EsArgs<T> A) {
#pragma clang fp contract(off)
  const long long m = blockIdx.x;
  const int q = (int)blockIdx.y, c = threadIdx.x, S = A.S;
  EsTerms<T> acc{T(0), T(0), T(0), 0, 0};
  for (int s = c; s < S; s += kEsChunks) es_first_whole<T>(A, m, s, q, acc);
  es_wave_finish<T>(A, m, q, c, acc);
}

// es_sum_wide_kernel (S >= 1024), grid (M, D + 1), sixteen waves each.  A partial's chain is sequential, its terms are not: in
// a round thread t loads the two returns of direction round * 1024 + t, forms the two products of a kept one -- the Philox
// block, the Box-Muller pair, the difference of the returns -- and leaves all of it in LDS; behind the barrier lane c of wave 0
// adds the sixteen terms of its partial, s = c, c + 64, ... in ascending order, onto its chains and counts.  The second walk
// has the same rounds: sixteen waves load, wave 0, which alone holds the mean, forms the squared deviations and adds.
template <typename T>
__global__ __launch_bounds__(kEsWide) void es_sum_wide_kernel(const EsArgs<T> A) {
#pragma clang fp contract(off)
  __shared__ T sA[kEsWide], sB[kEsWide], sP[kEsWide], sM[kEsWide];
  __shared__ int sFlag[kEsWide];                        // bit 0: valid, bit 1: kept
  const long long m = blockIdx.x;
  const int q = (int)blockIdx.y, t = threadIdx.x, c = t % kEsChunks, S = A.S;
  const bool adds = t < kEsChunks;                      // wave 0
  EsTerms<T> acc{T(0), T(0), T(0), 0, 0};
  for (int base = 0; base < S; base += kEsWide) {       // (uniform over the workgroup: every thread reaches both barriers)
    const int s = base + t;
    EsPair<T> p{T(0), T(0)};
    T rp = T(0), rm = T(0);
    int flag = 0;
    if (s < S) {
      const EsReturns<T> r = es_returns<T>(A, m, s);
      rp = r.rp;
      rm = r.rm;
      flag = (r.valid ? 1 : 0) | (r.kept ? 2 : 0);
      if (r.kept) p = es_products<T>(A, m, s, q, r);
      if (!A.select && q == 0) A.kept[(long long)s * A.M + m] = r.valid ? 1 : 0;
    }
    sA[t] = p.a;
    sB[t] = p.b;
    sP[t] = rp;
    sM[t] = rm;
    sFlag[t] = flag;
    __syncthreads();
    if (adds) {
#pragma unroll
      for (int j = 0; j < kEsWide / kEsChunks; ++j) {
        const int at = j * kEsChunks + c, f = sFlag[at];
        const bool k = (f & 2) != 0;                    // (a return that is not finite never touches a chain)
        const T ret = (acc.ret + sP[at]) + sM[at];
        acc.valid += f & 1;
        acc.kept += k ? 1 : 0;
        acc.ret = k ? ret : acc.ret;
        acc.g0 = k ? acc.g0 + sA[at] : acc.g0;
        acc.g1 = k ? acc.g1 + sB[at] : acc.g1;
      }
    }
    __syncthreads();
  }
  int count = 0, used = 0;
  T g0 = T(0), g1 = T(0), mean = T(0), var = T(0);
  if (adds) {                                           // the trees: every lane of wave 0 holds the same totals
    count = es_butterfly<int>(acc.valid);
    used = es_butterfly<int>(acc.kept);
    const T total = es_butterfly<T>(acc.ret);
    g0 = es_butterfly<T>(acc.g0);
    g1 = es_butterfly<T>(acc.g1);
    if (used > 0) mean = total / (T)(2 * used);
  }
  for (int base = 0; base < S; base += kEsWide) {
    const int s = base + t;
    T rp = T(0), rm = T(0);
    int flag = 0;
    if (s < S) {
      const EsReturns<T> r = es_returns<T>(A, m, s);
      rp = r.rp;
      rm = r.rm;
      flag = r.kept ? 2 : 0;
    }
    sP[t] = rp;
    sM[t] = rm;
    sFlag[t] = flag;
    __syncthreads();
    if (adds) {
#pragma unroll
      for (int j = 0; j < kEsWide / kEsChunks; ++j) {
        const int at = j * kEsChunks + c;
        const T dp = sP[at] - mean, dm = sM[at] - mean;
        const T sq = (var + dp * dp) + dm * dm;
        var = (sFlag[at] & 2) != 0 ? sq : var;
      }
    }
    __syncthreads();
  }
  if (!adds) return;
  var = es_butterfly<T>(var);
  if (c == 0) es_finish<T>(A, m, q, count, used, var, g0, g1);
}

// The adjacent-pair tree over partials that arrive one after the other, c = 0 .. 63: level b holds the sum of a finished block
// of 2^b partials until its right neighbour is finished.  `c` is uniform, the levels are indexed at compile time.  After the
// push of c = 63 the total is returned.
template <typename U>
__device__ __forceinline__ U es_push(U (&level)[kEsLevels], U v, int c) {
#pragma clang fp contract(off)
  bool carry = true;
#pragma unroll
  for (int b = 0; b < kEsLevels; ++b) {
    const bool bit = ((c >> b) & 1) != 0;
    const U merged = level[b] + v;
    level[b] = (carry && !bit) ? v : level[b];
    v = (carry && bit) ? merged : v;
    carry = carry && bit;
  }
  return v;
}

template <typename T>
__global__ __launch_bounds__(kEsBlock) void es_sum_few_kernel(const EsArgs<T> A) {
#pragma clang fp contract(off)
  const long long m = (long long)blockIdx.x * kEsBlock + threadIdx.x;
  if (m >= A.M) return;
  const int q = (int)blockIdx.y, S = A.S;
  T lr[kEsLevels], l0[kEsLevels], l1[kEsLevels];
#pragma unroll
  for (int b = 0; b < kEsLevels; ++b) lr[b] = l0[b] = l1[b] = T(0);
  int count = 0, used = 0;
  T total = T(0), g0 = T(0), g1 = T(0);
#pragma unroll 1
  for (int c = 0; c < kEsChunks; ++c) {
    EsTerms<T> part{T(0), T(0), T(0), 0, 0};
    if (c < S) es_first_whole<T>(A, m, c, q, part);     // uniform
    count += part.valid;
    used += part.kept;
    total = es_push<T>(lr, part.ret, c);
    g0 = es_push<T>(l0, part.g0, c);
    g1 = es_push<T>(l1, part.g1, c);
  }
  T var = T(0);
  if (used > 0) {
    const T mean = total / (T)(2 * used);
#pragma unroll
    for (int b = 0; b < kEsLevels; ++b) lr[b] = T(0);
#pragma unroll 1
    for (int c = 0; c < kEsChunks; ++c) var = es_push<T>(lr, c < S ? es_second<T>(A, m, c, mean, T(0)) : T(0), c);
  }
  es_finish<T>(A, m, q, count, used, var, g0, g1);
}

// the launches of the two calls (os2r_es_inst.hip, once per dtype)
template <typename T>
void launch_es_perturb(const EsArgs<T>& args, hipStream_t stream);
template <typename T>
void launch_es_update(const EsArgs<T>& args, hipStream_t stream);

}  // namespace os2r
