// os2r_cma.hpp — os2rk_cma_sample and os2rk_cma_update: Cholesky-CMA-ES of many populations of the linear policy (gfx950).  The
// normals are never read: every kernel that needs z[m][s] forms it from the counter RNG of os2r_device.hpp (normal2, stream
// OS2RK_STREAM), in double, rounded once to T.
//
// cma_factor_kernel, grid M, one wave each.  The covariance's lower triangle goes to LDS; in column j lane i >= j forms
// C[i][j] - sum A[i][k] A[j][k] (for i = j that is the diagonal's own chain, the same products), lane j's value is handed round,
// tested on its bits, rooted, and the lanes below divide.  The wave writes the factor, or zeros, as one contiguous span.
// cma_sample_kernel, grid ceil(S M / G) with G = 256 / (D + 1) lanes of the populations a workgroup: a thread owns one Philox
// block q of one (m, s), leaves its two normals in LDS and, behind the barrier, runs the two chains y[2 q], y[2 q + 1] over the
// lane's normals with the factor's rows from global memory (5.4 KB a population, read by every one of its lanes: cache hits).
// z and weights go as aligned pairs, as in es_perturb_kernel.
// cma_rank_kernel, grid ceil(S M / 256): the thread of (s, m) walks the S returns of population m (four loads in flight, the
// threads of a wave read neighbouring populations or, with M = 1, the same word) and counts the valid lanes, the valid lanes
// ahead of its own and the invalid ones below it: the rank of the contract, whatever the lane is.  The thread of s = 0 writes
// count and status.  The contract fixes the ranks, not the method: a count needs no LDS and no barrier, and costs S^2 M
// comparisons on order-preserving integer keys (es_key of os2r_es.hpp).
// cma_sum_kernel, grid M, sixteen waves each.  The 2 E + E (E + 1) / 2 sums of a population (zw, yw, the triangle R: 403 at
// D = 10) are dealt to the waves, sum k to wave k % 16: a lane holds at most 26 accumulators, indexed at compile time, and lane
// c of every wave is partial c of the wave's sums.  A round is 64 samples, s = 64 r + c: all sixteen waves regenerate the normals
// of the round's parents (a thread a Philox block), then the chains y and t = w y (a thread an entry), all of it left in LDS as
// rows [entry][c]; behind the barrier every sum is a product of two rows (w z[e], w y[e], t[i] y[j]), read without a bank
// conflict, added where sample s is a parent.  After the last round the xor butterfly over 1, 2, .. 32 leaves the adjacent-pair
// tree in lane 0 (the levels that would add only empty partials, with S <= 32, are left out); the totals meet in LDS and the
// workgroup forms steps 4 to 8 of the contract, a thread an entry of the covariance.  A population whose status is not 0 copies its state.  One kernel for every S: what a round costs where most of
// its 64 partials are empty, and what the one workgroup of a lone population costs, is in DESIGN.md section 4.
// No lane indexes a register array at run time, nothing goes to scratch (tests/test_cma_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_cma.h: the layout's dtype, no contraction, every chain in the order given
// there.  tests/test_cma_host.py restates it in numpy; tests/test_gpu_cma.py compares bit for bit.
#pragma once
#include "os2r_es.hpp"                 // es_key, es_butterfly, EsPair; through it os2r_bits.hpp and os2r_device.hpp
#include "../../include/os2r_cma.h"

namespace os2r {

constexpr uint32_t kStreamCmaNormal = OS2RK_STREAM;     // beside the five of os2r_device.hpp and the one of os2r_es.hpp
constexpr int kCmaChunks = OS2RK_CHUNKS;                 // partials of a sum over the parents: the lanes of one wave
constexpr int kCmaBlock = 256;                           // threads of a workgroup of the sample and rank kernels
constexpr int kCmaWaves = 16;                            // waves of a workgroup of the sum kernel
constexpr int kCmaSumBlock = kCmaWaves * kCmaChunks;
constexpr int kCmaMaxE = 2 * (OS2R_MAX_OBS + 1);         // 26
constexpr int kCmaMaxSums = 2 * kCmaMaxE + kCmaMaxE * (kCmaMaxE + 1) / 2;          // 403
constexpr int kCmaOwn = (kCmaMaxSums + kCmaWaves - 1) / kCmaWaves;                 // 26 sums a wave at the most
constexpr int kCmaRows = 3 * kCmaMaxE + 1;               // of a round in LDS: z, y, t = w y, and w
static_assert(kCmaChunks == 64 && kCmaChunks == kEsChunks, "a partial is a lane of a wave");
static_assert(kStreamCmaNormal > kStreamEsDirection, "a stream of its own");
static_assert(kCmaChunks * (OS2R_MAX_OBS + 1) <= kCmaSumBlock, "a thread a Philox block of a round");

template <typename T>
struct CmaArgs {
  const T* __restrict__ returns;      // [S M]
  const T* __restrict__ rankw;        // [mu]
  const T* __restrict__ mean;         // [M][E]
  const T* __restrict__ sigma;        // [M]
  const T* __restrict__ cov;          // [M][E][E]
  const T* __restrict__ p_sigma;      // [M][E]
  const T* __restrict__ p_c;          // [M][E]
  const T* factor_in;                 // [M][E][E]  (update; the sample call writes `factor` and reads it in its second launch)
  const int* failed_in;               // [M]        (update)
  T* factor;                          // [M][E][E]  (sample)
  int* failed;                        // [M]        (sample)
  T* __restrict__ weights;            // [S M][E]   (sample)
  T* __restrict__ z;                  // [S M][E] or null  (sample)
  T* __restrict__ mean_out;
  T* __restrict__ sigma_out;
  T* __restrict__ cov_out;
  T* __restrict__ p_sigma_out;
  T* __restrict__ p_c_out;
  int* __restrict__ count;            // [M]
  int* status;                        // [M]: written by the rank launch, read by the sum launch
  int* rank;                          // [S M]: likewise
  T* __restrict__ yw;                 // [M][E] or null
  T* __restrict__ ps_norm;            // [M] or null
  T* __restrict__ growth;             // [M] or null
  unsigned long long seed;
  long long M;
  uint32_t pop_offset, generation;
  int S, D, mu;
  T a_sigma, b_sigma, hsig_bound, a_c, b_c, k0_moving, k0_stalled, c_1, c_mu, g_sigma, chi, sigma_min, sigma_max;   // rounded by the host
};

// finite and > 0, on the bits (os2r_bits.hpp says why)
__device__ __forceinline__ bool cma_positive(float x) {
  const unsigned b = steer_bits(x);
  return (b >> 31) == 0u && (b >> 23 & 0xffu) != 0xffu && b != 0u;
}
__device__ __forceinline__ bool cma_positive(double x) {
  const unsigned long long b = steer_bits(x);
  return (b >> 63) == 0ull && (b >> 52 & 0x7ffull) != 0x7ffull && b != 0ull;
}

__device__ __forceinline__ float cma_exp(float x) { return expf(x); }
__device__ __forceinline__ double cma_exp(double x) { return exp(x); }

// the Philox block q of sample s of population m: entries 2 q and 2 q + 1 of z[m][s], rounded once to T
template <typename T>
__device__ __forceinline__ EsPair<T> cma_normals(const CmaArgs<T>& A, long long m, int s, int q) {
  double z0, z1;
  normal2(A.seed, A.pop_offset + (uint32_t)m, kStreamCmaNormal, A.generation, 16u * (uint32_t)s + (uint32_t)q, z0, z1);
  return EsPair<T>{(T)z0, (T)z1};
}

template <typename T>
__global__ __launch_bounds__(kCmaChunks) void cma_factor_kernel(const CmaArgs<T> A) {
#pragma clang fp contract(off)
  __shared__ T sF[kCmaMaxE * kCmaMaxE];
  const long long m = blockIdx.x;
  const int E = 2 * (A.D + 1), lane = threadIdx.x;
  const T* const C = A.cov + m * E * E;
  for (int at = lane; at < E * E; at += kCmaChunks) {
    const int i = at / E, j = at % E;
    sF[at] = i >= j ? C[at] : T(0);                     // only the lower triangle is read
  }
  __syncthreads();
  int failed = 0;
  for (int j = 0; j < E; ++j) {                         // (uniform: `failed` is the same in every lane)
    T acc = T(0);
    const bool mine = lane >= j && lane < E;
    if (mine) {
      acc = sF[lane * E + j];
      for (int k = 0; k < j; ++k) acc = acc - sF[lane * E + k] * sF[j * E + k];
    }
    const T diag = __shfl(acc, j);
    if (!cma_positive(diag)) {
      failed = j + 1;
      break;
    }
    const T root = es_sqrt(diag);
    if (mine) sF[lane * E + j] = lane == j ? root : acc / root;    // (its own entry: no other lane read it in this column)
    __syncthreads();
  }
  if (failed == 0 && !cma_positive(A.sigma[m])) failed = E + 1;
  T* const F = A.factor + m * E * E;
  for (int at = lane; at < E * E; at += kCmaChunks) F[at] = failed ? T(0) : sF[at];
  if (lane == 0) A.failed[m] = failed;
}

template <typename T>
__global__ __launch_bounds__(kCmaBlock) void cma_sample_kernel(const CmaArgs<T> A) {
#pragma clang fp contract(off)
  __shared__ T sZ[kCmaBlock * 2];                       // [lane of the workgroup][E]
  const int n = A.D + 1, E = 2 * n, G = kCmaBlock / n;
  const long long SM = (long long)A.S * A.M;
  const int g = (int)threadIdx.x / n, q = (int)threadIdx.x % n;
  const long long sm = (long long)blockIdx.x * G + g;
  const bool live = g < G && sm < SM;
  long long m = 0;
  if (live) {
    m = sm % A.M;
    const EsPair<T> d = cma_normals<T>(A, m, (int)(sm / A.M), q);
    sZ[g * E + 2 * q] = d.a;
    sZ[g * E + 2 * q + 1] = d.b;
    if (A.z) reinterpret_cast<EsPair<T>*>(A.z)[sm * n + q] = d;
  }
  __syncthreads();
  if (!live) return;
  const EsPair<T> mean = reinterpret_cast<const EsPair<T>*>(A.mean)[m * n + q];
  EsPair<T> out = mean;
  if (A.failed[m] == 0) {
    const T* const zl = sZ + g * E;
    const T* const r0 = A.factor + (m * E + 2 * q) * E;
    const T* const r1 = r0 + E;
    T y0 = r0[0] * zl[0], y1 = r1[0] * zl[0];
    for (int j = 1; j <= 2 * q; ++j) {
      y0 = y0 + r0[j] * zl[j];
      y1 = y1 + r1[j] * zl[j];
    }
    y1 = y1 + r1[2 * q + 1] * zl[2 * q + 1];
    const T sg = A.sigma[m];
    const T p0 = sg * y0, p1 = sg * y1;
    out.a = mean.a + p0;
    out.b = mean.b + p1;
  }
  reinterpret_cast<EsPair<T>*>(A.weights)[sm * n + q] = out;
}

// per lane its rank, per population count and status
template <typename T>
__global__ __launch_bounds__(kCmaBlock) void cma_rank_kernel(const CmaArgs<T> A) {
  using U = decltype(es_key(T(0)));
  const long long M = A.M, SM = (long long)A.S * M;
  const long long i = (long long)blockIdx.x * kCmaBlock + threadIdx.x;
  if (i >= SM) return;
  const long long m = i % M;
  const int S = A.S, mine = (int)(i / M);
  const T* const ret = A.returns + m;
  const T r_own = ret[(long long)mine * M];
  const bool own_valid = steer_finite(r_own);
  const U own = es_key(r_own);
  int valid = 0, ahead = 0, below = 0;                  // valid lanes; valid lanes ahead of a valid own; invalid lanes below s
  auto tally = [&](T r, int s) {
    const bool v = steer_finite(r);
    const U k = es_key(r);
    valid += v ? 1 : 0;
    ahead += (v && (k > own || (k == own && s < mine))) ? 1 : 0;
    below += (!v && s < mine) ? 1 : 0;
  };
  int s = 0;
  for (; s + 3 < S; s += 4) {                           // four loads are in flight together
    const T r0 = ret[(long long)s * M], r1 = ret[(long long)(s + 1) * M], r2 = ret[(long long)(s + 2) * M], r3 = ret[(long long)(s + 3) * M];
    tally(r0, s);
    tally(r1, s + 1);
    tally(r2, s + 2);
    tally(r3, s + 3);
  }
  for (; s < S; ++s) tally(ret[(long long)s * M], s);
  A.rank[i] = own_valid ? ahead : valid + below;
  if (mine == 0) {
    A.count[m] = valid;
    A.status[m] = A.failed_in[m] != 0 ? 2 : (valid < A.mu ? 1 : 0);
  }
}

// The adjacent-pair tree of a wave's 64 partials, in lane 0 (and in every lane that is a multiple of `span`).  With S <= 32 samples
// the partials from span = the power of two that holds S on are empty, and a level that adds a block of zeros changes no bit
// (the sign of a zero aside, which is not part of the contract): those levels are left out, six exchanges through LDS hardware
// per sum and level that a population of four samples does not pay for.
template <typename T>
__device__ __forceinline__ T cma_butterfly(T acc, int span) {
#pragma unroll
  for (int w = 1; w < kCmaChunks; w *= 2)
    if (w < span) acc = acc + __shfl_xor(acc, w);       // (uniform)
  return acc;
}

// The kernel's own argument block, read where it is used.  The compiler loads every field of a kernel's by-value argument in
// the entry block; the 84 words of CmaArgs<double>, most of them needed only behind the rounds, then live across them and spill
// SGPRs.  What the sum kernel needs late it reads through this pointer, which the empty asm keeps from being traced back to the
// argument; the early fields alone are read from `A`.
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(4))) CmaArgs<T>* cma_late_args() {
  auto* p = (const __attribute__((address_space(4))) CmaArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// sum k of a population -> the two rows of a round whose product is its term: rows 0 .. E - 1 are z, E .. 2 E - 1 y,
// 2 E .. 3 E - 1 t = w y, 3 E is w.  Sums 0 .. E - 1 are zw, E .. 2 E - 1 yw, then R by rows: (0,0), (1,0), (1,1), (2,0), ...
__device__ __forceinline__ int cma_rows_of(int k, int E) {
  if (k < E) return (3 * E) << 8 | k;                   // w z[e]
  if (k < 2 * E) return (3 * E) << 8 | k;               // w y[e]: row E + e
  const int r = k - 2 * E;
  int i = (int)((__builtin_sqrtf(8.0f * (float)r + 1.0f) - 1.0f) * 0.5f);
  i += (i + 1) * (i + 2) / 2 <= r ? 1 : 0;
  i -= i * (i + 1) / 2 > r ? 1 : 0;
  const int j = r - i * (i + 1) / 2;
  return (2 * E + i) << 8 | (E + j);                    // t[i] y[j]
}

template <typename T>
__global__ __launch_bounds__(kCmaSumBlock) void cma_sum_kernel(const CmaArgs<T> A) {
#pragma clang fp contract(off)
  __shared__ T sX[kCmaRows * kCmaChunks];               // the rows of a round, [row][c]
  __shared__ T sF[kCmaMaxE * kCmaMaxE];                 // the factor
  __shared__ T sTot[kCmaMaxSums];                       // the totals
  __shared__ T sPs[kCmaMaxE], sPc[kCmaMaxE], sScal[2];  // p_sigma_out, p_c_out; k0 and whether h holds
  __shared__ int sParent[kCmaChunks], sPair[kCmaOwn * kCmaWaves];
  const long long m = blockIdx.x;
  const int t = threadIdx.x, c = t % kCmaChunks, wave = t / kCmaChunks;
  const int n = A.D + 1, E = 2 * n, S = A.S, sums = 2 * E + E * (E + 1) / 2;
  if (A.status[m] != 0) {                               // (uniform over the workgroup) the state as it was
    const auto* const L = cma_late_args<T>();
    for (int at = t; at < E * E; at += kCmaSumBlock) L->cov_out[m * E * E + at] = L->cov[m * E * E + at];
    if (t < E) {
      L->mean_out[m * E + t] = L->mean[m * E + t];
      L->p_sigma_out[m * E + t] = L->p_sigma[m * E + t];
      L->p_c_out[m * E + t] = L->p_c[m * E + t];
      if (L->yw) L->yw[m * E + t] = T(0);
    }
    if (t == 0) {
      L->sigma_out[m] = L->sigma[m];
      if (L->ps_norm) L->ps_norm[m] = T(0);
      if (L->growth) L->growth[m] = T(1);
    }
    return;
  }
  for (int at = t; at < E * E; at += kCmaSumBlock) sF[at] = A.factor_in[m * E * E + at];
  // (a wave's slots beyond the last sum multiply row 0 by itself into an accumulator that nobody reads: a test of k < sums in
  // the rounds costs two SGPRs a slot, held across them)
  if (t < kCmaOwn * kCmaWaves) sPair[t] = t < sums ? cma_rows_of(t, E) : 0;
  T acc[kCmaOwn];
#pragma unroll
  for (int o = 0; o < kCmaOwn; ++o) acc[o] = T(0);
  for (int base = 0; base < S; base += kCmaChunks) {    // (uniform over the workgroup: every thread reaches every barrier)
    const int s = base + c;
    int rank = A.mu;
    if (s < S) rank = A.rank[(long long)s * A.M + m];
    const bool parent = rank < A.mu;
    if (wave < n) {                                     // wave q: Philox block q of the round's samples
      EsPair<T> d{T(0), T(0)};
      if (parent) d = cma_normals<T>(A, m, s, wave);
      sX[(2 * wave) * kCmaChunks + c] = d.a;
      sX[(2 * wave + 1) * kCmaChunks + c] = d.b;
    }
    if (wave == kCmaWaves - 1) {
      sX[3 * E * kCmaChunks + c] = parent ? A.rankw[rank] : T(0);
      sParent[c] = parent ? 1 : 0;
    }
    __syncthreads();
    const T w = sX[3 * E * kCmaChunks + c];
    for (int e = wave; e < E; e += kCmaWaves) {         // (e is uniform over the wave: the factor's row is read once for all lanes)
      T y = sF[e * E] * sX[c];
      for (int j = 1; j <= e; ++j) y = y + sF[e * E + j] * sX[j * kCmaChunks + c];
      sX[(E + e) * kCmaChunks + c] = y;
      sX[(2 * E + e) * kCmaChunks + c] = w * y;
    }
    __syncthreads();
    const bool adds = sParent[c] != 0;
#pragma unroll
    for (int o = 0; o < kCmaOwn; ++o) {
      const int pair = sPair[o * kCmaWaves + wave];
      const T term = sX[(pair >> 8) * kCmaChunks + c] * sX[(pair & 0xff) * kCmaChunks + c];
      const T next = acc[o] + term;
      acc[o] = adds ? next : acc[o];
    }
    __syncthreads();
  }
  int span = 1;                                         // the partials from `span` on are empty: 64, or the power of two that holds S
  while (span < kCmaChunks && span < S) span *= 2;
#pragma unroll
  for (int o = 0; o < kCmaOwn; ++o) {
    const int k = o * kCmaWaves + wave;
    const T total = cma_butterfly<T>(acc[o], span);
    if (k < sums && c == 0) sTot[k] = total;
  }
  __syncthreads();
  const auto* const L = cma_late_args<T>();
  // steps 4 to 8: zw = sTot[0 .. E), yw = sTot[E .. 2 E), R = sTot[2 E ..)
  const T sg = L->sigma[m];
  if (t < E) {
    const T yw = sTot[E + t];
    const T step = sg * yw;
    L->mean_out[m * E + t] = L->mean[m * E + t] + step;
    if (L->yw) L->yw[m * E + t] = yw;
    const T keep = L->a_sigma * L->p_sigma[m * E + t], push = L->b_sigma * sTot[t];
    const T ps = keep + push;
    sPs[t] = ps;
    L->p_sigma_out[m * E + t] = ps;
  }
  __syncthreads();
  if (t == 0) {
    T sq = T(0);
    for (int e = 0; e < E; ++e) sq = sq + sPs[e] * sPs[e];
    const T nrm = es_sqrt(sq);
    const bool h = nrm < L->hsig_bound;
    sScal[0] = h ? L->k0_moving : L->k0_stalled;
    sScal[1] = h ? T(1) : T(0);
    const T ratio = nrm / L->chi;
    const T arg = L->g_sigma * (ratio - T(1));
    const T growth = cma_exp(arg);
    T next = sg * growth;
    next = next < L->sigma_min ? L->sigma_min : next;
    next = next > L->sigma_max ? L->sigma_max : next;
    L->sigma_out[m] = next;
    if (L->ps_norm) L->ps_norm[m] = nrm;
    if (L->growth) L->growth[m] = growth;
  }
  __syncthreads();
  if (t < E) {
    const T keep = L->a_c * L->p_c[m * E + t], push = L->b_c * sTot[E + t];
    const T moved = keep + push;
    const T pc = sScal[1] != T(0) ? moved : keep;
    sPc[t] = pc;
    L->p_c_out[m * E + t] = pc;
  }
  __syncthreads();
  const T k0 = sScal[0];
  for (int at = t; at < E * E; at += kCmaSumBlock) {
    const int a = at / E, b = at % E, i = a > b ? a : b, j = a > b ? b : a;
    const T old = k0 * L->cov[(m * E + i) * E + j];
    const T one = L->c_1 * (sPc[i] * sPc[j]);
    const T many = L->c_mu * sTot[2 * E + i * (i + 1) / 2 + j];
    L->cov_out[m * E * E + at] = (old + one) + many;
  }
}

// the launches of the two calls (os2r_cma_inst.hip, once per dtype)
template <typename T>
void launch_cma_sample(const CmaArgs<T>& args, hipStream_t stream);
template <typename T>
void launch_cma_update(const CmaArgs<T>& args, hipStream_t stream);

}  // namespace os2r
