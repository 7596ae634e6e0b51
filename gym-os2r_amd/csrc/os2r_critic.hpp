// os2r_critic.hpp — os2rv_gae and os2rv_value_fit: the critic of many linear-Gaussian policies (gfx950), six kernels; the two
// that sum over the samples of a policy are the bodies of os2r_pg.hpp as they are.
//
// os2rv_gae, two launches:
//   critic_value_kernel, grid (ceil(N / 256), K), a thread per (k, lane): value[k][l] = val(x_k), one dot product of D terms
//     on a row the thread reads whole (neighbouring threads read neighbouring rows: the wave one contiguous span), 0 where
//     k >= len.  The K N dot products are independent: this launch is bound by the bytes of obs
//   critic_scan_kernel, grid ceil(N / 64), a thread per lane: the backward recurrence of include/os2r_critic.h over reward, done
//     and value, each [K][N] and read coalesced, four steps' loads issued before the first is used.  val(obs[k][l]) of a step
//     that is not cut is value[k + 1][l], carried in a register; only the bootstrap behind the last counted step and the
//     terminal observation of a truncated step are dot products of this launch.  It is bound by the chain: four dependent
//     operations a step
// os2rv_value_fit, three launches:
//   critic_moment_kernel, grid ceil(8 N / 256).  Each of a lane's E sums is a chain of its own over the steps, so a lane is
//     shared among kCrThreads = 8 neighbouring threads.  The rows of the products x_i x_j, i <= j < 12, are paired so that every
//     pair has 13 of them: thread h < 6 owns rows h and 11 - h and, for both, the sum of x_i and of x_i y -- 17 chains; the
//     sum of y is every thread's (that of thread 6 is stored), M[D][D] is len itself (a sum of len ones is exact below 2^24).
//     Threads 6 and 7 own no row.  Which operand meets which is decided by h in the address of the load and in a select of the
//     left factor: no register array is indexed at run time.  kCrMomSteps steps of loads are in flight.  A lane is valid iff every
//     one of its threads found its sums finite: three xor shuffles inside the wave
//   critic_sum_kernel (S > 64) and critic_sum_few_kernel (S <= 64): pg_wave_sum and pg_few_sum of os2r_pg.hpp over the E entries
//     of lane_mom and the two rows of lane_count
//   critic_solve_kernel, grid ceil(P / 64), a thread per policy: the factor and the two substitutions, the factor and z in
//     LDS laid out [entry][thread] (conflict-free; 13 x 13 would not stay in registers in fp64 without a spill), indexed at run
//     time by D -- LDS is memory, not a register array
// Nothing goes to scratch (tests/test_critic_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_critic.h: the layout's dtype, no contraction, every chain in the order given
// there.  tests/test_critic_host.py restates it in numpy; tests/test_gpu_critic.py compares bit for bit.
#pragma once
#include "os2r_pg.hpp"
#include "../../include/os2r_critic.h"

namespace os2r {

constexpr int kCrObs = OS2R_MAX_OBS;             // 12
constexpr int kCrThreads = 8;                    // threads of one lane in the moment kernel
constexpr int kCrPairs = kCrObs / 2;             // row pairs (h, 11 - h): the threads that own rows
constexpr int kCrProducts = kCrObs + 1;          // products x_i x_j of one row pair
constexpr int kCrSteps = 4;                      // steps of one round of the scan: their loads are in flight together
constexpr int kCrMomSteps = 2;                   // ... and of the moment kernel, which holds 15 values a step
constexpr int kCrBlock = 256;
constexpr int kCrScanBlock = 64;                 // the scan is a chain per lane: one wave a workgroup spreads few lanes wide
constexpr int kCrSolveBlock = 64;
constexpr int kCrMaxN = kCrObs + 1;              // D + 1 at most
constexpr int kCrTri = kCrMaxN * (kCrMaxN + 1) / 2;
constexpr int kCrIntegerSums = OS2RV_LANE_COUNTS; // steps, valid: the rows of lane_count
static_assert(kCrObs == 12 && OS2RV_CHUNKS == kPgChunks && 64 % kCrThreads == 0 && kCrPairs <= kCrThreads, "the split of a lane");

template <typename T>
struct GaeArgs {
  const T* __restrict__ obs;          // [K][N][D]
  const T* __restrict__ obs0;         // [N][D]
  const T* __restrict__ term_obs;     // [K][N][D] or null
  const T* __restrict__ reward;       // [K][N]
  const unsigned char* __restrict__ done;   // [K][N]
  const int* __restrict__ length;     // [N] or null
  const T* __restrict__ value_w;      // [D+1][P]
  T* adv;                             // [K][N]
  T* ret;                             // [K][N] or null
  T* value;                           // [K][N]: written by the first launch, read by the second
  long long P, N;
  int K, D;
  T gamma, c;                         // rounded to T by the host; c = gamma lambda formed in T
};

template <typename T>
struct FitArgs {
  const T* __restrict__ obs;          // [K][N][D]
  const T* __restrict__ obs0;         // [N][D]
  const T* __restrict__ target;       // [K][N]
  const int* __restrict__ length;     // [N] or null
  const T* __restrict__ prev_w;       // [D+1][P] or null
  T* w;                               // [D+1][P]
  T* lane_mom;                        // [E][N]: written by the first launch, read by the second
  T* mom;                             // [E][P]: written by the second, read by the third
  int* lane_count;                    // [2][N]: len, valid; as lane_mom
  int* failed;                        // [P] or null
  int* steps;                         // [P] or null
  int* valid;                         // [P] or null
  long long P, N;
  int K, S, D;
  T ridge;
};

__device__ __forceinline__ int cr_len(const int* __restrict__ length, long long l, int K) {
  const int len = length ? length[l] : K;
  return len < 0 ? 0 : (len > K ? K : len);
}

// the value weights of policy p: w[d] for d < D (0 above), w[kCrObs] the bias
template <typename T>
__device__ __forceinline__ void cr_weights(const T* __restrict__ W, long long P, long long p, int D, T (&w)[kCrObs + 1]) {
#pragma unroll
  for (int d = 0; d < kCrObs; ++d) w[d] = d < D ? W[(long long)d * P + p] : T(0);
  w[kCrObs] = W[(long long)D * P + p];
}

// val(x; w) = (((w_D + w_0 x_0) + w_1 x_1) + ...)
template <typename T>
__device__ __forceinline__ T cr_val(const T (&w)[kCrObs + 1], const T* __restrict__ x, int D) {
#pragma clang fp contract(off)
  T acc = w[kCrObs];
#pragma unroll
  for (int d = 0; d < kCrObs; ++d)
    if (d < D) acc = acc + w[d] * x[d];                 // uniform
  return acc;
}

template <typename T>
__global__ __launch_bounds__(kCrBlock) void critic_value_kernel(const GaeArgs<T> A) {
#pragma clang fp contract(off)
  const long long l = (long long)blockIdx.x * kCrBlock + threadIdx.x;
  if (l >= A.N) return;
  const int k = (int)blockIdx.y, D = A.D;
  const long long at = (long long)k * A.N + l;
  if (k >= cr_len(A.length, l, A.K)) {
    A.value[at] = T(0);
    return;
  }
  T w[kCrObs + 1];
  cr_weights(A.value_w, A.P, l % A.P, D, w);
  const T* const x = k ? A.obs + (at - A.N) * D : A.obs0 + l * D;
  A.value[at] = cr_val(w, x, D);
}

template <typename T>
struct GaeStep {
  T r, v;
  unsigned f;
  long long at;     // k N + l
};

template <typename T>
__global__ __launch_bounds__(kCrScanBlock) void critic_scan_kernel(const GaeArgs<T> A) {
#pragma clang fp contract(off)
  const long long l = (long long)blockIdx.x * kCrScanBlock + threadIdx.x;
  const long long N = A.N;
  if (l >= N) return;
  const int K = A.K, D = A.D;
  const int len = cr_len(A.length, l, K);
  T w[kCrObs + 1];
  cr_weights(A.value_w, A.P, l % A.P, D, w);
  const T gamma = A.gamma, c = A.c;
  // what follows the last counted step: val(obs[len - 1][l]), the chain the first launch would run for step len
  T next = len > 0 ? cr_val(w, A.obs + ((long long)(len - 1) * N + l) * D, D) : T(0);
  T trace = T(0);

  auto load = [&](int k) {
    GaeStep<T> s;
    s.at = (long long)k * N + l;
    s.r = A.reward[s.at];
    s.v = A.value[s.at];
    s.f = (unsigned)A.done[s.at];
    return s;
  };
  auto apply = [&](const GaeStep<T>& s) {
    T nv = next;
    const bool cut = (s.f & 7u) != 0u;
    if (s.f & 5u)
      nv = T(0);
    else if (s.f & 2u)
      nv = A.term_obs ? cr_val(w, A.term_obs + s.at * D, D) : T(0);
    const T delta = (s.r + gamma * nv) - s.v;
    trace = cut ? delta : delta + c * trace;
    A.adv[s.at] = trace;
    if (A.ret) A.ret[s.at] = trace + s.v;
    next = s.v;
  };
  int k = len - 1;
  for (; k >= kCrSteps - 1; k -= kCrSteps) {
    GaeStep<T> s[kCrSteps];
#pragma unroll
    for (int i = 0; i < kCrSteps; ++i) s[i] = load(k - i);
#pragma unroll
    for (int i = 0; i < kCrSteps; ++i) apply(s[i]);
  }
  for (; k >= 0; --k) apply(load(k));
  for (int z = len; z < K; ++z) {
    A.adv[(long long)z * N + l] = T(0);
    if (A.ret) A.ret[(long long)z * N + l] = T(0);
  }
}

// what one thread of the moment kernel reads of one step
template <typename T>
struct MomStep {
  T r[kCrProducts];   // the right factors of its 13 products; r[0] is x of its first row
  T xb, y;            // x of its second row, the target
};

template <typename T>
__global__ __launch_bounds__(kCrBlock) void critic_moment_kernel(const FitArgs<T> A) {
#pragma clang fp contract(off)
  const long long gid = (long long)blockIdx.x * kCrBlock + threadIdx.x;
  const long long N = A.N, l = gid / kCrThreads;
  if (l >= N) return;                                   // (whole lanes: 256 and 8 N are multiples of 8)
  const int h = (int)(gid % kCrThreads);
  const int K = A.K, D = A.D;
  const int Dh = h < kCrPairs ? D : 0;                   // threads 6 and 7 own no row: every slot of theirs is above it
  const int ra = h, rb = kCrObs - 1 - h;                // the two rows; row ra has kCrObs - h products, row rb h + 1
  const int len = cr_len(A.length, l, K);

  auto slot = [&](int e) { return e <= rb ? h + e : e - 1; };   // the column of product e: ra .. 11, then rb .. 11
  auto load = [&](int k) {
    MomStep<T> s;
    const T* const x = k ? A.obs + ((long long)(k - 1) * N + l) * D : A.obs0 + l * D;
#pragma unroll
    for (int e = 0; e < kCrProducts; ++e) s.r[e] = slot(e) < Dh ? x[slot(e)] : T(0);
    s.xb = rb < Dh ? x[rb] : T(0);
    s.y = A.target[(long long)k * N + l];
    return s;
  };

  T acc[kCrProducts];
#pragma unroll
  for (int e = 0; e < kCrProducts; ++e) acc[e] = T(0);
  T sum_a = T(0), sum_b = T(0), b_a = T(0), b_b = T(0), sum_y = T(0);
  auto apply = [&](const MomStep<T>& s) {
    const T xa = s.r[0];
#pragma unroll
    for (int e = 0; e < kCrProducts; ++e) acc[e] = acc[e] + (e <= rb ? xa : s.xb) * s.r[e];
    sum_a = sum_a + xa;
    sum_b = sum_b + s.xb;
    b_a = b_a + xa * s.y;
    b_b = b_b + s.xb * s.y;
    sum_y = sum_y + s.y;
  };
  int k = len - 1;
  for (; k >= kCrMomSteps - 1; k -= kCrMomSteps) {
    MomStep<T> s[kCrMomSteps];
#pragma unroll
    for (int i = 0; i < kCrMomSteps; ++i) s[i] = load(k - i);
#pragma unroll
    for (int i = 0; i < kCrMomSteps; ++i) apply(s[i]);
  }
  for (; k >= 0; --k) apply(load(k));

  // step 2: the sums this thread stores (a column at or above D saw zeros only, and is not asked)
  int fine = 1;
#pragma unroll
  for (int e = 0; e < kCrProducts; ++e) fine &= (slot(e) >= Dh || steer_finite(acc[e])) ? 1 : 0;
  fine &= (ra >= Dh || (steer_finite(sum_a) && steer_finite(b_a))) ? 1 : 0;
  fine &= (rb >= Dh || (steer_finite(sum_b) && steer_finite(b_b))) ? 1 : 0;
  if (h == kCrPairs) fine &= steer_finite(sum_y) ? 1 : 0;
#pragma unroll
  for (int m = 1; m < kCrThreads; m *= 2) fine &= __shfl_xor(fine, m);

  // M[i][j], i <= j <= D, at i (D + 1) - i (i - 1) / 2 + (j - i); b[i] behind the triangle
  const int n = D + 1, tri = n * (n + 1) / 2;
  auto entry = [&](int i, int j) { return A.lane_mom + (long long)(i * n - i * (i - 1) / 2 + (j - i)) * N + l; };
#pragma unroll
  for (int e = 0; e < kCrProducts; ++e)
    if (slot(e) < Dh) *entry(e <= rb ? ra : rb, slot(e)) = acc[e];
  if (ra < Dh) {
    *entry(ra, D) = sum_a;
    A.lane_mom[(long long)(tri + ra) * N + l] = b_a;
  }
  if (rb < Dh) {
    *entry(rb, D) = sum_b;
    A.lane_mom[(long long)(tri + rb) * N + l] = b_b;
  }
  if (h == kCrPairs) {
    *entry(D, D) = T(len);
    A.lane_mom[(long long)(tri + D) * N + l] = sum_y;
  }
  if (h == kCrThreads - 1) {
    A.lane_count[l] = len;
    A.lane_count[N + l] = fine;
  }
}

// Entry e of the sums of step 3 -> where its per-lane terms stand and where the policies' totals go: the E entries of mom, then
// steps and valid.  False: the total is not wanted.
template <typename T>
__device__ __forceinline__ bool cr_entry(const FitArgs<T>& A, int e, PgEntry<T>& out) {
  const int n = A.D + 1, E = n * (n + 1) / 2 + n;
  out.terms = nullptr; out.totals = nullptr; out.counts = nullptr; out.count_totals = nullptr;
  if (e < E) {
    out.terms = A.lane_mom + (long long)e * A.N;
    out.totals = A.mom + (long long)e * A.P;
    return true;
  }
  int* const totals = e == E ? A.steps : A.valid;
  if (!totals) return false;
  out.counts = A.lane_count + (long long)(e - E) * A.N;
  out.count_totals = totals;
  return true;
}

template <typename T>
__global__ __launch_bounds__(kPgChunks) void critic_sum_kernel(const FitArgs<T> A) {
#pragma clang fp contract(off)
  PgEntry<T> E;
  if (!cr_entry(A, (int)blockIdx.y, E)) return;         // uniform over the workgroup
  const long long p = blockIdx.x;
  const int c = threadIdx.x;
  const int* const fine = A.lane_count + A.N;
  if (E.terms) {
    const T total = pg_wave_sum<T>(E.terms, fine, A.P, p, A.S, c);
    if (c == 0) E.totals[p] = total;
  } else {
    const int total = pg_wave_sum<int>(E.counts, fine, A.P, p, A.S, c);
    if (c == 0) E.count_totals[p] = total;
  }
}

template <typename T>
__global__ __launch_bounds__(kPgBlock) void critic_sum_few_kernel(const FitArgs<T> A) {
#pragma clang fp contract(off)
  PgEntry<T> E;
  if (!cr_entry(A, (int)blockIdx.y, E)) return;
  const long long p = (long long)blockIdx.x * kPgBlock + threadIdx.x;
  if (p >= A.P) return;
  const int* const fine = A.lane_count + A.N;
  if (E.terms)
    E.totals[p] = pg_few_sum<T>(E.terms, fine, A.P, p, A.S);
  else
    E.count_totals[p] = pg_few_sum<int>(E.counts, fine, A.P, p, A.S);
}

// finite and > 0, on the bits (os2r_bits.hpp says why)
__device__ __forceinline__ bool cr_positive(float x) { return !steer_invalid(x) && (steer_bits(x) & 0x7fffffffu) != 0u; }
__device__ __forceinline__ bool cr_positive(double x) { return !steer_invalid(x) && (steer_bits(x) & 0x7fffffffffffffffull) != 0ull; }
// one correctly rounded IEEE square root (the builtin gets the fix-up sequence in fp32)
__device__ __forceinline__ float cr_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double cr_sqrt(double x) { return __builtin_sqrt(x); }

template <typename T>
__global__ __launch_bounds__(kCrSolveBlock) void critic_solve_kernel(const FitArgs<T> A) {
#pragma clang fp contract(off)
  __shared__ T lds[(kCrTri + kCrMaxN) * kCrSolveBlock];
  const int t = threadIdx.x;
  const long long P = A.P, p = (long long)blockIdx.x * kCrSolveBlock + t;
  if (p >= P) return;                                   // (no barrier below: a thread reads what it wrote itself)
  const int n = A.D + 1, tri = n * (n + 1) / 2;
  const T ridge = A.ridge;
  auto Lo = [&](int i, int j) -> T& { return lds[(i * (i + 1) / 2 + j) * kCrSolveBlock + t]; };     // L[i][j], j <= i
  auto Z = [&](int i) -> T& { return lds[(kCrTri + i) * kCrSolveBlock + t]; };
  auto M = [&](int i, int j) { return A.mom[(long long)(i * n - i * (i - 1) / 2 + (j - i)) * P + p]; };   // i <= j

  int failed = 0;
  for (int j = 0; j < n; ++j) {
    T d = M(j, j) + ridge;
    if (j > 0) {
      T st = Lo(j, 0) * Lo(j, 0);
      for (int q = 1; q < j; ++q) st = st + Lo(j, q) * Lo(j, q);
      d = d - st;
    }
    if (!cr_positive(d)) {
      failed = j + 1;
      break;
    }
    d = cr_sqrt(d);
    Lo(j, j) = d;
    for (int i = j + 1; i < n; ++i) {
      T u = M(j, i);
      if (j > 0) {
        T su = Lo(i, 0) * Lo(j, 0);
        for (int q = 1; q < j; ++q) su = su + Lo(i, q) * Lo(j, q);
        u = u - su;
      }
      Lo(i, j) = u / d;
    }
  }
  if (A.failed) A.failed[p] = failed;
  if (failed != 0) {
    for (int i = 0; i < n; ++i) A.w[(long long)i * P + p] = A.prev_w ? A.prev_w[(long long)i * P + p] : T(0);
    return;
  }
  for (int i = 0; i < n; ++i) {
    T rhs = A.mom[(long long)(tri + i) * P + p];
    if (A.prev_w) rhs = rhs + ridge * A.prev_w[(long long)i * P + p];
    if (i > 0) {
      T s = Lo(i, 0) * Z(0);
      for (int q = 1; q < i; ++q) s = s + Lo(i, q) * Z(q);
      rhs = rhs - s;
    }
    Z(i) = rhs / Lo(i, i);
  }
  for (int i = n - 1; i >= 0; --i) {                    // w_l, l > i, stands where z_l stood
    T v = Z(i);
    if (i + 1 < n) {
      T s = Lo(i + 1, i) * Z(i + 1);
      for (int q = i + 2; q < n; ++q) s = s + Lo(q, i) * Z(q);
      v = v - s;
    }
    v = v / Lo(i, i);
    Z(i) = v;
    A.w[(long long)i * P + p] = v;
  }
}

// the launches of the two calls (os2r_critic_inst.hip, once per dtype)
template <typename T>
void launch_gae(const GaeArgs<T>& args, hipStream_t stream);
template <typename T>
void launch_value_fit(const FitArgs<T>& args, hipStream_t stream);

}  // namespace os2r
