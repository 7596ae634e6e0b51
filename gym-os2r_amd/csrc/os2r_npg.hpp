// os2r_npg.hpp — os2rn_natural_step: the natural-gradient step of many linear-Gaussian policies in three stream-ordered launches
// (gfx950); the sums over the samples of a policy are the bodies of os2r_pg.hpp as they are.
//
// npg_moment_kernel, grid ceil(8 N / 256).  The split of a lane is critic_moment_kernel's (os2r_critic.hpp): a lane is shared among
// kCrThreads = 8 neighbouring threads, thread h < 6 owns the rows h and 11 - h of the products x_i x_m -- 13 products -- and, for
// both rows, the sum of x_i; threads 6 and 7 own no row (6 stores the two corners, 7 the lane's counts).  What is new is that
// every chain stands twice, once per action component: a product is formed once and added to the chain of component j under
// the predicate "component j is open on this step", which every one of the lane's eight threads forms for itself from the pair
// of actions (one aligned load of both: hence the alignment the entry point asks for) and the lane's two widths.  A closed step
// selects the old sum: a masked product may be a NaN and must not touch the chain.  30 chains a thread, kCrMomSteps steps of
// loads in flight.  After the walk each sum is divided by sigma_j sigma_j; the lane is valid iff every one of its threads found
// its quotients finite: three xor shuffles inside the wave.
// npg_sum_kernel (S > 64) and npg_sum_few_kernel (S <= 64): pg_wave_sum and pg_few_sum of os2r_pg.hpp over the 2 Tri entries of
// lane_mom and the four rows of lane_count.
// npg_solve_kernel, grid ceil(P / 32), one wave a workgroup: thread 32 j + t owns component j of policy 32 b + t.  The factor and
// the two substitutions are those of critic_solve_kernel, in LDS laid out [entry][thread]; d_j and d_ls,j stay there, and after
// one barrier both threads of a policy read the other's and form q and beta for themselves: the one exchange of the launch.
// Nothing goes to scratch (tests/test_npg_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_npg.h: the layout's dtype, no contraction, every chain in the order given
// there.  tests/test_npg_host.py restates it in numpy; tests/test_gpu_npg.py compares bit for bit.
#pragma once
#include "os2r_critic.hpp"
#include "../../include/os2r_npg.h"

namespace os2r {

constexpr int kNpgIntegerSums = OS2RN_LANE_COUNTS;    // steps, open_0, open_1, valid: the rows of lane_count
constexpr int kNpgSolveBlock = 64;                    // one wave: 32 policies x 2 components
constexpr int kNpgSolvePolicies = kNpgSolveBlock / 2;
constexpr int kNpgSolveSlots = kCrTri + kCrMaxN + 1;  // per thread in LDS: the factor, z (then d), d_ls
static_assert(OS2RN_CHUNKS == kPgChunks && OS2RN_TANH == OS2RG_TANH && OS2RN_SIGMA_PER_LANE == OS2RG_SIGMA_PER_LANE && kCrThreads == 8,
              "the sums, the flags and the split of a lane are the siblings'");

template <typename T>
struct NpgArgs {
  const T* __restrict__ obs;          // [K][N][D]
  const T* __restrict__ obs0;         // [N][D] or null
  const T* __restrict__ action;       // [K][N][2]; not read with tanh
  const T* __restrict__ sigma;        // [2], or [2][N] with sigma_per_lane
  const int* __restrict__ length;     // [N] or null
  const T* __restrict__ grad;         // [2][D+1][P]
  const T* __restrict__ lsig_grad;    // [2][P] or null
  T* step;                            // [2][D+1][P]
  T* dir;                             // [2][D+1][P] or null
  T* lsig_step;                       // [2][P], with lsig_grad
  T* beta;                            // [P] or null
  T* quad;                            // [P] or null
  int* failed;                        // [3][P] or null
  int* steps;                         // [P] or null
  int* open;                          // [2][P] or null
  int* valid;                         // [P] or null
  T* lane_mom;                        // [2 Tri][N]: written by the first launch, read by the second
  T* mom;                             // [2 Tri][P]: written by the second, read by the third
  int* lane_count;                    // [4][N]: len, n_0, n_1, valid; as lane_mom
  long long P, N;
  int K, S, D, tanh, sigma_per_lane;
  int unit;                           // the kl argument is 0: beta = 1
  T damping, kl;                      // rounded to T by the host
};

// the two actions of one step, read at once
template <typename T>
struct alignas(2 * sizeof(T)) NpgPair {
  T a0, a1;
};

// what one thread of the moment kernel reads of one step
template <typename T>
struct NpgStep {
  T r[kCrProducts];   // the right factors of its 13 products; r[0] is x of its first row
  T xb;               // x of its second row
  NpgPair<T> a;
};

template <typename T>
__global__ __launch_bounds__(kCrBlock) void npg_moment_kernel(const NpgArgs<T> A) {
#pragma clang fp contract(off)
  const long long gid = (long long)blockIdx.x * kCrBlock + threadIdx.x;
  const long long N = A.N, l = gid / kCrThreads;
  if (l >= N) return;                                   // (whole lanes: 256 and 8 N are multiples of 8)
  const int h = (int)(gid % kCrThreads);
  const int K = A.K, D = A.D;
  const int Dh = h < kCrPairs ? D : 0;                   // threads 6 and 7 own no row: every slot of theirs is above it
  const int ra = h, rb = kCrObs - 1 - h;                // the two rows; row ra has kCrObs - h products, row rb h + 1
  const int len = cr_len(A.length, l, K);
  const bool tanh = A.tanh != 0;
  const T sig0 = A.sigma[A.sigma_per_lane ? l : 0ll], sig1 = A.sigma[A.sigma_per_lane ? N + l : 1ll];
  const bool wide0 = pg_positive(sig0), wide1 = pg_positive(sig1);
  const NpgPair<T>* const actions = reinterpret_cast<const NpgPair<T>*>(A.action);

  auto slot = [&](int e) { return e <= rb ? h + e : e - 1; };   // the column of product e: ra .. 11, then rb .. 11
  auto load = [&](int k) {
    NpgStep<T> s;
    const long long at = (long long)k * N + l;
    const T* const x = A.obs0 ? (k ? A.obs + (at - N) * D : A.obs0 + l * D) : A.obs + at * D;
#pragma unroll
    for (int e = 0; e < kCrProducts; ++e) s.r[e] = slot(e) < Dh ? x[slot(e)] : T(0);
    s.xb = rb < Dh ? x[rb] : T(0);
    if (tanh)
      s.a.a0 = s.a.a1 = T(0);
    else
      s.a = actions[at];
    return s;
  };

  T acc0[kCrProducts], acc1[kCrProducts];
#pragma unroll
  for (int e = 0; e < kCrProducts; ++e) acc0[e] = acc1[e] = T(0);
  T sa0 = T(0), sb0 = T(0), sa1 = T(0), sb1 = T(0);
  int n0 = 0, n1 = 0;
  auto apply = [&](const NpgStep<T>& s) {
    const bool open0 = wide0 && (tanh || pg_below_one(s.a.a0));
    const bool open1 = wide1 && (tanh || pg_below_one(s.a.a1));
    n0 += open0 ? 1 : 0;
    n1 += open1 ? 1 : 0;
    const T xa = s.r[0];
#pragma unroll
    for (int e = 0; e < kCrProducts; ++e) {
      const T prod = (e <= rb ? xa : s.xb) * s.r[e];
      acc0[e] = open0 ? acc0[e] + prod : acc0[e];
      acc1[e] = open1 ? acc1[e] + prod : acc1[e];
    }
    sa0 = open0 ? sa0 + xa : sa0;
    sb0 = open0 ? sb0 + s.xb : sb0;
    sa1 = open1 ? sa1 + xa : sa1;
    sb1 = open1 ? sb1 + s.xb : sb1;
  };
  int k = len - 1;
  for (; k >= kCrMomSteps - 1; k -= kCrMomSteps) {
    NpgStep<T> s[kCrMomSteps];
#pragma unroll
    for (int i = 0; i < kCrMomSteps; ++i) s[i] = load(k - i);
#pragma unroll
    for (int i = 0; i < kCrMomSteps; ++i) apply(s[i]);
  }
  for (; k >= 0; --k) apply(load(k));

  // the division by sigma_j sigma_j (a component whose sigma is not > 0 never opened: its sums are 0 and stay 0)
  const T s20 = sig0 * sig0, s21 = sig1 * sig1;
  auto over0 = [&](T v) { return wide0 ? v / s20 : T(0); };
  auto over1 = [&](T v) { return wide1 ? v / s21 : T(0); };
#pragma unroll
  for (int e = 0; e < kCrProducts; ++e) {
    acc0[e] = over0(acc0[e]);
    acc1[e] = over1(acc1[e]);
  }
  sa0 = over0(sa0); sb0 = over0(sb0); sa1 = over1(sa1); sb1 = over1(sb1);
  const T corner0 = over0(T(n0)), corner1 = over1(T(n1));

  // the lane's verdict: the quotients this thread stores (a column at or above D saw zeros only, and is not asked)
  int fine = 1;
#pragma unroll
  for (int e = 0; e < kCrProducts; ++e) fine &= (slot(e) >= Dh || (steer_finite(acc0[e]) && steer_finite(acc1[e]))) ? 1 : 0;
  fine &= (ra >= Dh || (steer_finite(sa0) && steer_finite(sa1))) ? 1 : 0;
  fine &= (rb >= Dh || (steer_finite(sb0) && steer_finite(sb1))) ? 1 : 0;
  if (h == kCrPairs) fine &= (steer_finite(corner0) && steer_finite(corner1)) ? 1 : 0;
#pragma unroll
  for (int m = 1; m < kCrThreads; m *= 2) fine &= __shfl_xor(fine, m);

  // F[i][m], i <= m <= D, at i (D + 1) - i (i - 1) / 2 + (m - i); component 1 behind component 0
  const int n = D + 1, tri = n * (n + 1) / 2;
  T* const out0 = A.lane_mom + l;
  T* const out1 = A.lane_mom + (long long)tri * N + l;
  auto entry = [&](int i, int m) { return (long long)(i * n - i * (i - 1) / 2 + (m - i)) * N; };
#pragma unroll
  for (int e = 0; e < kCrProducts; ++e)
    if (slot(e) < Dh) {
      const long long at = entry(e <= rb ? ra : rb, slot(e));
      out0[at] = acc0[e];
      out1[at] = acc1[e];
    }
  if (ra < Dh) {
    out0[entry(ra, D)] = sa0;
    out1[entry(ra, D)] = sa1;
  }
  if (rb < Dh) {
    out0[entry(rb, D)] = sb0;
    out1[entry(rb, D)] = sb1;
  }
  if (h == kCrPairs) {
    out0[entry(D, D)] = corner0;
    out1[entry(D, D)] = corner1;
  }
  if (h == kCrThreads - 1) {
    A.lane_count[l] = len;
    A.lane_count[N + l] = n0;
    A.lane_count[2 * N + l] = n1;
    A.lane_count[3 * N + l] = fine;
  }
}

// Entry e of the sums of step 2 -> where its per-lane terms stand and where the policies' totals go: the 2 Tri entries of mom,
// then steps, open[0], open[1] and valid.  False: the total is not wanted.
template <typename T>
__device__ __forceinline__ bool npg_entry(const NpgArgs<T>& A, int e, PgEntry<T>& out) {
  const int n = A.D + 1, E = n * (n + 1);
  out.terms = nullptr; out.totals = nullptr; out.counts = nullptr; out.count_totals = nullptr;
  if (e < E) {
    out.terms = A.lane_mom + (long long)e * A.N;
    out.totals = A.mom + (long long)e * A.P;
    return true;
  }
  const int row = e - E;                                // of lane_count
  int* const totals = row == 0 ? A.steps : (row == 3 ? A.valid : (A.open ? A.open + (long long)(row - 1) * A.P : nullptr));
  if (!totals) return false;
  out.counts = A.lane_count + (long long)row * A.N;
  out.count_totals = totals;
  return true;
}

template <typename T>
__global__ __launch_bounds__(kPgChunks) void npg_sum_kernel(const NpgArgs<T> A) {
#pragma clang fp contract(off)
  PgEntry<T> E;
  if (!npg_entry(A, (int)blockIdx.y, E)) return;        // uniform over the workgroup
  const long long p = blockIdx.x;
  const int c = threadIdx.x;
  const int* const fine = A.lane_count + (kNpgIntegerSums - 1) * A.N;
  if (E.terms) {
    const T total = pg_wave_sum<T>(E.terms, fine, A.P, p, A.S, c);
    if (c == 0) E.totals[p] = total;
  } else {
    const int total = pg_wave_sum<int>(E.counts, fine, A.P, p, A.S, c);
    if (c == 0) E.count_totals[p] = total;
  }
}

template <typename T>
__global__ __launch_bounds__(kPgBlock) void npg_sum_few_kernel(const NpgArgs<T> A) {
#pragma clang fp contract(off)
  PgEntry<T> E;
  if (!npg_entry(A, (int)blockIdx.y, E)) return;
  const long long p = (long long)blockIdx.x * kPgBlock + threadIdx.x;
  if (p >= A.P) return;
  const int* const fine = A.lane_count + (kNpgIntegerSums - 1) * A.N;
  if (E.terms)
    E.totals[p] = pg_few_sum<T>(E.terms, fine, A.P, p, A.S);
  else
    E.count_totals[p] = pg_few_sum<int>(E.counts, fine, A.P, p, A.S);
}

// an integer total of policy p the caller did not ask the second launch for: the row's entries of its valid lanes, one after the
// other (an integer sum does not depend on its order)
__device__ __forceinline__ int npg_total(const int* __restrict__ row, const int* __restrict__ fine, long long P, long long p, int S) {
  int total = 0;
#pragma unroll 4
  for (int s = 0; s < S; ++s) {
    const long long l = (long long)s * P + p;
    total += fine[l] != 0 ? row[l] : 0;
  }
  return total;
}

template <typename T>
__global__ __launch_bounds__(kNpgSolveBlock) void npg_solve_kernel(const NpgArgs<T> A) {
#pragma clang fp contract(off)
  __shared__ T lds[kNpgSolveSlots * kNpgSolveBlock];
  const int t = threadIdx.x, j = t / kNpgSolvePolicies, other = t ^ kNpgSolvePolicies;
  const long long P = A.P, N = A.N, p = (long long)blockIdx.x * kNpgSolvePolicies + (t % kNpgSolvePolicies);
  const bool mine = p < P;                              // (every thread of the wave reaches the barrier)
  const int n = A.D + 1, tri = n * (n + 1) / 2;
  const T damping = A.damping, kl = A.kl;
  auto Lo = [&](int i, int m) -> T& { return lds[(i * (i + 1) / 2 + m) * kNpgSolveBlock + t]; };     // L[i][m], m <= i
  auto Z = [&](int i, int th) -> T& { return lds[(kCrTri + i) * kNpgSolveBlock + th]; };            // z, then d; slot n: d_ls
  const T* const mom = A.mom + (long long)j * tri * P + p;
  const T* const grad = A.grad + (long long)j * n * P + p;
  auto M = [&](int i, int m) { return mom[(long long)(i * n - i * (i - 1) / 2 + (m - i)) * P]; };   // i <= m

  int failed = 0, steps = 0;
  T c = T(0);
  if (mine) {
    const int* const fine = A.lane_count + (kNpgIntegerSums - 1) * N;
    steps = A.steps ? A.steps[p] : npg_total(A.lane_count, fine, P, p, A.S);
    c = T(steps);
    T dls = T(0);
    if (steps == 0) {
      failed = 1;
    } else {
      for (int m = 0; m < n; ++m) {
        T d = M(m, m) / c + damping;
        if (m > 0) {
          T st = Lo(m, 0) * Lo(m, 0);
          for (int q = 1; q < m; ++q) st = st + Lo(m, q) * Lo(m, q);
          d = d - st;
        }
        if (!cr_positive(d)) {
          failed = m + 1;
          break;
        }
        d = cr_sqrt(d);
        Lo(m, m) = d;
        for (int i = m + 1; i < n; ++i) {
          T u = M(m, i) / c;
          if (m > 0) {
            T su = Lo(i, 0) * Lo(m, 0);
            for (int q = 1; q < m; ++q) su = su + Lo(i, q) * Lo(m, q);
            u = u - su;
          }
          Lo(i, m) = u / d;
        }
      }
      if (A.lsig_grad) {
        const int nj = A.open ? A.open[(long long)j * P + p] : npg_total(A.lane_count + (long long)(1 + j) * N, fine, P, p, A.S);
        const T nn = T(nj);
        const T den = (nn + nn) / c + damping;
        if (cr_positive(den)) dls = (A.lsig_grad[(long long)j * P + p] / c) / den;
      }
    }
    if (failed != 0) {
      for (int i = 0; i < n; ++i) Z(i, t) = T(0);
    } else {
      for (int i = 0; i < n; ++i) {
        T rhs = grad[(long long)i * P] / c;
        if (i > 0) {
          T s = Lo(i, 0) * Z(0, t);
          for (int q = 1; q < i; ++q) s = s + Lo(i, q) * Z(q, t);
          rhs = rhs - s;
        }
        Z(i, t) = rhs / Lo(i, i);
      }
      for (int i = n - 1; i >= 0; --i) {                // d_l, l > i, stands where z_l stood
        T v = Z(i, t);
        if (i + 1 < n) {
          T s = Lo(i + 1, i) * Z(i + 1, t);
          for (int q = i + 2; q < n; ++q) s = s + Lo(q, i) * Z(q, t);
          v = v - s;
        }
        Z(i, t) = v / Lo(i, i);
      }
    }
    Z(n, t) = dls;
  }
  __syncthreads();
  if (!mine) return;

  // q, formed by both threads of the policy: component 0, component 1, then the two widths
  const int t0 = j == 0 ? t : other, t1 = j == 0 ? other : t;
  T q = T(0);
  if (steps != 0) {
    const T* const g0 = A.grad + p;
    q = (g0[0] / c) * Z(0, t0);
    for (int i = 1; i < n; ++i) q = q + (g0[(long long)i * P] / c) * Z(i, t0);
    for (int i = 0; i < n; ++i) q = q + (g0[(long long)(n + i) * P] / c) * Z(i, t1);
    if (A.lsig_grad) {
      q = q + (A.lsig_grad[p] / c) * Z(n, t0);
      q = q + (A.lsig_grad[P + p] / c) * Z(n, t1);
    }
  }
  const bool good = cr_positive(q);
  T beta = T(0);
  if (good) beta = A.unit ? T(1) : cr_sqrt((kl + kl) / q);

  for (int i = 0; i < n; ++i) {
    const T d = Z(i, t);
    A.step[((long long)j * n + i) * P + p] = beta * d;
    if (A.dir) A.dir[((long long)j * n + i) * P + p] = d;
  }
  if (A.lsig_step) A.lsig_step[(long long)j * P + p] = beta * Z(n, t);
  if (A.failed) A.failed[(long long)j * P + p] = failed;
  if (j == 0) {
    if (A.beta) A.beta[p] = beta;
    if (A.quad) A.quad[p] = q;
    if (A.failed) A.failed[2 * P + p] = good ? 0 : 1;
  }
}

// the three launches (os2r_npg_inst.hip, once per dtype)
template <typename T>
void launch_natural_step(const NpgArgs<T>& args, hipStream_t stream);

}  // namespace os2r
