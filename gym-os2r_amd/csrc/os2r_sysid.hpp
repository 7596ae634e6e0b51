// os2r_sysid.hpp — os2ri_perturb and os2ri_update: finite-difference Gauss-Newton / Levenberg-Marquardt identification of the
// per-environment parameters of many robots (gfx950).
//
// sysid_perturb_kernel, grid ceil(F N / 256): a thread per (row, lane) of the packed parameters, the lane index fastest, so a
// wave stores one contiguous span.  The row's parameter, if it is an identified one, is found by walking the P rows of the
// argument block.
// sysid_segment_kernel, grid ceil(M / 64), ceil(P / 2) waves each: lane l of every wave is segment 64 b + l, and wave v owns the
// rows v and P - 1 - v of the triangle G (the middle wave of an odd P its one row), so every thread holds P + 1 chains of G, its
// two of b and, in wave 0, c: at most 25.  The triangle's loops run over a compile-time q under a test that is uniform over the
// wave: no lane indexes a register array at run time and no lane is masked off.  The differences d_p of a (k, d) term are formed
// once, by the wave that owns row p, and shared through LDS: a tile holds the d_p of kSysidTile / (64 P) slots of one step (all
// twelve up to P = 5, three at P = 21), wave 0 adds the nominal residual and the verdict on the reading, and behind the barrier
// every wave walks the tile.  obs is [K][N][D] with D fastest: a wave reads, per lane of the rollout, 64 neighbouring segments.
// The sums go out as [E][M], the segment fastest, which is what the second launch reads.
// sysid_sum_kernel (M / T > 64), grid (T, E + 1), one wave each, and sysid_sum_few_kernel (M / T <= 64), grid (ceil(T / 256),
// E + 1), one thread each: the 64 partials and the adjacent-pair tree of os2r_pg.hpp, the included body (pg_wave_sum, pg_few_sum)
// with the set in the place of the policy and the segment in the place of the sample; row E sums the verdicts themselves, the
// valid segments of the set.  One set of thousands of segments is E + 1 independent waves, not one workgroup.
// sysid_step_kernel, grid T, one wave each: lane i is row i of the set's system.  The totals meet in LDS, the lanes form H and g,
// the verdict and the new lam are formed by every lane alike, and the damped system is factored by columns: lane i >= j forms
// A[i][j] - sum L[i][k] L[j][k], lane j's value is handed round, tested on its bits and rooted, the lanes below divide.  Both
// substitutions run by columns as well, which leaves every lane's chain in the order of the contract.
// No lane indexes a register array at run time, nothing goes to scratch (tests/test_sysid_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_sysid.h: the layout's dtype, no contraction, every chain in the order given
// there.  tests/sysid_ref.py restates it in numpy; tests/test_gpu_sysid.py compares bit for bit.
#pragma once
#include "os2r_pg.hpp"                 // pg_wave_sum, pg_few_sum; through it os2r_bits.hpp
#include "../../include/os2r_sysid.h"

namespace os2r {

constexpr int kSysidMaxP = OS2RI_MAX_PARAMS;
constexpr int kSysidLanes = OS2RI_CHUNKS;                        // segments of a workgroup of the segment kernel: the lanes of a wave
constexpr int kSysidMaxWaves = (kSysidMaxP + 1) / 2;             // 11 row pairs
constexpr int kSysidRowsA = kSysidMaxP / 2;                      // rows 0..9 can be the lower row of a pair
constexpr int kSysidTile = kSysidMaxP * 3 * kSysidLanes;         // elements of the tile of differences: three slots at P = 21
constexpr int kSysidMaxSums = kSysidMaxP * (kSysidMaxP + 1) / 2 + kSysidMaxP + 1;   // 253
constexpr int kSysidBlock = 256;                                 // threads of a workgroup of the perturb and few-segments kernels
static_assert(kSysidLanes == 64 && kSysidLanes == kPgChunks, "a partial is a lane of a wave");
static_assert(kSysidMaxWaves * kSysidLanes <= 1024, "the row pairs of a segment are one workgroup");

template <typename T>
struct SysidArgs {
  const T* __restrict__ theta;        // [T][P]
  const T* __restrict__ base;         // [F][M]            (perturb)
  T* __restrict__ params;             // [F][N]            (perturb)
  const T* __restrict__ obs;          // [K][N][D]
  const T* __restrict__ meas;         // [K][M][D]
  const unsigned char* __restrict__ done;   // [K][N] or null
  const T* __restrict__ prec;         // [D]
  const T* __restrict__ theta_best;   // [T][P]
  const T* __restrict__ cost_best;    // [T]
  const T* __restrict__ hess;         // [T][P][P]
  const T* __restrict__ grad;         // [T][P]
  const T* __restrict__ lam;          // [T]
  const int* __restrict__ status;     // [T]
  const int* __restrict__ iters;      // [T]
  T* __restrict__ theta_best_out;
  T* __restrict__ cost_best_out;
  T* __restrict__ hess_out;
  T* __restrict__ grad_out;
  T* __restrict__ lam_out;
  int* __restrict__ status_out;
  int* __restrict__ iters_out;
  T* __restrict__ theta_next;         // [T][P]
  T* __restrict__ cost;               // [T] or null
  int* __restrict__ valid;            // [T] or null
  unsigned char* __restrict__ accepted;   // [T] or null
  int* __restrict__ failed;           // [T] or null
  T* __restrict__ delta;              // [T][P] or null
  T* sums;                            // [E][M] and behind it [E][T]: written by one launch, read by the next
  int* counts;                        // [M] and behind it [T]: likewise
  long long sets, M;                  // T, M
  int P, K, D, F;
  int row[kSysidMaxP];                // of the packed parameters
  T h[kSysidMaxP], lo[kSysidMaxP], hi[kSysidMaxP];                     // rounded by the host
  T shrink, grow, lam_min, lam_max, diag_floor, tol, cost_floor;       // likewise
};

// finite and > 0, on the bits (os2r_bits.hpp says why)
__device__ __forceinline__ bool sysid_positive(float x) {
  const unsigned b = steer_bits(x);
  return (b >> 31) == 0u && (b >> 23 & 0xffu) != 0xffu && b != 0u;
}
__device__ __forceinline__ bool sysid_positive(double x) {
  const unsigned long long b = steer_bits(x);
  return (b >> 63) == 0ull && (b >> 52 & 0x7ffull) != 0x7ffull && b != 0ull;
}
// a zero of either sign
__device__ __forceinline__ bool sysid_zero(float x) { return (steer_bits(x) & 0x7fffffffu) == 0u; }
__device__ __forceinline__ bool sysid_zero(double x) { return (steer_bits(x) & 0x7fffffffffffffffull) == 0ull; }
__device__ __forceinline__ float sysid_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double sysid_sqrt(double x) { return __builtin_sqrt(x); }
__device__ __forceinline__ float sysid_negate(float x) { return __int_as_float(__float_as_int(x) ^ (int)0x80000000u); }
__device__ __forceinline__ double sysid_negate(double x) { return __longlong_as_double(__double_as_longlong(x) ^ (long long)0x8000000000000000ull); }

// The kernel's own argument block, read where it is used and indexed at run time: a load from the kernel-argument segment, where
// an index into the by-value copy would make a private array of it.
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(4))) SysidArgs<T>* sysid_args() {
  auto* p = (const __attribute__((address_space(4))) SysidArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// the two points of a parameter about theta, with the operations of the contract
template <typename T>
__device__ __forceinline__ T sysid_plus(T th, T h, T hi) {
#pragma clang fp contract(off)
  const T v = th + h;
  return v > hi ? hi : v;
}
template <typename T>
__device__ __forceinline__ T sysid_minus(T th, T h, T lo) {
#pragma clang fp contract(off)
  const T v = th - h;
  return v < lo ? lo : v;
}

template <typename T>
__global__ __launch_bounds__(kSysidBlock) void sysid_perturb_kernel(const SysidArgs<T> A) {
#pragma clang fp contract(off)
  const auto* const L = sysid_args<T>();
  const long long M = A.M, N = (long long)(2 * A.P + 1) * M;
  const long long gid = (long long)blockIdx.x * kSysidBlock + threadIdx.x;
  if (gid >= (long long)A.F * N) return;
  const int r = (int)(gid / N);
  const long long n = gid % N, m = n % M;
  const int s = (int)(n / M), P = A.P;
  T v = A.base[(long long)r * M + m];
  for (int p = 0; p < P; ++p) {
    if (L->row[p] != r) continue;
    const T th = A.theta[(m % A.sets) * P + p];
    v = s == 1 + p ? sysid_plus<T>(th, L->h[p], L->hi[p]) : (s == 1 + P + p ? sysid_minus<T>(th, L->h[p], L->lo[p]) : th);
  }
  A.params[gid] = v;
}

template <typename T>
__global__ __launch_bounds__(kSysidMaxWaves * kSysidLanes) void sysid_segment_kernel(const SysidArgs<T> A) {
#pragma clang fp contract(off)
  __shared__ T sD[kSysidTile];                          // the differences of a tile, [p][slot of the tile][lane]
  __shared__ T sR[OS2R_MAX_OBS * kSysidLanes];          // the nominal residual r, [slot][lane]
  __shared__ T sWR[OS2R_MAX_OBS * kSysidLanes];         // w r
  __shared__ int sUse[OS2R_MAX_OBS * kSysidLanes];      // the reading arrived and its slot is kept
  __shared__ int sBad[kSysidLanes];
  const int lane = (int)threadIdx.x % kSysidLanes;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kSysidLanes);   // (so that what follows from it is known to be uniform)
  const int P = A.P, K = A.K, D = A.D;
  const long long M = A.M, N = (long long)(2 * P + 1) * M;
  const long long seg = (long long)blockIdx.x * kSysidLanes + lane;
  const bool live = seg < M;
  const long long m = live ? seg : M - 1;               // (a lane behind the last segment reads the last one and stores nothing)
  const int rowB = P - 1 - wave, rowA = wave;
  const bool hasA = rowA < rowB;                        // (uniform over the wave)
  int tile = kSysidTile / (P * kSysidLanes);
  tile = tile > D ? D : tile;
  const long long laneBp = (long long)(1 + rowB) * M + m, laneBm = (long long)(1 + P + rowB) * M + m;
  const long long laneAp = (long long)(1 + rowA) * M + m, laneAm = (long long)(1 + P + rowA) * M + m;

  T gA[kSysidRowsA], gB[kSysidMaxP];
#pragma unroll
  for (int q = 0; q < kSysidRowsA; ++q) gA[q] = T(0);
#pragma unroll
  for (int q = 0; q < kSysidMaxP; ++q) gB[q] = T(0);
  T bA = T(0), bB = T(0), c = T(0);
  int bad = 0;
  if (wave == 0) sBad[lane] = 0;

  for (int k = 0; k < K; ++k) {                         // (uniform over the workgroup: every thread reaches every barrier)
    const long long step = (long long)k * N;
    if (A.done) {
      bad |= A.done[step + laneBp] | A.done[step + laneBm];
      if (hasA) bad |= A.done[step + laneAp] | A.done[step + laneAm];
      if (wave == 0) bad |= A.done[step + m];
    }
    for (int d0 = 0; d0 < D; d0 += tile) {
      const int here = D - d0 < tile ? D - d0 : tile;
      for (int dd = 0; dd < here; ++dd) {
        const int d = d0 + dd;
        sD[(rowB * tile + dd) * kSysidLanes + lane] = A.obs[(step + laneBp) * D + d] - A.obs[(step + laneBm) * D + d];
        if (hasA) sD[(rowA * tile + dd) * kSysidLanes + lane] = A.obs[(step + laneAp) * D + d] - A.obs[(step + laneAm) * D + d];
        if (wave == 0) {
          const T y = A.meas[((long long)k * M + m) * D + d], w = A.prec[d];
          const T r = A.obs[(step + m) * D + d] - y;
          sR[dd * kSysidLanes + lane] = r;
          sWR[dd * kSysidLanes + lane] = w * r;
          sUse[dd * kSysidLanes + lane] = (sysid_positive(w) && steer_finite(y)) ? 1 : 0;
        }
      }
      __syncthreads();
      for (int dd = 0; dd < here; ++dd) {
        // (the row numbers as this round's own scalars: compared against every q ahead of the loops, the verdicts would be held
        // in thirty scalar registers across them)
        int rb = rowB, ra = rowA;
        asm volatile("" : "+s"(rb), "+s"(ra));
        const bool use = sUse[dd * kSysidLanes + lane] != 0;
        const T w = A.prec[d0 + dd];
        const T r = sR[dd * kSysidLanes + lane];
        const T* const col = sD + dd * kSysidLanes + lane;              // d_q at col[q tile 64]
        const T wdB = w * col[rowB * tile * kSysidLanes];
        const T nbB = bB + wdB * r;
        bB = use ? nbB : bB;
#pragma unroll
        for (int q = 0; q < kSysidMaxP; ++q)
          if (q <= rb) {                                // (uniform)
            const T next = gB[q] + wdB * col[q * tile * kSysidLanes];
            gB[q] = use ? next : gB[q];
          }
        if (hasA) {
          const T wdA = w * col[rowA * tile * kSysidLanes];
          const T nbA = bA + wdA * r;
          bA = use ? nbA : bA;
#pragma unroll
          for (int q = 0; q < kSysidRowsA; ++q)
            if (q <= ra) {
              const T next = gA[q] + wdA * col[q * tile * kSysidLanes];
              gA[q] = use ? next : gA[q];
            }
        }
        if (wave == 0) {
          const T nc = c + sWR[dd * kSysidLanes + lane] * r;
          c = use ? nc : c;
        }
      }
      __syncthreads();
    }
  }

  // step 2: every sum this thread owns is finite, and no lane of the segment it read was done
  bad |= (steer_finite(bB) && (!hasA || steer_finite(bA)) && (wave != 0 || steer_finite(c))) ? 0 : 1;
#pragma unroll
  for (int q = 0; q < kSysidMaxP; ++q)
    if (q <= rowB) bad |= steer_finite(gB[q]) ? 0 : 1;
#pragma unroll
  for (int q = 0; q < kSysidRowsA; ++q)
    if (hasA && q <= rowA) bad |= steer_finite(gA[q]) ? 0 : 1;
  if (bad != 0) sBad[lane] = 1;                         // (every writer writes the same)
  __syncthreads();
  if (!live) return;
  T* const out = A.sums + m;
  out[(long long)(1 + rowB) * M] = bB;
#pragma unroll
  for (int q = 0; q < kSysidMaxP; ++q)
    if (q <= rowB) out[(long long)(1 + P + rowB * (rowB + 1) / 2 + q) * M] = gB[q];
  if (hasA) {
    out[(long long)(1 + rowA) * M] = bA;
#pragma unroll
    for (int q = 0; q < kSysidRowsA; ++q)
      if (q <= rowA) out[(long long)(1 + P + rowA * (rowA + 1) / 2 + q) * M] = gA[q];
  }
  if (wave == 0) {
    out[0] = c;
    A.counts[m] = sBad[lane] != 0 ? 0 : 1;
  }
}

// Row e < E of the second launch: the sum e of every set; row E: the valid segments of every set
template <typename T>
__global__ __launch_bounds__(kPgChunks) void sysid_sum_kernel(const SysidArgs<T> A) {
#pragma clang fp contract(off)
  const long long t = blockIdx.x, sets = A.sets, M = A.M;
  const int e = (int)blockIdx.y, E = A.P * (A.P + 1) / 2 + A.P + 1, Q = (int)(M / sets), c = threadIdx.x;
  const int* const fine = A.counts;
  if (e < E) {
    const T total = pg_wave_sum<T>(A.sums + (long long)e * M, fine, sets, t, Q, c);
    if (c == 0) A.sums[(long long)E * M + (long long)e * sets + t] = total;
  } else {
    const int total = pg_wave_sum<int>(fine, fine, sets, t, Q, c);
    if (c == 0) A.counts[M + t] = total;
  }
}

template <typename T>
__global__ __launch_bounds__(kSysidBlock) void sysid_sum_few_kernel(const SysidArgs<T> A) {
#pragma clang fp contract(off)
  const long long sets = A.sets, M = A.M;
  const long long t = (long long)blockIdx.x * kSysidBlock + threadIdx.x;
  if (t >= sets) return;
  const int e = (int)blockIdx.y, E = A.P * (A.P + 1) / 2 + A.P + 1, Q = (int)(M / sets);
  const int* const fine = A.counts;
  if (e < E)
    A.sums[(long long)E * M + (long long)e * sets + t] = pg_few_sum<T>(A.sums + (long long)e * M, fine, sets, t, Q);
  else
    A.counts[M + t] = pg_few_sum<int>(fine, fine, sets, t, Q);
}

template <typename T>
__global__ __launch_bounds__(kSysidLanes) void sysid_step_kernel(const SysidArgs<T> A) {
#pragma clang fp contract(off)
  __shared__ T sTot[kSysidMaxSums];
  __shared__ T sA[kSysidMaxP * kSysidMaxP];
  __shared__ T sDelta[kSysidMaxP];
  const auto* const L = sysid_args<T>();
  const long long t = blockIdx.x, sets = A.sets, M = A.M;
  const int lane = threadIdx.x, P = A.P, E = P * (P + 1) / 2 + P + 1;
  const bool row = lane < P;
  const int st = A.status[t], nv = A.counts[M + t], it = A.iters[t];
  const T old = A.cost_best[t], lam = A.lam[t];
  const T th = row ? A.theta[t * P + lane] : T(0), best = row ? A.theta_best[t * P + lane] : T(0);
  if (st != 0 || nv == 0) {                             // (uniform) the state as it was
    for (int at = lane; at < P * P; at += kSysidLanes) A.hess_out[t * P * P + at] = A.hess[t * P * P + at];
    if (row) {
      A.theta_best_out[t * P + lane] = best;
      A.grad_out[t * P + lane] = A.grad[t * P + lane];
      A.theta_next[t * P + lane] = st != 0 ? best : th;
      if (A.delta) A.delta[t * P + lane] = T(0);
    }
    if (lane == 0) {
      A.cost_best_out[t] = old;
      A.lam_out[t] = lam;
      A.status_out[t] = st;
      A.iters_out[t] = it;
      if (A.cost) A.cost[t] = old;
      if (A.valid) A.valid[t] = nv;
      if (A.accepted) A.accepted[t] = 0;
      if (A.failed) A.failed[t] = 0;
    }
    return;
  }
  const T* const tot = A.sums + (long long)E * M + t;
  for (int e = lane; e < E; e += kSysidLanes) sTot[e] = tot[(long long)e * sets];
  const T h = row ? L->h[lane] : T(1), lo = row ? L->lo[lane] : T(0), hi = row ? L->hi[lane] : T(0);
  const T Delta = sysid_plus<T>(th, h, hi) - sysid_minus<T>(th, h, lo);
  if (row) sDelta[lane] = Delta;
  __syncthreads();
  // steps 4 and 5
  const T J = sTot[0] / T(2);
  const bool accept = steer_bits(J) < steer_bits(old);
  const bool held = sysid_zero(Delta);
  if (accept) {
    if (row) {
      for (int q = 0; q <= lane; ++q) {
        const T den = Delta * sDelta[q];
        T v = sTot[1 + P + lane * (lane + 1) / 2 + q] / den;
        if (held || sysid_zero(sDelta[q])) v = q == lane ? T(1) : T(0);
        sA[lane * P + q] = v;
        sA[q * P + lane] = v;
      }
    }
  } else {
    for (int at = lane; at < P * P; at += kSysidLanes) sA[at] = A.hess[t * P * P + at];
  }
  T g = T(0);
  if (row) g = accept ? (held ? T(0) : sTot[1 + lane] / Delta) : A.grad[t * P + lane];
  T next_lam;
  int status = 0;
  if (accept) {
    next_lam = lam * A.shrink;
    next_lam = next_lam < A.lam_min ? A.lam_min : next_lam;
    const T drop = old - J, bound = A.tol * old;
    if (J <= A.cost_floor || (steer_finite(old) && drop <= bound)) status = 1;
  } else {
    next_lam = lam * A.grow;
    if (next_lam > A.lam_max) status = 2;
  }
  const T base = accept ? th : best;
  __syncthreads();
  for (int at = lane; at < P * P; at += kSysidLanes) A.hess_out[t * P * P + at] = sA[at];
  if (row) {
    A.theta_best_out[t * P + lane] = base;
    A.grad_out[t * P + lane] = g;
  }
  if (lane == 0) {
    A.cost_best_out[t] = accept ? J : old;
    A.lam_out[t] = next_lam;
    A.status_out[t] = status;
    A.iters_out[t] = it + 1;
    if (A.cost) A.cost[t] = J;
    if (A.valid) A.valid[t] = nv;
    if (A.accepted) A.accepted[t] = accept ? 1 : 0;
  }
  __syncthreads();
  // step 6: the damped diagonal, the factor by columns, the two substitutions by columns
  if (row) {
    const T hpp = sA[lane * P + lane];
    const T big = hpp < A.diag_floor ? A.diag_floor : hpp;
    const T add = next_lam * big;
    sA[lane * P + lane] = hpp + add;
  }
  __syncthreads();
  int failed = 0;
  for (int j = 0; j < P; ++j) {                         // (uniform: `failed` is the same in every lane)
    T acc = T(0);
    const bool mine = lane >= j && row;
    if (mine) {
      acc = sA[lane * P + j];
      for (int k = 0; k < j; ++k) acc = acc - sA[lane * P + k] * sA[j * P + k];
    }
    const T diag = __shfl(acc, j);
    if (!sysid_positive(diag)) {
      failed = j + 1;
      break;
    }
    const T root = sysid_sqrt(diag);
    if (mine) sA[lane * P + j] = lane == j ? root : acc / root;    // (its own entry: no other lane read it in this column)
    __syncthreads();
  }
  T step = T(0);
  if (failed == 0) {
    const T pivot = row ? sA[lane * P + lane] : T(1);
    T acc = sysid_negate(g), y = T(0);
    for (int j = 0; j < P; ++j) {
      T mine = T(0);
      if (lane == j) mine = acc / pivot;                // (the one quotient of the round)
      const T yj = __shfl(mine, j);
      y = lane == j ? yj : y;
      if (row && lane > j) acc = acc - sA[lane * P + j] * yj;
    }
    acc = y;
    for (int j = P - 1; j >= 0; --j) {
      T mine = T(0);
      if (lane == j) mine = acc / pivot;
      const T xj = __shfl(mine, j);
      step = lane == j ? xj : step;
      if (lane < j) acc = acc - sA[j * P + lane] * xj;
    }
  }
  if (row) {
    T next = base + step;
    next = next < lo ? lo : next;
    next = next > hi ? hi : next;
    A.theta_next[t * P + lane] = next;
    if (A.delta) A.delta[t * P + lane] = step;
  }
  if (lane == 0 && A.failed) A.failed[t] = failed;
}

// the launches of the two calls (os2r_sysid_inst.hip, once per dtype)
template <typename T>
void launch_sysid_perturb(const SysidArgs<T>& args, hipStream_t stream);
template <typename T>
void launch_sysid_update(const SysidArgs<T>& args, hipStream_t stream);

}  // namespace os2r
