// os2r_ukf.hpp — os2ru_ukf_points and os2ru_ukf_update: the unscented Kalman filter of many robots, two launches (gfx950).
//
// Both kernels have the arrangement of the Kalman update of the sibling library (os2r_ekf.hpp): one robot per n lanes, n = 2 nq,
// the grid ceil(M / 32) workgroups, a workgroup kUkfRobots = 32 robots x n lanes, thread (lane c, robot e) = c * 32 + e: the 32
// threads of one c read and write 32 consecutive elements of the robot-fastest arrays, and LDS arrays are [.][.][e]
// (conflict-free).  Tail threads shadow the last robot and their stores are masked.  Verdicts (failed, lost, a slot's apply)
// mask work and never branch round a barrier; what branches round one is uniform over the grid (a kernel argument).
//
// The factor (ukf_factor_points, shared by both kernels, so step 4 of the update has the bits of a separate points launch):
// thread c owns row c of L in registers and holds P[j][c], j <= c, the column of the upper triangle that is row c of the lower.
// Column j: every thread of a robot reads row j of L (l < j, written in the columns before) and P[j][j] from LDS and forms the
// pivot t, its verdict and sqrt(t) itself -- j products more per thread than publishing the pivot would cost, and one barrier
// per column where publishing it needs two; thread c forms L[c][j], stores it to LDS, barrier.  n barriers per factor (one for
// the diagonal, none behind the last column).  The thread's own diagonal entry P[c][c] is read on its own, from global memory
// or LDS: no lane indexes a register array at run time.  Then thread c stores row c of the S points, S runs of 32 robots.
//
// The update:
//   prologue   thread c reads row c of the S points of its robot (S coalesced loads, kept in registers: 21 values with nq = 5),
//              its share of the done flags and the measurements; Q comes from the argument segment.  Column c of the symmetric
//              p_in, which only a lost robot uses, is read behind the covariance, where the points' registers are free.  Every
//              global input of the workgroup is read before its first store: that lets p_out be p_in
//   lost       thread c publishes "a lane of mine is done or not finite"; barrier; every thread of a robot ORs the n flags
//   mean       in registers: acc, xbar, then the deviations d_s in the place of the points
//   covariance the deviations stream through LDS four points at a time, in two buffers that alternate, so that a chunk costs one
//              barrier: publish d_s[c] of the chunk, barrier, accumulate P-[i][c] += d_s[i] d_s[c] for every i from LDS.  d_0 has
//              a buffer of its own and travels with the first chunk.  Holding every deviation of the workgroup at once would be
//              S n 32 sizeof(T) = 53 760 bytes in fp64 with nq = 5 beside P; the chunks take 9 n 32 sizeof(T) and lie where P
//              goes afterwards (one barrier more), so with nq = 5 they add nothing.  One point per barrier was the other
//              candidate: 2n barriers of n multiply-adds each, against n / 2 with the chunks
//   slots      the slot loop of ekf_update_kernel (os2r_ekf.hpp), a copy of its text: that loop is part of a kernel body, not a
//              function, and os2r_ekf.hpp stays as it is.  DESIGN.md section 4 ("Both are copies because one text measured
//              slower") records why such bodies stay copies; a change to one text is made in the other.  It gives the bits of
//              the sibling on the same x and P-
//   epilogue   x_out, p_out, nis, used, refused, lost; then, with points_out (a kernel argument), a barrier and the factor in the
//              LDS that held P and k
// LDS of a workgroup, static, no dynamic LDS.  ukf_points_kernel: (n n + n) 32 sizeof(T) bytes -- 28160 for double and nq = 5.
// ukf_update_kernel: ((max(n n, 9 n) + 2 n + 12) 32 + n n + 12) sizeof(T) + (32 n + 12) * 4 bytes -- 36016 for double and nq = 5:
// four workgroups fit the 160 KiB of a CU.
// What the build gave (code-object metadata; outcomes, not targets): no scratch, no spill, no AGPRs; with nq = 5,
// ukf_points_kernel 54 registers in fp64 and 37 in fp32, five workgroups of five waves on a CU by its LDS; ukf_update_kernel 102
// and 68, in fp64 four waves on a SIMD and so three workgroups on a CU, in fp32 five.  DESIGN.md section 4 has the measurements.
// The arithmetic is the contract of include/os2r_ukf.h: the layout's dtype, no contraction, sums from the left.
// tests/test_ukf_host.py restates it in numpy and reads the resources from the metadata; tests/test_gpu_ukf.py compares bit for bit.
#pragma once
#include "os2r_lqr.hpp"   // by_chain_length, OS2R_CONST
#include "os2r_bits.hpp"
#include "../../include/os2r_ukf.h"

namespace os2r {

constexpr int kUkfRobots = 32;                 // robots of one workgroup
constexpr int kUkfMaxN = 2 * OS2R_MAX_DOF;
constexpr int kUkfObs = OS2R_MAX_OBS;
constexpr int kUkfChunk = 4;                   // points of one chunk of deviations; divides 2n for every nq
constexpr int kUkfWavesPerSimd = 4;            // at most 128 registers (five: the fp64 update with nq = 5 spills seven)

template <typename T>
struct UkfPointsArgs {
  const T* __restrict__ x;         // [n][M]
  const T* __restrict__ p;         // [n][n][M], upper triangle read
  T* __restrict__ points;          // [n][S M]
  int* __restrict__ failed;        // [M] or null
  long long M;
  T gamma;                         // rounded to T by the host
};

template <typename T>
struct UkfArgs {
  const T* __restrict__ q;         // [nq][S M]
  const T* __restrict__ qd;        // [nq][S M]
  const unsigned char* __restrict__ done;   // [S M] or null
  const T* p_in;                   // [n][n][M], upper triangle read; p_out may be this very pointer
  const T* __restrict__ meas;      // [M][D]
  const T* __restrict__ prec;      // [D]
  T* __restrict__ x_out;           // [n][M]
  T* p_out;                        // [n][n][M]
  T* __restrict__ nis;             // [M] or null
  int* __restrict__ used;          // [M] or null
  int* __restrict__ refused;       // [M] or null
  T* __restrict__ innov;           // [M][D] or null
  int* __restrict__ lost;          // [M] or null
  T* __restrict__ points;          // [n][S M] or null
  int* __restrict__ failed;        // [M] or null
  long long M;
  int D;
  int slot_col[kUkfObs];           // state column a raw observation slot shows, -1: none
  T gate, gamma, wm0, wc0, wi;     // rounded to T by the host; gate 0: no gate
  T qn[kUkfMaxN * kUkfMaxN];       // the process noise [n][n] row-major, rounded to T by the host
};

// finite and > 0, on the bits (os2r_bits.hpp says why): neither negative nor not finite, and no zero
__device__ __forceinline__ bool ukf_positive(float x) { return !steer_invalid(x) && (steer_bits(x) & 0x7fffffffu) != 0u; }
__device__ __forceinline__ bool ukf_positive(double x) { return !steer_invalid(x) && (steer_bits(x) & 0x7fffffffffffffffull) != 0ull; }
// one correctly rounded IEEE square root (in fp32 __fsqrt_rn is a bare v_sqrt_f32, 1 ulp; the builtin gets the fix-up sequence)
__device__ __forceinline__ float ukf_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double ukf_sqrt(double x) { return __builtin_sqrt(x); }

// The factor of one robot's P and its S points, by the n threads of the robot (thread c, robot e of the workgroup).  pcol[j],
// j <= c, is P[j][c]; what it holds for j > c is not used.  diag is P[c][c]: handed over beside the column, because a chain of
// selects that picks pcol[c] is compiled into a run-time index, and the column into scratch.  sL [n][n][e] and sDiag [n][e] are
// LDS nobody else reads or writes from the call on.  Every thread of the workgroup calls it: it holds barriers.
template <typename T, int n>
__device__ __forceinline__ void ukf_factor_points(const T x, const T diag, const T (&pcol)[n], const T gamma, T* const sL,
                                                  T* const sDiag, const int c, const int e, const long long m, const long long M, const bool valid,
                                                  T* const __restrict__ points, int* const __restrict__ failed_out) {
#pragma clang fp contract(off)
  constexpr int E = kUkfRobots, S = 2 * n + 1;
  sDiag[c * E + e] = diag;
  __syncthreads();
  T li[n];                                              // row c of L
  int failed = 0;
#pragma unroll
  for (int j = 0; j < n; ++j) {
    T t = sDiag[j * E + e], u = pcol[j];
    if (j > 0) {
      const T r0 = sL[(j * n + 0) * E + e];
      T st = r0 * r0, su = li[0] * r0;
#pragma unroll
      for (int l = 1; l < j; ++l) {
        const T r = sL[(j * n + l) * E + e];
        st = st + r * r;
        su = su + li[l] * r;
      }
      t = t - st;
      u = u - su;
    }
    failed = failed == 0 && !ukf_positive(t) ? j + 1 : failed;   // the same in every thread of the robot
    const T d = ukf_sqrt(t);
    const T v = u / d;
    li[j] = c < j ? T(0) : (c == j ? d : v);
    if (j + 1 < n) {
      sL[(c * n + j) * E + e] = li[j];
      __syncthreads();
    }
  }
  if (valid) {
    const bool ok = failed == 0;
    T* const row = points + (long long)c * S * M + m;
    row[0] = x;
#pragma unroll
    for (int j = 0; j < n; ++j) {
      const T g = gamma * li[j];
      const T up = x + g, down = x - g;
      row[(long long)(1 + j) * M] = ok ? up : x;
      row[(long long)(1 + n + j) * M] = ok ? down : x;
    }
    if (failed_out && c == 0) failed_out[m] = failed;
  }
}

template <typename T, int NQ>
__global__ __launch_bounds__(kUkfRobots * 2 * NQ, kUkfWavesPerSimd) void ukf_points_kernel(const UkfPointsArgs<T> P) {
#pragma clang fp contract(off)
  constexpr int n = 2 * NQ, E = kUkfRobots;
  __shared__ T sL[n * n * E], sDiag[n * E];
  const int e = threadIdx.x % E, c = threadIdx.x / E;
  const long long M = P.M, m_raw = (long long)blockIdx.x * E + e;
  const bool valid = m_raw < M;
  const long long m = valid ? m_raw : M - 1;
  const T x = P.x[(long long)c * M + m];
  T pcol[n];
#pragma unroll
  for (int l = 0; l < n; ++l) pcol[l] = P.p[(long long)((l <= c ? l : c) * n + c) * M + m];   // (below the diagonal: not used)
  const T diag = P.p[(long long)(c * n + c) * M + m];
  ukf_factor_points<T, n>(x, diag, pcol, P.gamma, sL, sDiag, c, e, m, M, valid, P.points, P.failed);
}

template <typename T, int NQ>
__global__ __launch_bounds__(kUkfRobots * 2 * NQ, kUkfWavesPerSimd) void ukf_update_kernel(const UkfArgs<T> P) {
#pragma clang fp contract(off)
  constexpr int n = 2 * NQ, E = kUkfRobots, S = 2 * n + 1, CH = kUkfChunk;
  constexpr int kMat = n * n > (1 + 2 * CH) * n ? n * n : (1 + 2 * CH) * n;
  static_assert((2 * n) % CH == 0, "the chunks cover the points 1..2n");
  __shared__ T sM[kMat * E], sX[n * E], sK[n * E], sY[kUkfObs * E], sR[kUkfObs], sQ[n * n];
  __shared__ int sDrop[kUkfObs], sFlag[n * E];
  T* const sD0 = sM;                // [n][e]: the deviation of point 0
  T* const sDv = sM + n * E;        // [2][CH][n][e]: the chunks, until P- is formed
  T* const sP = sM;                 // [n][n][e], from then on
  const int e = threadIdx.x % E, c = threadIdx.x / E;   // c is uniform over a half-wave
  const long long M = P.M, m_raw = (long long)blockIdx.x * E + e;
  const bool valid = m_raw < M;
  const long long m = valid ? m_raw : M - 1;            // tail threads shadow the last robot, their stores are masked
  const int D = P.D;
  // (what is read with a run-time index comes from the argument segment as memory, not from a copy of the struct)
  const OS2R_CONST UkfArgs<T>* ka = (const OS2R_CONST UkfArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();

  // prologue: every global input of this workgroup
  if ((int)threadIdx.x < n * n) sQ[threadIdx.x] = ka->qn[threadIdx.x];
  if ((int)threadIdx.x < kUkfObs) {
    const T pr = P.prec[(int)threadIdx.x < D ? (int)threadIdx.x : D - 1];
    sDrop[threadIdx.x] = ukf_positive(pr) ? 0 : 1;
    sR[threadIdx.x] = T(1) / pr;
  }
  for (int d = c; d < D; d += n) sY[d * E + e] = P.meas[m * D + d];
  const T* const row = (c < NQ ? P.q + (long long)c * S * M : P.qd + (long long)(c - NQ) * S * M) + m;
  T chi[S];
  bool bad = false;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    chi[s] = row[(long long)s * M];
    bad |= !steer_finite(chi[s]);
  }
  if (P.done)
    for (int s = c; s < S; s += n) bad |= P.done[(long long)s * M + m] != 0;
  sFlag[c * E + e] = bad ? 1 : 0;

  // the mean and the deviations, in registers
  const T chi0 = chi[0];
  T acc = chi[1];
#pragma unroll
  for (int s = 2; s < S; ++s) acc = acc + chi[s];
  const T xbar = P.wm0 * chi0 + P.wi * acc;
#pragma unroll
  for (int s = 0; s < S; ++s) chi[s] = chi[s] - xbar;

  // the covariance: cov[i] = sum_{s >= 1} d_s[i] d_s[c], the chunks alternating between two buffers
  T cov[n];
  sD0[c * E + e] = chi[0];
#pragma unroll
  for (int k = 0; k < 2 * n / CH; ++k) {
    T* const buf = sDv + (k % 2) * CH * n * E;
#pragma unroll
    for (int h = 0; h < CH; ++h) buf[(h * n + c) * E + e] = chi[1 + k * CH + h];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < CH; ++h) {
      const T dc = chi[1 + k * CH + h];
#pragma unroll
      for (int i = 0; i < n; ++i) {
        const T prod = buf[(h * n + i) * E + e] * dc;
        if (k == 0 && h == 0) cov[i] = prod;
        else cov[i] = cov[i] + prod;
      }
      // The sums are pinned where they stand (an empty asm on each, and a boundary for the scheduler): left alone, instruction
      // selection moves all 2n n multiply-adds behind the last barrier and spills what the LDS loads brought until then
#pragma unroll
      for (int i = 0; i < n; ++i) asm volatile("" : "+v"(cov[i]));
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // (sFlag was published before the first of those barriers.)  p_in is read here, where the points' registers are free: still
  // before the first store of the workgroup
  T pc[n];
#pragma unroll
  for (int l = 0; l < n; ++l) pc[l] = l <= c ? P.p_in[(long long)(l * n + c) * M + m] : P.p_in[(long long)(c * n + l) * M + m];
  int lost = 0;
#pragma unroll
  for (int i = 0; i < n; ++i) lost |= sFlag[i * E + e];
  const bool is_lost = lost != 0;
#pragma unroll
  for (int i = 0; i < n; ++i) {
    const T pm = sQ[i * n + c] + (P.wc0 * (sD0[i * E + e] * chi[0]) + P.wi * cov[i]);
    pc[i] = is_lost ? pc[i] : pm;
  }
  T x = is_lost ? chi0 : xbar;
  __syncthreads();                  // nobody reads the chunks any more: the upper triangle of P- goes where they were
  // From here on pc[i], i <= c, is P[i][c], and LDS holds the upper triangle: thread c stores all of pc, so that no store sits
  // behind a mask of its own -- what it puts below the diagonal (pc[i], i > c, whatever that holds) is never read
  sX[c * E + e] = x;
#pragma unroll
  for (int i = 0; i < n; ++i) sP[(i * n + c) * E + e] = pc[i];
  __syncthreads();

  // the slots: the text of ekf_update_kernel's loop (os2r_ekf.hpp)
  T nis = T(0);
  int used = 0, refused = 0;
  for (int d = 0; d < D; ++d) {
    const int sc = ka->slot_col[d];                     // uniform over the grid
    T* const innov = P.innov ? P.innov + m * D + d : nullptr;
    if (sc < 0) {
      if (innov && c == 0 && valid) *innov = T(0);
      continue;
    }
    // the verdict of the robot, the same in each of its threads
    const T y = sY[d * E + e], r = sR[d];
    const T s = sP[(sc * n + sc) * E + e] + r;
    const T v = y - sX[sc * E + e];
    const T z = (v * v) / s;
    const bool look = sDrop[d] == 0 && steer_finite(y);
    const bool s_ok = ukf_positive(s), z_ok = steer_finite(z);
    const bool refuse = look && !(s_ok && z_ok);
    const bool gated = P.gate > T(0) && z > P.gate;
    const bool apply = look && s_ok && z_ok && !gated;
    const T pj = sP[((sc < c ? sc : c) * n + (sc < c ? c : sc)) * E + e];   // P[sc][c] = P[c][sc], from the upper triangle
    const T kc = pj / s;
    sK[c * E + e] = kc;
    __syncthreads();
    {
      const T xn = x + kc * v;
      x = apply ? xn : x;
      sX[c * E + e] = x;
#pragma unroll
      for (int i = 0; i < n; ++i) {
        const T pn = pc[i] - sK[i * E + e] * pj;
        pc[i] = apply ? pn : pc[i];
        sP[(i * n + c) * E + e] = pc[i];
      }
      const T zn = nis + z;
      nis = apply ? zn : nis;
      used |= apply ? 1 << d : 0;
      refused |= refuse ? 1 << d : 0;
      if (innov && c == 0 && valid) *innov = apply ? v : T(0);
    }
    __syncthreads();
  }

  // epilogue (behind a barrier in every case: the one before the slots, or the last slot's)
  if (valid) {
    P.x_out[(long long)c * M + m] = x;
#pragma unroll
    for (int i = 0; i < n; ++i) P.p_out[(long long)(i * n + c) * M + m] = sP[((i < c ? i : c) * n + (i < c ? c : i)) * E + e];
    if (c == 0) {
      if (P.nis) P.nis[m] = nis;
      if (P.used) P.used[m] = used;
      if (P.refused) P.refused[m] = refused;
      if (P.lost) P.lost[m] = lost;
    }
  }
  if (P.points) {                   // a kernel argument: every wave takes these barriers or none
    const T diag = sP[(c * n + c) * E + e];
    __syncthreads();                // nobody reads P in LDS any more: the factor goes where it was
    ukf_factor_points<T, n>(x, diag, pc, P.gamma, sM, sK, c, e, m, M, valid, P.points, P.failed);
  }
}

// the launches (os2r_ukf_inst.hip, once per dtype): 1 if there is no kernel for this nq
template <typename T>
int launch_ukf_points(int nq, const UkfPointsArgs<T>& args, hipStream_t stream);
template <typename T>
int launch_ukf_update(int nq, const UkfArgs<T>& args, hipStream_t stream);

}  // namespace os2r
