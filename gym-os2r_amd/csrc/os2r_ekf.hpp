// os2r_ekf.hpp — os2re_ekf_update: the Kalman filter update of many robots in one launch (gfx950).
//
// One robot per n lanes, n = 2 nq, in the shape of lqr_gains_kernel (os2r_lqr.hpp).  The grid is ceil(M / 32) workgroups; a
// workgroup is kEkfRobots = 32 robots x n columns, thread (column c, robot e) = c * 32 + e: the 32 lanes of one column read and
// write 32 consecutive elements of the robot-fastest arrays (256 B in fp64), and a wave holds two whole columns.  Lane c owns
// column c of P and x_c.  P, x and what the lanes hand each other are in LDS as [.][.][e] (conflict-free: a half-wave reads 32
// consecutive words, both half-waves of a b64 read are served apart).
//   prologue   lane c reads x_c, column c of the symmetric P (the upper triangle of p_in: row c right of the diagonal), row c of
//              A, the measurements of its share of the slots; the first D threads form r_d = 1 / prec_d.  Every global input
//              of the workgroup is read here, before its first store: that is what lets x_out be x_pred and p_out be p_in
//   with a_dev (a kernel argument: every wave takes these barriers or none)
//     barrier  A is in LDS
//     phase 1  lane c: column c of AP, from A in LDS and its column of P in registers, kept in registers
//     barrier  nobody reads A in LDS any more: AP goes where it was
//     barrier  AP is in LDS
//     phase 2  lane c: P-[i][c], i <= c, from AP in LDS, its row of A in registers and Q, kept in registers
//     barrier  nobody reads AP in LDS any more: the upper triangle of P- goes where it was
//   barrier    P-, x, the measurements and r_d are in LDS
//   per slot d with c = slot_col[d] >= 0 (a kernel argument, read from the argument segment: no lane indexes a register array
//   with it), two barriers:
//     gain     every lane of a robot forms the same s, v, z and the same verdict from LDS -- P[c][c], x_c, y_d, r_d -- and lane
//              i publishes k_i = P[c][i] / s (row c: by the bitwise symmetry of P the same bits as P[i][c])
//     barrier  k is in LDS
//     update   lane j: x_j += k_j v and P[i][j] -= k_i P[c][j] for i <= j, the upper triangle, where the robot's verdict is
//              "applied"; a robot that skips or refuses the slot writes back what it read: the verdicts of a workgroup's robots
//              differ, they mask the work and never branch round a barrier
//     barrier  P and x of the next slot are in LDS
//   epilogue   lane c stores x_c and column c of P, its lower part from row c of the upper triangle in LDS; lane 0 of a robot nis, used and refused.  innov is stored slot by slot by
//              lane 0 (it may overlap no input)
// Publishing k_i costs the second barrier of a slot; the other form, every lane dividing for the k_i, i <= j, it needs, costs
// up to n divisions per lane and slot where this one costs one.  In the built code object an IEEE division is 11 or 12
// instructions in either dtype, and the published form pays a store, a barrier and n loads of k with their waits, n + 4: the
// wave that holds the last column saves about 90 instructions per slot with n = 10 and about 25 with n = 4.  The slot loop is 274
// instructions in fp64 with n = 10 (197 with n = 4); with a mask `i <= c` on the update and stores to both triangles it was 344,
// 30 of them `s_and_saveexec` with their branches and restores.  The bits are the same either way.
// LDS of a workgroup: one n x n matrix (A, then AP, then P: each goes through registers into the place of the one before it,
// which costs two barriers per launch and halves the LDS), x, k, the measurements, r and Q:
// ((n n + 2 n + 12) 32 + n n + 12) sizeof(T) + 12 * 4 bytes -- 34736 for double and nq = 5: four workgroups fit the
// 160 KiB of a CU; its 113 registers allow four waves on a SIMD (kEkfWavesPerSimd: five made it spill), sixteen on a CU, three
// workgroups of five; no dynamic LDS.  Tail lanes shadow the last robot and their stores are masked.  No lane indexes a
// register array at run time, nothing goes to scratch (tests/test_ekf_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_ekf.h: the layout's dtype, no contraction, every sum of products
// ((x0 y0 + x1 y1) + x2 y2) + ... with the index ascending.  tests/test_ekf_host.py restates it in numpy; tests/test_gpu_ekf.py
// compares bit for bit.
#pragma once
#include "os2r_lqr.hpp"   // by_chain_length, OS2R_CONST
#include "os2r_bits.hpp"
#include "../../include/os2r_ekf.h"

namespace os2r {

constexpr int kEkfRobots = 32;                 // robots of one workgroup
constexpr int kEkfMaxN = 2 * OS2R_MAX_DOF;
constexpr int kEkfObs = OS2R_MAX_OBS;
constexpr int kEkfWavesPerSimd = 4;            // three workgroups of five waves on the four SIMDs of a CU: at most 128 registers

template <typename T>
struct EkfArgs {
  const T* x_pred;                 // [n][M]; x_out may be this very pointer
  const T* p_in;                   // [n][n][M], upper triangle read; p_out may be this very pointer
  const T* __restrict__ a;         // [n][n][M] or null
  const T* __restrict__ meas;      // [M][D]
  const T* __restrict__ prec;      // [D]
  T* x_out;                        // [n][M]
  T* p_out;                        // [n][n][M]
  T* __restrict__ nis;             // [M] or null
  int* __restrict__ used;          // [M] or null
  int* __restrict__ refused;       // [M] or null
  T* __restrict__ innov;           // [M][D] or null
  long long M;
  int D;
  int slot_col[kEkfObs];           // state column a raw observation slot shows, -1: none
  T gate;                          // rounded to T by the host; 0: no gate
  T q[kEkfMaxN * kEkfMaxN];        // [n][n] row-major, rounded to T by the host; not read without a
};

// finite and > 0, on the bits (os2r_bits.hpp says why): neither negative nor not finite, and no zero
__device__ __forceinline__ bool ekf_positive(float x) { return !steer_invalid(x) && (steer_bits(x) & 0x7fffffffu) != 0u; }
__device__ __forceinline__ bool ekf_positive(double x) { return !steer_invalid(x) && (steer_bits(x) & 0x7fffffffffffffffull) != 0ull; }

template <typename T, int NQ>
__global__ __launch_bounds__(kEkfRobots * 2 * NQ, kEkfWavesPerSimd) void ekf_update_kernel(const EkfArgs<T> P) {
#pragma clang fp contract(off)
  constexpr int n = 2 * NQ, E = kEkfRobots;
  __shared__ T sM[n * n * E], sX[n * E], sK[n * E], sY[kEkfObs * E], sR[kEkfObs], sQ[n * n];
  __shared__ int sDrop[kEkfObs];
  T* const sA = sM;                 // [n][n][e], until phase 1 is over
  T* const sAP = sM;                // [n][n][e], during phase 2
  T* const sP = sM;                 // [n][n][e], from then on
  const int e = threadIdx.x % E, c = threadIdx.x / E;   // c is uniform over a half-wave
  const long long M = P.M, m_raw = (long long)blockIdx.x * E + e;
  const bool valid = m_raw < M;
  const long long m = valid ? m_raw : M - 1;            // tail lanes shadow the last robot, their stores are masked
  const int D = P.D;
  const bool predict = P.a != nullptr;                  // uniform over the grid
  // (what is read with a run-time index comes from the argument segment as memory, not from a copy of the struct)
  const OS2R_CONST EkfArgs<T>* ka = (const OS2R_CONST EkfArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();

  // prologue: every global input of this workgroup
  if (predict && (int)threadIdx.x < n * n) sQ[threadIdx.x] = ka->q[threadIdx.x];
  if ((int)threadIdx.x < kEkfObs) {
    const T pr = P.prec[(int)threadIdx.x < D ? (int)threadIdx.x : D - 1];
    sDrop[threadIdx.x] = ekf_positive(pr) ? 0 : 1;
    sR[threadIdx.x] = T(1) / pr;
  }
  for (int d = c; d < D; d += n) sY[d * E + e] = P.meas[m * D + d];
  T x = P.x_pred[(long long)c * M + m];
  sX[c * E + e] = x;
  T pc[n], ar[n];
#pragma unroll
  for (int l = 0; l < n; ++l) {
    pc[l] = l <= c ? P.p_in[(long long)(l * n + c) * M + m] : P.p_in[(long long)(c * n + l) * M + m];
    ar[l] = predict ? P.a[(long long)(c * n + l) * M + m] : T(0);
  }

  if (predict) {
#pragma unroll
    for (int l = 0; l < n; ++l) sA[(c * n + l) * E + e] = ar[l];
    __syncthreads();
    // phase 1: column c of AP
    T ap[n];
#pragma unroll
    for (int i = 0; i < n; ++i) {
      T acc = sA[(i * n + 0) * E + e] * pc[0];
#pragma unroll
      for (int l = 1; l < n; ++l) acc = acc + sA[(i * n + l) * E + e] * pc[l];
      ap[i] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < n; ++i) sAP[(i * n + c) * E + e] = ap[i];
    __syncthreads();
    // phase 2: P-[i][c], i <= c
#pragma unroll
    for (int i = 0; i < n; ++i)
      if (i <= c) {
        T acc = sAP[(i * n + 0) * E + e] * ar[0];
#pragma unroll
        for (int l = 1; l < n; ++l) acc = acc + sAP[(i * n + l) * E + e] * ar[l];
        pc[i] = sQ[i * n + c] + acc;
      }
    __syncthreads();
  }
  // From here on pc[i], i <= c, is P[i][c], and LDS holds the upper triangle: lane c stores all of pc, so that no store sits
  // behind a mask of its own -- what it puts below the diagonal (pc[i], i > c, whatever that holds) is never read
#pragma unroll
  for (int i = 0; i < n; ++i) sP[(i * n + c) * E + e] = pc[i];
  __syncthreads();

  // the slots
  T nis = T(0);
  int used = 0, refused = 0;
  for (int d = 0; d < D; ++d) {
    const int sc = ka->slot_col[d];                     // uniform over the grid
    T* const innov = P.innov ? P.innov + m * D + d : nullptr;
    if (sc < 0) {
      if (innov && c == 0 && valid) *innov = T(0);
      continue;
    }
    // the verdict of the robot, the same in each of its lanes
    const T y = sY[d * E + e], r = sR[d];
    const T s = sP[(sc * n + sc) * E + e] + r;
    const T v = y - sX[sc * E + e];
    const T z = (v * v) / s;
    const bool look = sDrop[d] == 0 && steer_finite(y);
    const bool s_ok = ekf_positive(s), z_ok = steer_finite(z);
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
      for (int i = 0; i < n; ++i) {                     // (every i: see above; the wave of the last column does them all anyway)
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
    }
  }
}

// the launch (os2r_ekf_inst.hip, once per dtype): 1 if there is no kernel for this nq
template <typename T>
int launch_ekf_update(int nq, const EkfArgs<T>& args, hipStream_t stream);

}  // namespace os2r
