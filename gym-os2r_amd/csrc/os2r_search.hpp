// os2r_search.hpp — os2rs_ilqr_line_search: the forward-pass evaluation of iLQR for many trajectories in one launch (gfx950).
//
// A workgroup is kSearchTraj = 64 trajectories x nalpha candidates: wave i holds candidate i, its lane t trajectory
// blockIdx.x * 64 + t, so thread (candidate i, trajectory t) = i * 64 + t and what differs between candidates is wave-uniform.
//   phase 1  every lane runs the K knots of its candidate lane j = i M + m and the end in order and accumulates J (steps 1-6
//            of include/os2r_search.h); the done flags are OR-ed along the way.  Of a row of D observation slots only the
//            slots that show a state column are read (col_slot, the inverse of slot_col, comes from the host); a row is
//            contiguous, so the lines its lanes touch are reused from the cache across the column loop.  The next knot's
//            values are requested before the current knot's sums, wait in registers, and nothing of them is used before
//            the knot ends.  Q and Qf stay where the launch put them, in the kernel-argument segment, and are read by scalar
//            loads: the first build staged them in LDS as os2r_ilqr.hpp does, and a lone wave waited for each of its
//            n * n broadcast reads per knot (profiles/ilqr_line_search_rate.txt has both builds' times).
//   barrier  J and the verdicts are in LDS as [nalpha][64]
//   phase 2  every lane finds the choice of its trajectory (the same scan in every wave); the nalpha waves then share the K
//            knots plus the end of the write-back, wave w taking items w, w + nalpha, ...: a lane whose trajectory accepted a
//            candidate reads that candidate's row again, forms gx, gu (gf at the end) by the code of phase 1 -- the same
//            operations in the same order, so the same bits -- and writes the nominal; wave 0 writes choice and cost.
// Tail lanes shadow the last trajectory, their stores are masked.  No lane indexes a register array at run time, nothing goes
// to scratch (tests/test_ilqr_line_search_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_search.h: the layout's dtype, no contraction, every sum of products
// ((x0 y0 + x1 y1) + x2 y2) + ... with the index ascending.  tests/test_gpu_ilqr_line_search.py restates it in numpy, bit for bit.
#pragma once
#include "os2r_lqr.hpp"
#include "../../include/os2r_search.h"

namespace os2r {

constexpr int kSearchTraj = 64;   // trajectories of one workgroup: one wave per candidate

template <typename T>
struct SearchArgs {
  const T* __restrict__ knot_obs;      // [K][N][D], N = nalpha * M, candidate lane j = i * M + m
  const T* __restrict__ end_obs;       // [N][D]
  const T* __restrict__ act;           // [K][N][2]
  const uint8_t* __restrict__ done;    // [K][N] or null
  const T* __restrict__ target;        // [M][D]
  T* cost;                             // [M]: read (unless accept_always), written where a candidate was accepted
  T* __restrict__ act_nom;             // [K][M][2] or null
  T* __restrict__ obs_nom;             // [K][M][D] or null
  T* __restrict__ end_nom;             // [M][D] or null
  T* __restrict__ lx;                  // [n][L] or null, L = K * M
  T* __restrict__ lu;                  // [2][L] or null
  T* __restrict__ pvec_final;          // [n][M] or null
  int* __restrict__ choice;            // [M]
  int* __restrict__ index;             // [L] or null
  T* __restrict__ cand_cost;           // [nalpha][M] or null
  long long M;
  int K, D, nalpha, accept_always;
  int col_slot[kLqrMaxN];              // the lowest raw observation slot that shows state column c, -1: none
  T r00, r01, r11;
  T q[kLqrMaxN * kLqrMaxN];            // [n][n] row-major, rounded to T by the host
  T qf[kLqrMaxN * kLqrMaxN];           // the terminal Hessian (q again where the caller gave none)
};

// the values of a row of observations at the slots that show the state columns; where none does, slot 0 is read and search_quad
// drops the value: n loads behind each other, no branch between them
template <typename T, int n>
__device__ __forceinline__ void search_row(const T* row, const int (&cs)[kLqrMaxN], T (&raw)[n]) {
#pragma unroll
  for (int c = 0; c < n; ++c) raw[c] = row[cs[c] < 0 ? 0 : cs[c]];
}

// steps 2 and 3 (or 6, with Qf): e = raw - tg on the shown columns, g = Q e, -> 0.5 e'g.  Q is read where the launch put it, in
// the kernel-argument segment, by scalar loads (the address is wave-uniform): its entries reach the multiplications as scalar
// operands and take no vector register.  The pointer passes through an empty asm so that the compiler knows nothing about it:
// left alone, it hoists the n * n loads out of the knot loop and spills what it hoisted.
template <typename T, int n>
__device__ __forceinline__ T search_quad(const OS2R_CONST T* q, const int (&cs)[kLqrMaxN], const T (&raw)[n], const T (&tg)[n], T (&g)[n]) {
#pragma clang fp contract(off)
  asm volatile("" : "+s"(q));
  T e[n];
#pragma unroll
  for (int c = 0; c < n; ++c) e[c] = cs[c] >= 0 ? raw[c] - tg[c] : T(0);
  T s = T(0);
#pragma unroll
  for (int r = 0; r < n; ++r) {
    T acc = q[r * n + 0] * e[0];
#pragma unroll
    for (int c = 1; c < n; ++c) acc = acc + q[r * n + c] * e[c];
    g[r] = acc;
    const T t = e[r] * acc;
    s = r == 0 ? t : s + t;
  }
  return T(0.5) * s;
}

template <typename T>
__device__ __forceinline__ T search_clamp(T a) { return a < T(-1) ? T(-1) : (a > T(1) ? T(1) : a); }

// step 4 on clamped actions: gu = R a, -> 0.5 a'gu
template <typename T>
__device__ __forceinline__ T search_act(T r00, T r01, T r11, T a0, T a1, T& gu0, T& gu1) {
#pragma clang fp contract(off)
  gu0 = r00 * a0 + r01 * a1;
  gu1 = r01 * a0 + r11 * a1;
  return T(0.5) * (a0 * gu0 + a1 * gu1);
}

template <typename T, int NQ>
__global__ __launch_bounds__(kSearchTraj * OS2RC_MAX_ALPHAS) void ilqr_line_search_kernel(const SearchArgs<T> P) {
#pragma clang fp contract(off)
  constexpr int n = 2 * NQ, E = kSearchTraj;
  __shared__ T sJ[OS2RC_MAX_ALPHAS * E];
  __shared__ int sOk[OS2RC_MAX_ALPHAS * E];
  const int t = threadIdx.x % E, w = threadIdx.x / E;   // w, the candidate, is uniform over a wave
  const long long M = P.M, m_raw = (long long)blockIdx.x * E + t;
  const bool valid = m_raw < M;
  const long long m = valid ? m_raw : M - 1;            // tail lanes shadow the last trajectory, their stores are masked
  const int K = P.K, D = P.D, nalpha = P.nalpha;
  const long long N = (long long)nalpha * M, L = (long long)K * M;
  const long long j = (long long)w * M + m;

  const OS2R_CONST SearchArgs<T>* ka = (const OS2R_CONST SearchArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();
  const OS2R_CONST T* q = ka->q;
  const OS2R_CONST T* qf = ka->qf;
  T tg[n];
  search_row<T, n>(P.target + m * D, P.col_slot, tg);

  // phase 1: the cost of candidate lane j
  T J = T(0);
  {
    T raw[n], rawn[n], g[n];
    search_row<T, n>(P.knot_obs + j * D, P.col_slot, raw);
    T a0 = P.act[2 * j], a1 = P.act[2 * j + 1], a0n = a0, a1n = a1;
    unsigned dn = 0u, dk = P.done ? P.done[j] : 0u, dkn = 0u;
    for (int k = 0; k < K; ++k) {
      // the next knot's values (behind the last knot: the end's), in flight during this knot
      if (k + 1 < K) {
        const long long jn = (long long)(k + 1) * N + j;
        search_row<T, n>(P.knot_obs + jn * D, P.col_slot, rawn);
        a0n = P.act[2 * jn];
        a1n = P.act[2 * jn + 1];
        if (P.done) dkn = P.done[jn];
      } else {
        search_row<T, n>(P.end_obs + j * D, P.col_slot, rawn);
      }
      const T sx = search_quad<T, n>(q, P.col_slot, raw, tg, g);
      T gu0, gu1;
      const T su = search_act<T>(P.r00, P.r01, P.r11, search_clamp(a0), search_clamp(a1), gu0, gu1);
      J = (J + sx) + su;
      dn |= dk;
      dk = dkn;
#pragma unroll
      for (int c = 0; c < n; ++c) raw[c] = rawn[c];
      a0 = a0n;
      a1 = a1n;
    }
    J = J + search_quad<T, n>(qf, P.col_slot, raw, tg, g);
    bool ok = lqr_finite(J) && dn == 0u;
    if (!P.accept_always) ok = ok && J < P.cost[m];
    sJ[w * E + t] = J;
    sOk[w * E + t] = ok ? 1 : 0;
    if (valid && P.cand_cost) P.cand_cost[j] = J;
  }
  __syncthreads();

  // phase 2: the choice of the lane's trajectory (step 7), the same in every wave
  int best = -1;
  T bestJ = T(0);
  for (int i = 0; i < nalpha; ++i) {
    const T Ji = sJ[i * E + t];
    const bool take = sOk[i * E + t] != 0 && (best < 0 || Ji < bestJ);
    best = take ? i : best;
    bestJ = take ? Ji : bestJ;
  }
  if (w == 0 && valid) {
    P.choice[m] = best;
    if (best >= 0) P.cost[m] = bestJ;
  }
  const bool knot_out = P.act_nom || P.obs_nom || P.lx || P.lu || P.index;
  const bool end_out = P.end_nom || P.pvec_final;
  const long long jb = (long long)best * M + m;         // the accepted candidate lane (meaningless where best < 0)
  for (int k = w; k <= K; k += nalpha) {
    if (k < K) {
      if (!knot_out) continue;
      const long long lane = (long long)k * M + m, src = (long long)k * N + jb;
      if (valid && P.index) P.index[lane] = best >= 0 ? (int)src : -1;
      if (!valid || best < 0) continue;
      const T* row = P.knot_obs + src * D;
      if (P.obs_nom) {
#pragma unroll
        for (int d = 0; d < OS2R_MAX_OBS; ++d)
          if (d < D) P.obs_nom[lane * D + d] = row[d];
      }
      if (P.act_nom || P.lu) {
        const T a0 = search_clamp(P.act[2 * src]), a1 = search_clamp(P.act[2 * src + 1]);
        T gu0, gu1;
        (void)search_act<T>(P.r00, P.r01, P.r11, a0, a1, gu0, gu1);
        if (P.act_nom) {
          P.act_nom[2 * lane] = a0;
          P.act_nom[2 * lane + 1] = a1;
        }
        if (P.lu) {
          P.lu[lane] = gu0;
          P.lu[L + lane] = gu1;
        }
      }
      if (P.lx) {
        T raw[n], g[n];
        search_row<T, n>(row, P.col_slot, raw);
        (void)search_quad<T, n>(q, P.col_slot, raw, tg, g);
#pragma unroll
        for (int r = 0; r < n; ++r) P.lx[(long long)r * L + lane] = g[r];
      }
    } else {
      if (!end_out || !valid || best < 0) continue;
      const T* row = P.end_obs + jb * D;
      if (P.end_nom) {
#pragma unroll
        for (int d = 0; d < OS2R_MAX_OBS; ++d)
          if (d < D) P.end_nom[m * D + d] = row[d];
      }
      if (P.pvec_final) {
        T raw[n], g[n];
        search_row<T, n>(row, P.col_slot, raw);
        (void)search_quad<T, n>(qf, P.col_slot, raw, tg, g);
#pragma unroll
        for (int r = 0; r < n; ++r) P.pvec_final[(long long)r * M + m] = g[r];
      }
    }
  }
}

// the launch (os2r_search_inst.hip, once per dtype): 1 if there is no kernel for this nq
template <typename T>
int launch_ilqr_line_search(int nq, const SearchArgs<T>& args, hipStream_t stream);

}  // namespace os2r
