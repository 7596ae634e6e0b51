// os2r_ilqr.hpp — os2rc_ilqr_backward: the backward pass of iLQR for many trajectories in one launch (gfx950).
//
// The lane layout is that of os2r_lqr.hpp: one trajectory per n + 2 lanes, n = 2 nq, a workgroup is kLqrEnvs = 32 trajectories
// x (n + 2) columns, thread (column c, trajectory e) = c * 32 + e.  Lane c < n keeps column c of A_k in registers, lane n + b
// column b of B_k; P, A, B, G, K live in LDS as [.][.][e] (conflict-free: a half-wave reads 32 consecutive words).  The vector
// part rides on the same lanes: the value gradient p takes n * 32 words of LDS, column lane c forms Qx[c] from its own column
// and p, input lane b forms Qu[b] and publishes it.  Per knot:
//   top      the input lanes publish their column of B_k
//   barrier  (P', p' of the knot before and B_k are visible)
//   phase 1  every lane: pv = P v, g_r = sum_l B[l][r] pv[l] (G[r][c] for a column lane, column b of B^T P B for input lane b)
//            and gv = grad + sum_l v[l] p[l] (Qx[c] or Qu[b]); the column lanes publish their column of A_k.  The next knot's
//            column and gradient entry are requested before phase 1 and wait in registers.
//   barrier  (G, B^T P B, Qu and A_k are visible; nobody reads P or p any more)
//   phase 2a column lane j: S, T = S + mu, det, the verdict, K[.][j] and -- every column lane for itself, the two extra
//            divisions are cheaper than a barrier -- k; the knot's gains, feed-forward step, flag and dv go out
//   barrier  only when mu != 0 (P' needs the K of other columns) or the weight table is asked for (a kernel argument: every
//            wave takes it or none)
//   phase 2b column lane j: P'[i][j], i <= j, to both triangles, and p'[j]; meanwhile input lane b writes row b of the knot's
//            weight set for every step size
// No lane indexes a register array at run time, nothing goes to scratch (tests/test_ilqr_backward_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_control.h: the layout's dtype, no contraction, every sum of products
// ((x0 y0 + x1 y1) + x2 y2) + ... with the index ascending.  tests/test_gpu_ilqr_backward.py restates it in numpy, bit for bit.
//
// os2r_ilqr_mu.hpp (one mu per trajectory) and os2r_ilqr_box.hpp (that, with the box QP in phase 2a) hold copies of this text,
// against the rule of DESIGN.md section 4; the first says why.  Whoever changes one of the three texts changes the others.
#pragma once
#include "os2r_lqr.hpp"
#include "../../include/os2r_control.h"

namespace os2r {

template <typename T>
struct IlqrArgs {
  const T* __restrict__ a;         // [n][n][L], L = K * M, lane of (knot k, trajectory m) = k * M + m
  const T* __restrict__ b;         // [n][2][L]
  const T* __restrict__ lx;        // [n][L] or null (zeros)
  const T* __restrict__ lu;        // [2][L] or null (zeros)
  const T* pmat_final;             // [n][n][M] or null (Q); upper triangle read; pmat_out may alias it
  const T* pvec_final;             // [n][M] or null (zeros); pvec_out may alias it
  T* pmat_out;                     // [n][n][M] or null
  T* pvec_out;                     // [n][M] or null
  T* __restrict__ gain;            // [K][2][n][M] or null
  T* __restrict__ ff;              // [K][2][M] or null
  uint8_t* __restrict__ flag;      // [K][M] or null
  T* __restrict__ dv;              // [K][2][M] or null
  const T* __restrict__ actions;   // [L][2], with weights
  const T* __restrict__ obs;       // [L][D], with weights
  T* __restrict__ weights;         // [K][2][D+1][nalpha * M] or null
  long long M;
  int K, D, nalpha;
  int slot_col[OS2R_MAX_OBS];      // state column a raw observation slot shows, -1: the slot carries no gain
  T r00, r01, r11, mu;
  T alpha[OS2RC_MAX_ALPHAS];       // rounded to T by the host
  T q[kLqrMaxN * kLqrMaxN];        // [n][n] row-major, rounded to T by the host
};

template <typename T, int NQ>
__global__ __launch_bounds__(kLqrEnvs * (2 * NQ + 2)) void ilqr_backward_kernel(const IlqrArgs<T> P) {
#pragma clang fp contract(off)
  constexpr int n = 2 * NQ, E = kLqrEnvs;
  __shared__ T sP[n * n * E], sA[n * n * E], sB[n * 2 * E], sG[2 * (n + 2) * E], sK[2 * n * E], sQ[n * n];
  __shared__ T sp[n * E], sQu[2 * E], sKf[2 * E], sAl[OS2RC_MAX_ALPHAS];
  const int e = threadIdx.x % E, c = threadIdx.x / E;   // c is uniform over a half-wave, c < n over a wave (n is even)
  const bool col_lane = c < n;
  const long long M = P.M, m_raw = (long long)blockIdx.x * E + e;
  const bool valid = m_raw < M;
  const long long m = valid ? m_raw : M - 1;            // tail lanes shadow the last trajectory, their stores are masked
  const int K = P.K;
  const long long L = (long long)K * M;
  // the lane's column of [A | B]: element l at src[l * stride + k * M]; its entry of [lx | lu] at grad[k * M]
  const T* src = col_lane ? P.a + (long long)c * L + m : P.b + (long long)(c - n) * L + m;
  const long long stride = (col_lane ? n : 2) * L;
  const T* gbase = col_lane ? P.lx : P.lu;
  const T* grad = gbase ? gbase + (long long)(col_lane ? c : c - n) * L + m : nullptr;
  const bool reg = P.mu != T(0), third = reg || P.weights != nullptr;

  {  // Q and the step sizes for everybody (read with a lane index: from the argument segment as memory, not from a copy of the struct)
    const OS2R_CONST IlqrArgs<T>* ka = (const OS2R_CONST IlqrArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();
    if ((int)threadIdx.x < n * n) sQ[threadIdx.x] = ka->q[threadIdx.x];
    if ((int)threadIdx.x < OS2RC_MAX_ALPHAS) sAl[threadIdx.x] = ka->alpha[threadIdx.x];
  }
  __syncthreads();
  if (col_lane) {
#pragma unroll
    for (int i = 0; i < n; ++i)
      if (i <= c) {
        const T p = P.pmat_final ? P.pmat_final[(long long)(i * n + c) * M + m] : sQ[i * n + c];
        sP[(i * n + c) * E + e] = p;
        sP[(c * n + i) * E + e] = p;
      }
    sp[c * E + e] = P.pvec_final ? P.pvec_final[(long long)c * M + m] : T(0);
  }

  int k = K - 1;
  T v[n], vn[n];
#pragma unroll
  for (int l = 0; l < n; ++l) vn[l] = v[l] = src[l * stride + (long long)k * M];
  T gr = grad ? grad[(long long)k * M] : T(0), grn = gr;

  for (; k >= 0; --k) {
    if (!col_lane) {
#pragma unroll
      for (int l = 0; l < n; ++l) sB[(l * 2 + (c - n)) * E + e] = v[l];
    }
    __syncthreads();
    // the next knot's column and gradient entry, in flight during this knot
    if (k > 0) {
#pragma unroll
      for (int l = 0; l < n; ++l) vn[l] = src[l * stride + (long long)(k - 1) * M];
      if (grad) grn = grad[(long long)(k - 1) * M];
    }
    // phase 1
    T pv[n];
#pragma unroll
    for (int i = 0; i < n; ++i) {
      T acc = sP[(i * n + 0) * E + e] * v[0];
#pragma unroll
      for (int l = 1; l < n; ++l) acc = acc + sP[(i * n + l) * E + e] * v[l];
      pv[i] = acc;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      T acc = sB[(0 * 2 + r) * E + e] * pv[0];
#pragma unroll
      for (int l = 1; l < n; ++l) acc = acc + sB[(l * 2 + r) * E + e] * pv[l];
      sG[(r * (n + 2) + c) * E + e] = acc;
    }
    T gv;   // Qx[c] of a column lane, Qu[b] of an input lane
    {
      T acc = v[0] * sp[0 * E + e];
#pragma unroll
      for (int l = 1; l < n; ++l) acc = acc + v[l] * sp[l * E + e];
      gv = gr + acc;
    }
    if (col_lane) {
#pragma unroll
      for (int l = 0; l < n; ++l) sA[(l * n + c) * E + e] = v[l];
    } else {
      sQu[(c - n) * E + e] = gv;
    }
    __syncthreads();
    // phase 2a
    T k0 = T(0), k1 = T(0), f0 = T(0), f1 = T(0);
    if (col_lane) {
      const T s00 = P.r00 + sG[(0 * (n + 2) + n) * E + e];
      const T s01 = P.r01 + sG[(0 * (n + 2) + n + 1) * E + e];
      const T s11 = P.r11 + sG[(1 * (n + 2) + n + 1) * E + e];
      const T t00 = reg ? s00 + P.mu : s00, t11 = reg ? s11 + P.mu : s11;
      const T det = t00 * t11 - s01 * s01;
      const bool ok = lqr_finite(det) && t00 > T(0) && det > T(0);
      const T g0 = sG[(0 * (n + 2) + c) * E + e], g1 = sG[(1 * (n + 2) + c) * E + e];
      const T qu0 = sQu[0 * E + e], qu1 = sQu[1 * E + e];
      k0 = (t11 * g0 - s01 * g1) / det;
      k1 = (t00 * g1 - s01 * g0) / det;
      f0 = lqr_neg((t11 * qu0 - s01 * qu1) / det);
      f1 = lqr_neg((t00 * qu1 - s01 * qu0) / det);
      k0 = ok ? k0 : T(0);
      k1 = ok ? k1 : T(0);
      f0 = ok ? f0 : T(0);
      f1 = ok ? f1 : T(0);
      if (valid) {
        if (P.gain) {
          P.gain[(((long long)k * 2 + 0) * n + c) * M + m] = k0;
          P.gain[(((long long)k * 2 + 1) * n + c) * M + m] = k1;
        }
        if (c == 0) {
          if (P.flag) P.flag[(long long)k * M + m] = ok ? 0 : 1;
          if (P.ff) {
            P.ff[((long long)k * 2 + 0) * M + m] = f0;
            P.ff[((long long)k * 2 + 1) * M + m] = f1;
          }
        }
        if (c == 1 && P.dv) {
          P.dv[((long long)k * 2 + 0) * M + m] = f0 * qu0 + f1 * qu1;
          P.dv[((long long)k * 2 + 1) * M + m] = T(0.5) * (((s00 * f0) * f0 + (s11 * f1) * f1) + T(2) * ((s01 * f0) * f1));
        }
      }
      if (third) {
        sK[(0 * n + c) * E + e] = k0;
        sK[(1 * n + c) * E + e] = k1;
        if (c == 0) {
          sKf[0 * E + e] = f0;
          sKf[1 * E + e] = f1;
        }
      }
    }
    if (third) __syncthreads();
    // phase 2b
    if (col_lane) {
#pragma unroll
      for (int i = 0; i < n; ++i)
        if (i <= c) {
          T acc = sA[(0 * n + i) * E + e] * pv[0];
#pragma unroll
          for (int l = 1; l < n; ++l) acc = acc + sA[(l * n + i) * E + e] * pv[l];
          const T gk = sG[(0 * (n + 2) + i) * E + e] * k0 + sG[(1 * (n + 2) + i) * E + e] * k1;
          T p = (sQ[i * n + c] + acc) - gk;
          if (reg) p = p - P.mu * (sK[(0 * n + i) * E + e] * k0 + sK[(1 * n + i) * E + e] * k1);
          sP[(i * n + c) * E + e] = p;
          sP[(c * n + i) * E + e] = p;
        }
      T pj = gv + (sG[(0 * (n + 2) + c) * E + e] * f0 + sG[(1 * (n + 2) + c) * E + e] * f1);
      if (reg) pj = pj + P.mu * (k0 * f0 + k1 * f1);
      sp[c * E + e] = pj;
    } else if (P.weights) {
      // row j = c - n of the knot's set: a = (a0 + alpha k) - K (x - x_k) on the raw observation slots, one lane per step size
      const int j = c - n, D = P.D, nalpha = P.nalpha;
      const long long lane = (long long)k * M + m, NM = (long long)nalpha * M;
      T* w = P.weights + (((long long)k * 2 + j) * (D + 1)) * NM + m;
      T acc = T(0);
      bool first = true;
#pragma unroll
      for (int d = 0; d < OS2R_MAX_OBS; ++d)
        if (d < D) {
          const int sc = P.slot_col[d];
          T wd = T(0);
          if (sc >= 0) {
            wd = lqr_neg(sK[(j * n + sc) * E + e]);
            const T t = wd * P.obs[lane * D + d];
            acc = first ? t : acc + t;
            first = false;
          }
          if (valid)
            for (int i = 0; i < nalpha; ++i) w[(long long)d * NM + (long long)i * M] = wd;
        }
      T a0 = P.actions[2 * lane + j];
      a0 = a0 < T(-1) ? T(-1) : (a0 > T(1) ? T(1) : a0);
      const T fj = sKf[j * E + e];
      if (valid)
        for (int i = 0; i < nalpha; ++i) w[(long long)D * NM + (long long)i * M] = (a0 + sAl[i] * fj) - acc;
    }
#pragma unroll
    for (int l = 0; l < n; ++l) v[l] = vn[l];
    gr = grn;
  }

  if (P.pmat_out || P.pvec_out) {
    __syncthreads();
    if (col_lane && valid) {
      if (P.pmat_out) {
#pragma unroll
        for (int i = 0; i < n; ++i) P.pmat_out[(long long)(i * n + c) * M + m] = sP[(i * n + c) * E + e];
      }
      if (P.pvec_out) P.pvec_out[(long long)c * M + m] = sp[c * E + e];
    }
  }
}

// the launch (os2r_ilqr_inst.hip, once per dtype): 1 if there is no kernel for this nq
template <typename T>
int launch_ilqr_backward(int nq, const IlqrArgs<T>& args, hipStream_t stream);

}  // namespace os2r
