// os2r_ilqr_box.hpp — os2rb_ilqr_backward_box: the backward pass of iLQR whose feed-forward step stays inside a box around the
// nominal action, one regularisation mu per trajectory or one for all (gfx950).
//
// The kernel is ilqr_backward_mu_kernel of os2r_ilqr_mu.hpp -- the same lane layout (32 trajectories x (n + 2) columns, P, A, B,
// G, K in LDS), the same prefetch, the same phases and barriers, the same operations in the same order -- with these differences:
//   mu       from the array, or, where that is null, the argument of os2rc_ilqr_backward: a uniform choice made once
//   actions  a column lane reads the two nominal actions of its trajectory's knot, prefetched with the next column
//   phase 2a after K and k of the interior, as there, every column lane solves the box QP of include/os2r_box.h (B1-B4) for
//            itself, as it forms k for itself: four edge candidates by selects, never by a branch that diverges (neighbouring
//            trajectories differ in their active set).  A wave none of whose trajectories leaves the box skips the candidates:
//            that branch is uniform, and what it skips is only ever selected by a lane that left the box.  Lane c == 0 writes
//            the clamp byte next to the flag.
// No lane indexes a register array at run time, nothing goes to scratch (tests/test_ilqr_box_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_box.h.  Every class test of a value (finite, NaN) is made on its bits
// (os2r_bits.hpp): the library is built without NaN and infinity semantics.
//
// This is the third text of the backward pass, next to os2r_ilqr.hpp and os2r_ilqr_mu.hpp, against the rule of DESIGN.md
// section 4.  Whoever changes one of the three texts changes the others.
#pragma once
#include "os2r_ilqr.hpp"
#include "os2r_bits.hpp"   // steer_invalid, steer_finite, steer_nan
#include "../../include/os2r_box.h"

namespace os2r {

template <typename T>
struct IlqrBoxArgs {
  IlqrArgs<T> base;                // as os2rc_ilqr_backward fills it; base.actions is always set; base.mu is read where mu is null
  const T* __restrict__ mu;        // [M] or null
  uint8_t* __restrict__ clamp;     // [K][M] or null
  T lo[2], hi[2];                  // rounded to T by the host; -inf / +inf: no bound
};

template <typename T, int NQ>
__global__ __launch_bounds__(kLqrEnvs * (2 * NQ + 2)) void ilqr_backward_box_kernel(const IlqrBoxArgs<T> PM) {
#pragma clang fp contract(off)
  constexpr int n = 2 * NQ, E = kLqrEnvs;
  const IlqrArgs<T>& P = PM.base;
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
  // the trajectory's mu, once: negative or not finite runs as 0 with every knot refused (the host has checked the scalar)
  const T mu_in = PM.mu ? PM.mu[m] : P.mu;
  const bool mu_bad = PM.mu != nullptr && steer_invalid(mu_in);
  const T mu = mu_bad ? T(0) : mu_in;
  const bool reg = mu != T(0);
  // the box: which of its four sides there are
  const T lo0 = PM.lo[0], lo1 = PM.lo[1], hi0 = PM.hi[0], hi1 = PM.hi[1];
  const bool has_lo0 = steer_finite(lo0), has_lo1 = steer_finite(lo1), has_hi0 = steer_finite(hi0), has_hi1 = steer_finite(hi1);

  {  // Q and the step sizes for everybody (read with a lane index: from the argument segment as memory, not from a copy of the struct)
    const OS2R_CONST IlqrBoxArgs<T>* ka = (const OS2R_CONST IlqrBoxArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();
    if ((int)threadIdx.x < n * n) sQ[threadIdx.x] = ka->base.q[threadIdx.x];
    if ((int)threadIdx.x < OS2RC_MAX_ALPHAS) sAl[threadIdx.x] = ka->base.alpha[threadIdx.x];
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
  // the knot's nominal actions, for the column lanes
  T na0 = T(0), na1 = T(0);
  if (col_lane) {
    na0 = P.actions[2 * ((long long)k * M + m) + 0];
    na1 = P.actions[2 * ((long long)k * M + m) + 1];
  }
  T nn0 = na0, nn1 = na1;

  for (; k >= 0; --k) {
    if (!col_lane) {
#pragma unroll
      for (int l = 0; l < n; ++l) sB[(l * 2 + (c - n)) * E + e] = v[l];
    }
    __syncthreads();
    // the next knot's column, gradient entry and nominal actions, in flight during this knot
    if (k > 0) {
#pragma unroll
      for (int l = 0; l < n; ++l) vn[l] = src[l * stride + (long long)(k - 1) * M];
      if (grad) grn = grad[(long long)(k - 1) * M];
      if (col_lane) {
        nn0 = P.actions[2 * ((long long)(k - 1) * M + m) + 0];
        nn1 = P.actions[2 * ((long long)(k - 1) * M + m) + 1];
      }
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
      const T t00 = reg ? s00 + mu : s00, t11 = reg ? s11 + mu : s11;
      const T det = t00 * t11 - s01 * s01;
      const bool ok = lqr_finite(det) && t00 > T(0) && det > T(0) && !mu_bad;
      const T g0 = sG[(0 * (n + 2) + c) * E + e], g1 = sG[(1 * (n + 2) + c) * E + e];
      const T qu0 = sQu[0 * E + e], qu1 = sQu[1 * E + e];
      k0 = (t11 * g0 - s01 * g1) / det;
      k1 = (t00 * g1 - s01 * g0) / det;
      f0 = lqr_neg((t11 * qu0 - s01 * qu1) / det);
      f1 = lqr_neg((t00 * qu1 - s01 * qu0) / det);
      // B1: the box around the clamped nominal
      const T a00 = na0 < T(-1) ? T(-1) : (na0 > T(1) ? T(1) : na0);
      const T a01 = na1 < T(-1) ? T(-1) : (na1 > T(1) ? T(1) : na1);
      const T dlo0 = lo0 - a00, dhi0 = hi0 - a00, dlo1 = lo1 - a01, dhi1 = hi1 - a01;
      // B2
      const bool inside = !steer_nan(f0) && !steer_nan(f1) && dlo0 <= f0 && f0 <= dhi0 && dlo1 <= f1 && f1 <= dhi1;
      bool have = false;
      unsigned cl = 0u;
      // B3, B4: skipped where no trajectory of the wave leaves the box (a uniform branch)
      if (__builtin_amdgcn_ballot_w64(ok && !inside) != 0ull) {
        T best = T(0), w0 = T(0), w1 = T(0), wk0 = T(0), wk1 = T(0);
        // the free row of K, should the other component be the clamped one
        const T row0 = g0 / t00, row1 = g1 / t11;
        // one candidate: component cc at b, the other at the clipped minimum along the edge
        auto edge = [&](const bool there, const int cc, const bool upper, const T b) {
          const T qj = cc == 0 ? qu1 : qu0, tjj = cc == 0 ? t11 : t00;
          const T dloj = cc == 0 ? dlo1 : dlo0, dhij = cc == 0 ? dhi1 : dhi0;
          const T raw = lqr_neg((qj + s01 * b) / tjj);
          const bool below = raw < dloj, above = raw > dhij, pinned = below || above;
          T u = below ? dloj : raw;
          u = above ? dhij : u;
          const T c0 = cc == 0 ? b : u, c1 = cc == 0 ? u : b;
          const T val = T(0.5) * (((t00 * c0) * c0 + (t11 * c1) * c1) + T(2) * ((s01 * c0) * c1)) + (qu0 * c0 + qu1 * c1);
          const bool alive = there && !steer_nan(raw) && steer_finite(val);
          const bool take = alive && (!have || val < best);
          const unsigned byte = (1u << cc) | (pinned ? 1u << (1 - cc) : 0u) | (upper ? 4u << cc : 0u) | (above ? 4u << (1 - cc) : 0u);
          const T free_row = pinned ? T(0) : (cc == 0 ? row1 : row0);
          best = take ? val : best;
          w0 = take ? c0 : w0;
          w1 = take ? c1 : w1;
          wk0 = take ? (cc == 0 ? T(0) : free_row) : wk0;
          wk1 = take ? (cc == 0 ? free_row : T(0)) : wk1;
          cl = take ? byte : cl;
          have = have || take;
        };
        edge(has_lo0, 0, false, dlo0);
        edge(has_hi0, 0, true, dhi0);
        edge(has_lo1, 1, false, dlo1);
        edge(has_hi1, 1, true, dhi1);
        k0 = inside ? k0 : wk0;
        k1 = inside ? k1 : wk1;
        f0 = inside ? f0 : w0;
        f1 = inside ? f1 : w1;
      }
      const bool solved = ok && (inside || have);
      cl = (ok && !inside && have) ? cl : 0u;
      k0 = solved ? k0 : T(0);
      k1 = solved ? k1 : T(0);
      f0 = solved ? f0 : T(0);
      f1 = solved ? f1 : T(0);
      if (valid) {
        if (P.gain) {
          P.gain[(((long long)k * 2 + 0) * n + c) * M + m] = k0;
          P.gain[(((long long)k * 2 + 1) * n + c) * M + m] = k1;
        }
        if (c == 0) {
          if (P.flag) P.flag[(long long)k * M + m] = solved ? 0 : 1;
          if (PM.clamp) PM.clamp[(long long)k * M + m] = (uint8_t)cl;
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
      sK[(0 * n + c) * E + e] = k0;
      sK[(1 * n + c) * E + e] = k1;
      if (c == 0) {
        sKf[0 * E + e] = f0;
        sKf[1 * E + e] = f1;
      }
    }
    __syncthreads();   // always: P' of a regularised trajectory needs the K of other columns, and its neighbour may be one
    // phase 2b
    if (col_lane) {
#pragma unroll
      for (int i = 0; i < n; ++i)
        if (i <= c) {
          T acc = sA[(0 * n + i) * E + e] * pv[0];
#pragma unroll
          for (int l = 1; l < n; ++l) acc = acc + sA[(l * n + i) * E + e] * pv[l];
          const T gk = sG[(0 * (n + 2) + i) * E + e] * k0 + sG[(1 * (n + 2) + i) * E + e] * k1;
          const T p0 = (sQ[i * n + c] + acc) - gk;
          const T p1 = p0 - mu * (sK[(0 * n + i) * E + e] * k0 + sK[(1 * n + i) * E + e] * k1);
          const T p = reg ? p1 : p0;
          sP[(i * n + c) * E + e] = p;
          sP[(c * n + i) * E + e] = p;
        }
      const T pj0 = gv + (sG[(0 * (n + 2) + c) * E + e] * f0 + sG[(1 * (n + 2) + c) * E + e] * f1);
      const T pj1 = pj0 + mu * (k0 * f0 + k1 * f1);
      sp[c * E + e] = reg ? pj1 : pj0;
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
    na0 = nn0;
    na1 = nn1;
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

// the launch (os2r_ilqr_box_inst.hip, once per dtype): 1 if there is no kernel for this nq
template <typename T>
int launch_ilqr_backward_box(int nq, const IlqrBoxArgs<T>& args, hipStream_t stream);

}  // namespace os2r
