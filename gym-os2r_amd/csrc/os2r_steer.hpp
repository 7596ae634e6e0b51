// os2r_steer.hpp — os2rt_ilqr_steer: the line search of iLQR that also steers every trajectory's mu, in one launch (gfx950).
//
// The workgroup and the phases are those of os2r_search.hpp: kSearchTraj = 64 trajectories x nalpha candidates, wave i holds
// candidate i, its lane t trajectory blockIdx.x * 64 + t; phase 1 runs the knots of candidate lane j = i M + m with the next
// knot's values in flight, Q and Qf are read from the kernel-argument segment by scalar loads; after the barrier every lane
// finds its trajectory's choice and the waves share the write-back of the nominal.  The helpers (search_row, search_quad,
// search_act, search_clamp) are os2r_search.hpp's, so the costs and the nominal have its bits.  What is added:
//   before   when the rule has an Armijo constant (a kernel argument: every wave sums or none), the two terms of the predicted
//   phase 1  change, d1 and d2, are summed over the knots, sixteen knots' pairs requested together, and only
//            armijo (-(alpha_i d1 + alpha_i^2 d2)) stays in a register across the knots, alpha_i a scalar operand from the
//            argument segment: the knot loop is os2r_search.hpp's (DESIGN.md section 4 says why the sums do not ride along in it).
//   phase 1  at its end status is requested beside cost, and by wave 0 mu and iters too; the verdict on candidate i also asks
//            cost - J >= that threshold.  A trajectory whose status is not 0 accepts nothing.
//   phase 2  wave 0 writes mu, status and iters next to choice and cost (steps 5 and 6 of include/os2r_steer.h), from what it
//            holds: it waits for no memory before it takes its share of the write-back.
// Tail lanes shadow the last trajectory, their stores are masked.  Every store is an ordinary vector store.  No lane indexes a
// register array at run time, nothing goes to scratch (tests/test_ilqr_steer_host.py reads the metadata).
//
// The arithmetic is the contract of include/os2r_steer.h.  tests/test_ilqr_steer_host.py restates it in numpy, bit for bit.
//
// The knot loop, the scan and the write-back below are still a copy of os2r_search.hpp's text, against the rule of DESIGN.md
// section 4: split into three functions that both kernels call, the fp64 line search measured 3 to 13 % slower
// (profiles/refactor_bodies_ab.txt).  Whoever changes one of the two texts changes the other.
#pragma once
#include "os2r_search.hpp"
#include "os2r_bits.hpp"   // steer_finite, steer_nan, steer_invalid, steer_abs
#include "../../include/os2r_steer.h"

namespace os2r {

template <typename T>
struct SteerArgs {
  SearchArgs<T> base;                  // as os2rs_ilqr_line_search fills it; base.accept_always is not read
  const T* __restrict__ dv;            // [K][2][M]
  T* mu;                               // [M], in and out
  int* status;                         // [M], in and out
  int* iters;                          // [M] or null, in and out
  T armijo, shrink, grow, mu_floor, mu_start, mu_max, tol;   // the rule, rounded to T by the host
  T alpha[OS2RC_MAX_ALPHAS];           // rounded to T by the host
};

template <typename T, int NQ>
__global__ __launch_bounds__(kSearchTraj * OS2RC_MAX_ALPHAS) void ilqr_steer_kernel(const SteerArgs<T> S) {
#pragma clang fp contract(off)
  constexpr int n = 2 * NQ, E = kSearchTraj;
  const SearchArgs<T>& P = S.base;
  __shared__ T sJ[OS2RC_MAX_ALPHAS * E];
  __shared__ int sOk[OS2RC_MAX_ALPHAS * E];
  const int t = threadIdx.x % E, w = threadIdx.x / E;   // w, the candidate, is uniform over a wave
  const long long M = P.M, m_raw = (long long)blockIdx.x * E + t;
  const bool valid = m_raw < M;
  const long long m = valid ? m_raw : M - 1;            // tail lanes shadow the last trajectory, their stores are masked
  const int K = P.K, D = P.D, nalpha = P.nalpha;
  const long long N = (long long)nalpha * M, L = (long long)K * M;
  const long long j = (long long)w * M + m;

  const OS2R_CONST SteerArgs<T>* ka = (const OS2R_CONST SteerArgs<T>*)__builtin_amdgcn_kernarg_segment_ptr();
  const OS2R_CONST T* q = ka->base.q;
  const OS2R_CONST T* qf = ka->base.qf;
  const bool armijo = S.armijo != T(0);                 // a kernel argument: every wave sums d1, d2 or none
  T tg[n];
  search_row<T, n>(P.target + m * D, P.col_slot, tg);
  // the predicted change of the lane's candidate, before phase 1 (only its threshold stays in a register across the knots):
  // d1, d2 summed over the knots, e = alpha d1 + alpha^2 d2, -> armijo (-e)
  T need = T(0);
  bool e_ok = true;
  if (armijo) {
    // sixteen knots' pairs are requested together and then added in order (a pair behind the last knot is the last knot's again
    // and a zero is added in its place): one wave per SIMD hides no latency behind another, so the sums cost one memory round
    // trip per batch, ceil(K / 16) of them, and a load per addition would make that K.  (Thirty-two pairs in fp32 put the nq-2
    // kernel's batch in scratch.)
    constexpr int kBatch = 16;
    const T* dvm = S.dv + m;
    T d1 = T(0), d2 = T(0);
    for (int k = 0; k < K; k += kBatch) {
      T v1[kBatch], v2[kBatch];
#pragma unroll
      for (int b = 0; b < kBatch; ++b) {
        const int kb = k + b < K ? k + b : K - 1;
        v1[b] = dvm[(long long)(2 * kb) * M];
        v2[b] = dvm[(long long)(2 * kb + 1) * M];
      }
#pragma unroll
      for (int b = 0; b < kBatch; ++b) {
        const T x1 = k + b < K ? v1[b] : T(0), x2 = k + b < K ? v2[b] : T(0);
        d1 = k + b == 0 ? x1 : d1 + x1;
        d2 = k + b == 0 ? x2 : d2 + x2;
      }
    }
    const T al = ka->alpha[__builtin_amdgcn_readfirstlane(w)];
    const T e = (al * d1) + ((al * al) * d2);
    e_ok = steer_finite(e);
    need = S.armijo * lqr_neg(e);
  }

  // phase 1: the cost of candidate lane j
  T J = T(0), cost_old, mu = T(0);
  int iters_old = 0;
  bool active;
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
    // what is needed from here on is read from the argument segment afresh (through a pointer the compiler knows nothing about):
    // read from the by-value copy, the pointers and the rule are loaded at the top of the kernel and held across the knots
    asm volatile("" : "+s"(ka));
    cost_old = P.cost[m];
    active = ka->status[m] == 0;
    if (w == 0) {                                       // wave 0 alone updates mu and iters: requested here, beside cost and status,
      mu = ka->mu[m];                                   // so that after the barrier it only computes and stores before it takes its
      if (ka->iters) iters_old = ka->iters[m];          // share of the write-back
    }
    bool ok = active && steer_finite(J) && dn == 0u && J < cost_old;
    if (armijo) ok = ok && e_ok && cost_old - J >= need;
    sJ[w * E + t] = J;
    sOk[w * E + t] = ok ? 1 : 0;
    if (valid && P.cand_cost) P.cand_cost[j] = J;
  }
  __syncthreads();

  // phase 2: the choice of the lane's trajectory (step 4), the same in every wave
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
    T* mu_at = ka->mu + m;
    int* status_at = ka->status + m;
    int* iters = ka->iters;
    if (best >= 0) {                                    // step 5
      P.cost[m] = bestJ;
      const T shrunk = ka->shrink * mu;
      *mu_at = (!steer_nan(mu) && mu > ka->mu_floor) ? shrunk : T(0);
      if (iters) iters[m] = iters_old + 1;
      if (cost_old - bestJ <= ka->tol * steer_abs(cost_old)) *status_at = OS2RT_CONVERGED;
    } else if (active) {                                // step 6
      const T grown = ka->grow * mu;
      const T start = ka->mu_start;
      const T to = grown > start ? grown : start;
      if (steer_invalid(mu) || to > ka->mu_max) *status_at = OS2RT_STALLED;
      else *mu_at = to;
    }
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

// the launch (os2r_steer_inst.hip, once per dtype): 1 if there is no kernel for this nq
template <typename T>
int launch_ilqr_steer(int nq, const SteerArgs<T>& args, hipStream_t stream);

}  // namespace os2r
