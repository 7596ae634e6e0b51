/*
 * os2r_box.h — C-ABI of libos2r_box.so, the companion library of libos2r.so, libos2r_control.so and libos2r_steer.so for the
 * backward pass of iLQR under box limits on the two actions (control-limited DDP: Tassa, Mansard and Todorov, ICRA 2014).
 *
 * Like os2r_steer.h it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are the same: every
 * entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed as
 * `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller, all `*_host`
 * pointers host memory that is read before the call returns.  The error text belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 */
#ifndef OS2R_BOX_H_
#define OS2R_BOX_H_

#include "os2r_control.h" /* Os2rControlLayout, OS2RC_MAX_ALPHAS; through it os2r.h: OS2R_API, the dtypes, the status codes */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_BOX_ABI_VERSION 1

OS2R_API int os2rb_abi_version(void);
OS2R_API const char* os2rb_last_error(void); /* of the calling thread's last failed call */

/* os2rt_ilqr_backward_mu (os2r_steer.h) whose feed-forward step stays inside a box around the nominal action.  Every argument
 * that os2rt_ilqr_backward_mu has means what it means there -- the same layouts, the same nullability --, except:
 *   mu, mu_dev     mu_dev == NULL: the scalar mu regularises every trajectory, finite and >= 0, rounded once, as in
 *                  os2rc_ilqr_backward.  Otherwise mu_dev [M] (layout->dtype, read only) holds one mu per trajectory and the scalar
 *                  must be 0; an entry that is negative or not finite runs as 0 with every knot of its trajectory refused, as in
 *                  os2r_steer.h
 *   actions_dev    [L][2], required: the nominal actions, the array given to os2r_linearize; the bounds are relative to them
 *   lo_host        [2], hi_host [2]: the limits of the two actions.  lo_host[c] is -infinity (none) or finite in [-1, 1],
 *                  hi_host[c] +infinity (none) or finite in [-1, 1], lo_host[c] < hi_host[c]; rounded once to the dtype
 *   clamp_dev      nullable, [K][M] uint8: which components the limits hold at the knot (B4 below)
 * At least one of gain_dev, ff_dev, pmat_out_dev, pvec_out_dev, dv_dev, weights_dev is required.  The call does no host
 * synchronisation, no allocation and no write outside the outputs.
 * Arithmetic (part of the contract), under the rules of os2r_control.h: layout->dtype throughout, every product rounded on its own
 * (no fused multiply-add), sums ascending, a minus flips the sign bit.  Per knot, steps 1-5 are those of os2r_control.h with mu
 * read per trajectory as in os2r_steer.h (T = S + mu I; with mu == 0, T is S itself).  Then, with c the component, j = 1 - c:
 *   B1. a0_c = min(max(actions[k M + m][c], -1), 1);  dlo_c = lo_c - a0_c,  dhi_c = hi_c - a0_c; an infinite bound stays infinite
 *   B2. the interior: K and k by the expressions of steps 4 and 6 of os2r_control.h, unchanged;
 *       inside = dlo_0 <= k0 <= dhi_0 and dlo_1 <= k1 <= dhi_1, false where k0 or k1 is a NaN.  A knot that is ok (step 2) and
 *       inside is written exactly as os2rt_ilqr_backward_mu writes it, with the clamp byte 0
 *   B3. otherwise, if ok, four candidates on the edges of the box, e = 0..3 = (c, side) = (0, lo), (0, hi), (1, lo), (1, hi), with
 *       b = dlo_c or dhi_c:
 *         a candidate whose bound is infinite is skipped
 *         u = -((Qu_j + T01 b) / T_jj);  pinned = u < dlo_j or u > dhi_j;  u = min(max(u, dlo_j), dhi_j), a NaN staying a NaN
 *         k_c = b,  k_j = u
 *         v = 0.5 (((T00 k0) k0 + (T11 k1) k1) + 2 ((T01 k0) k1)) + (Qu0 k0 + Qu1 k1): the model's value, T regularised
 *         a candidate whose v is not finite is skipped
 *       the candidate with the lowest v wins, ties to the lowest e.  This is exact: the objective is convex, every candidate is
 *       the exact minimum of a clipped 1-D quadratic on its edge, and a corner is reached as a pinned candidate
 *   B4. for the winner: row c of K is 0; row j is 0 if pinned, else K[j][col] = G[j][col] / T_jj; k is the candidate;
 *       clamp = (1 << c) | (pinned ? 1 << j : 0), and bit 2 + i is set where component i is held at its upper bound (c at side hi;
 *       j where the unclipped u > dhi_j).  A knot without a surviving candidate, or one that is not ok, gets K = 0, k = 0, flag 1
 *       and clamp 0, and the recursion goes on with those values
 *   B5. steps 7-10 of os2r_control.h with that K and k, unchanged: with the clamped rows of K zero and (T k + Qu)_j = 0 at a free
 *       component they are the value update of Tassa et al. for any K;  dv keeps its formulas, S unregularised; the weight table
 *       keeps its layout, so os2r_rollout_policy_scheduled, os2rs_ilqr_line_search and os2rt_ilqr_steer take the outputs as
 *       they are
 * With both lo_host entries -infinity and both hi_host entries +infinity every output that os2rt_ilqr_backward_mu has too holds
 * its bits, and clamp_dev is all zero.
 * Errors, each with a text of its own that starts with "os2rb_ilqr_backward_box: ", all found before the first HIP call (a
 * refused call writes nothing): those of os2rc_ilqr_backward (a mu that is negative or not finite included), and
 * OS2R_ERR_INVALID for a null actions_dev, lo_host or hi_host; a bound that is a NaN or the wrong infinity; a finite bound outside
 * [-1, 1]; lo >= hi; mu_dev together with mu != 0.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device,
 * OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rb_ilqr_backward_box(const Os2rControlLayout* layout, int32_t nknots, int64_t ntraj,
                                     const void* a_dev, const void* b_dev, const void* lx_dev, const void* lu_dev,
                                     const double* q_host, const double* r_host, double mu, const void* mu_dev,
                                     const double* lo_host, const double* hi_host,
                                     const void* pmat_final_dev, const void* pvec_final_dev,
                                     void* gain_dev, void* ff_dev, void* pmat_out_dev, void* pvec_out_dev, uint8_t* flag_dev, void* dv_dev,
                                     uint8_t* clamp_dev,
                                     const void* actions_dev, const void* obs_dev, const double* alpha_host, int32_t nalpha, void* weights_dev,
                                     void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_BOX_H_ */
