/*
 * os2r_search.h — C-ABI of libos2r_search.so, the companion library of libos2r.so and libos2r_control.so for the forward-pass
 * evaluation of iLQR: the line search over the candidates a recorded os2r_rollout_policy_scheduled returned.
 *
 * Like os2r_control.h it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are the same: every
 * entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed as
 * `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller, all `*_host`
 * pointers host memory that is read before the call returns.  The error text belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 */
#ifndef OS2R_SEARCH_H_
#define OS2R_SEARCH_H_

#include "os2r_control.h" /* Os2rControlLayout, OS2RC_MAX_ALPHAS; through it os2r.h: OS2R_API, the dtypes, the status codes */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_SEARCH_ABI_VERSION 1
#define OS2RS_ACCEPT_ALWAYS 1u /* flags: a candidate need not lower cost_dev (which is then not read) */

OS2R_API int os2rs_abi_version(void);
OS2R_API const char* os2rs_last_error(void); /* of the calling thread's last failed call */

/* The line search of iLQR for many independent trajectories in one launch: the cost of every candidate, one accepted step size
 * per trajectory, the nominal updated in place where a step was accepted -- actions, knot observations, cost and the gradients
 * os2rc_ilqr_backward reads, in its layout -- and the index that moves exactly the accepted knots.
 * With K = nknots, M = ntraj, nalpha candidates, N = nalpha M, L = K M, D = layout->obs_dim, n = 2 layout->nq: candidate lane
 * j = i M + m is trajectory m under step size i, the environment order of the handle os2rc_ilqr_backward's table is made for.
 * Every floating-point device array is in layout->dtype.  Of the layout dtype, nq, device, obs_dim and slot_col are read.
 * Inputs (read only):
 *   knot_obs_dev   [K][N][D]: the observation at the top of env-step k (want_knot_obs of the recorded rollout)
 *   end_obs_dev    [N][D]: the observation after the last step (row K-1 of the rollout's obs)
 *   act_dev        [K][N][2]: the applied actions; clamped to [-1, 1] on read, as os2r_linearize and os2rc_ilqr_backward do.  What
 *                  the clamp makes of a NaN is not part of the contract (it may propagate or become -1 or 1); a rollout applies none
 *   done_dev       nullable, [K][N] uint8: a candidate with any nonzero entry is not acceptable (an episode that ended inside it
 *                  makes its cost meaningless)
 *   target_dev     [M][D]: the target observation of trajectory m; only raw slots (slot_col[d] >= 0) are read
 *   q_host         [n][n] row-major doubles, r_host [2][2]: the cost Hessians, as in os2rc_ilqr_backward: finite, exactly
 *                  symmetric, rounded once to the dtype, passed as kernel arguments
 *   qf_host        nullable, [n][n]: the terminal Hessian, same rules; NULL: q_host
 *   flags          OS2RS_ACCEPT_ALWAYS or 0
 * The nominal, in and out -- the kernel reads only cost_dev, and writes each array only at the entries of trajectories that
 * accepted a candidate; every other byte is left as it was:
 *   cost_dev       [M], required; read unless OS2RS_ACCEPT_ALWAYS is set
 *   act_nom_dev    nullable, [K][M][2]
 *   obs_nom_dev    nullable, [K][M][D]
 *   end_nom_dev    nullable, [M][D]
 *   lx_dev         nullable, [n][L]; lu_dev nullable, [2][L]; pvec_final_dev nullable, [n][M]: the layouts os2rc_ilqr_backward reads
 * Pure outputs (every entry written on every call):
 *   choice_dev     [M] int32, required: the accepted candidate i, or -1
 *   index_dev      nullable, [L] int32: entry k M + m is k N + i M + m where trajectory m accepted candidate i, else -1: the index
 *                  os2r_copy_envs takes on a K M-lane knots handle from the K N-lane handle the rollout recorded into (a negative
 *                  entry keeps the lane)
 *   cand_cost_dev  nullable, [nalpha][M]: the cost of every candidate
 * The call does no host synchronisation, no allocation and no write outside these arrays.  Input and output arrays must not
 * overlap.
 * Arithmetic (part of the contract): layout->dtype throughout, every product rounded on its own (no fused multiply-add), every
 * sum of products sum_l x_l y_l evaluated as ((x_0 y_0 + x_1 y_1) + x_2 y_2) + ... with l ascending.  The sign of a zero is not
 * part of the contract.  For candidate lane j of trajectory m:
 *   1. at knot k, o is row j of knot_obs[k] and a_c = clamp(act[k][j][c], -1, 1)
 *   2. e[c], c < n, is o[d] - target[m][d] for the lowest raw slot d with slot_col[d] == c, and 0 if no slot shows column c
 *   3. gx[r] = sum_c Q[r][c] e[c] over all c < n;  sx = 0.5 sum_r e[r] gx[r]
 *   4. gu[c] = R[c][0] a_0 + R[c][1] a_1;  su = 0.5 (a_0 gu[0] + a_1 gu[1])
 *   5. J = (J + sx) + su, starting from J = 0, with k ascending
 *   6. behind the last knot e is formed from end_obs[j]:  gf[r] = sum_c Qf[r][c] e[c];  J = J + 0.5 sum_r e[r] gf[r]
 *   7. candidate i is acceptable when J is finite (tested on the bit pattern), no done entry of lane j is nonzero, and either
 *      OS2RS_ACCEPT_ALWAYS is set or J < cost[m];  choice[m] is the acceptable candidate with the smallest J, ties to the lowest
 *      i, and -1 if none is acceptable
 *   8. where choice[m] = i >= 0, with j = i M + m:  cost[m] = J;  act_nom[k][m][c] = a_c (clamped);  obs_nom[k][m][:] = o (all D
 *      slots);  end_nom[m][:] = end_obs[j][:];  lx[r][k M + m] = gx[r];  lu[c][k M + m] = gu[c];  pvec_final[r][m] = gf[r] --
 *      the values of steps 1-6 for that lane, bit for bit
 * With nalpha = 1, OS2RS_ACCEPT_ALWAYS and the first nominal's own recorded rollout as the candidate, the call initialises every
 * nominal array.
 * Errors, each with a text of its own that starts with "os2rs_ilqr_line_search: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype or nq; obs_dim outside 1..12; a slot_col entry outside
 * -1..n-1; nknots or ntraj < 1; nalpha outside 1..OS2RC_MAX_ALPHAS; K nalpha M above 2^31 - 1 (index_dev is int32); unknown flag
 * bits; a null knot_obs_dev, end_obs_dev, act_dev, target_dev, q_host, r_host, cost_dev or choice_dev; a Q, R or Qf that is not
 * finite or not exactly symmetric.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for a
 * failed HIP call. */
OS2R_API int os2rs_ilqr_line_search(const Os2rControlLayout* layout, int32_t nknots, int64_t ntraj, int32_t nalpha, uint32_t flags,
                                    const void* knot_obs_dev, const void* end_obs_dev, const void* act_dev, const uint8_t* done_dev,
                                    const void* target_dev, const double* q_host, const double* r_host, const double* qf_host,
                                    void* cost_dev, void* act_nom_dev, void* obs_nom_dev, void* end_nom_dev, void* lx_dev, void* lu_dev,
                                    void* pvec_final_dev, int32_t* choice_dev, int32_t* index_dev, void* cand_cost_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_SEARCH_H_ */
