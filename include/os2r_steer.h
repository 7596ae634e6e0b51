/*
 * os2r_steer.h — C-ABI of libos2r_steer.so, the companion library of libos2r.so, libos2r_control.so and libos2r_search.so for an
 * iLQR iteration that no host value steers: the backward pass with one regularisation mu per trajectory, read from the device,
 * and the line search that also decides, per trajectory and in the same launch, what becomes of that mu.
 *
 * Like os2r_search.h it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are the same: every
 * entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed as
 * `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller, all `*_host`
 * pointers host memory that is read before the call returns.  The error text belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 */
#ifndef OS2R_STEER_H_
#define OS2R_STEER_H_

#include "os2r_control.h" /* Os2rControlLayout, OS2RC_MAX_ALPHAS; through it os2r.h: OS2R_API, the dtypes, the status codes */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_STEER_ABI_VERSION 1
#define OS2RT_ACTIVE 0    /* status: the trajectory is being optimised */
#define OS2RT_CONVERGED 1 /* status: an accepted step lowered the cost by no more than tol |cost| */
#define OS2RT_STALLED 2   /* status: nothing was accepted and mu cannot be raised any further (or is invalid) */

/* How os2rt_ilqr_steer judges a step and moves mu; every member is finite and rounded once to the layout's dtype. */
typedef struct Os2rSteerRule {
  double armijo;   /* >= 0; 0: no test on the predicted change */
  double shrink;   /* 0..1: mu after an accepted step is shrink mu ... */
  double grow;     /* >= 1: mu after a rejected iteration is max(grow mu, mu_start) */
  double mu_floor; /* >= 0: ... unless mu <= mu_floor, then it is 0 */
  double mu_start; /* > 0 */
  double mu_max;   /* >= mu_start: a trajectory whose mu would pass it stalls */
  double tol;      /* >= 0; 0: nothing ever converges */
} Os2rSteerRule;

OS2R_API int os2rt_abi_version(void);
OS2R_API const char* os2rt_last_error(void); /* of the calling thread's last failed call */

/* os2rc_ilqr_backward (os2r_control.h) with one mu per trajectory: every argument but mu_dev is that call's, and so are the
 * layouts, the outputs and the arithmetic, steps 1-10 there, with mu read per trajectory:
 *   mu_dev         [M], layout->dtype, required, read only
 * For every trajectory m every output is bit for bit what os2rc_ilqr_backward writes for that trajectory when called with
 * mu = mu[m].  Where mu[m] == 0, T is S itself and the last terms of steps 7 and 8 are skipped (by a select, not by adding a
 * zero).  A mu[m] that is negative or not finite (tested on the bit pattern) cannot be refused by the host without a
 * synchronisation: that trajectory runs as mu = 0 with every knot refused -- flag 1, K = 0, k = 0, the recursion going on with
 * those values.
 * The call does no host synchronisation, no allocation and no write outside the outputs.
 * Errors, each with a text of its own that starts with "os2rt_ilqr_backward_mu: ", all found before the first HIP call (a refused
 * call writes nothing): those of os2rc_ilqr_backward without the two about mu, and OS2R_ERR_INVALID for a null mu_dev.
 * OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rt_ilqr_backward_mu(const Os2rControlLayout* layout, int32_t nknots, int64_t ntraj,
                                    const void* a_dev, const void* b_dev, const void* lx_dev, const void* lu_dev,
                                    const double* q_host, const double* r_host, const void* mu_dev,
                                    const void* pmat_final_dev, const void* pvec_final_dev,
                                    void* gain_dev, void* ff_dev, void* pmat_out_dev, void* pvec_out_dev, uint8_t* flag_dev, void* dv_dev,
                                    const void* actions_dev, const void* obs_dev, const double* alpha_host, int32_t nalpha, void* weights_dev,
                                    void* stream);

/* os2rs_ilqr_line_search (os2r_search.h) that also applies, per trajectory and in the same launch, an Armijo test on the
 * predicted change, the update of mu, a convergence test and a freeze.  K, M, N, L, D, n and every argument that
 * os2rs_ilqr_line_search has too are as there (there are no flags); in addition:
 *   dv_dev         [K][2][M], read only: as os2rc_ilqr_backward writes it
 *   alpha_host     [nalpha]: the candidates' step sizes, finite, rounded once to the dtype, passed as kernel arguments
 *   rule_host      the rule above
 *   mu_dev         [M] (dtype), status_dev [M] int32: required, in and out
 *   iters_dev      nullable, [M] int32, in and out: the accepted steps of a trajectory
 * The nominal (cost_dev, which is always read, and the nullable arrays) is written only at the entries of trajectories that
 * accepted a candidate; choice_dev, index_dev and cand_cost_dev are written at every entry on every call.  The call does no host
 * synchronisation, no allocation and no write outside these arrays.  Input and output arrays must not overlap.
 * Arithmetic (part of the contract), under the rules of os2r_search.h: layout->dtype throughout, every product rounded on its
 * own, sums ascending.  Per trajectory m:
 *   1. the cost J of every candidate: steps 1-6 of os2r_search.h, unchanged
 *   2. d1 = sum_k dv[k][0][m], d2 = sum_k dv[k][1][m], with k ascending, starting from the first term
 *   3. candidate i is acceptable when status[m] == 0; step 7 of os2r_search.h holds (J finite, no done entry, J < cost[m]); and,
 *      when armijo != 0, e = (alpha_i d1) + ((alpha_i alpha_i) d2) is finite (on its bit pattern) and
 *      cost[m] - J >= armijo (-e).  With armijo == 0 the third condition is skipped, and with every status 0 the choice, index,
 *      cost and nominal are then those of os2rs_ilqr_line_search bit for bit
 *   4. choice[m] is the acceptable candidate with the smallest J, ties to the lowest i, and -1 if none is acceptable
 *   5. where a candidate is accepted: the nominal is updated as in step 8 of os2r_search.h;
 *      mu[m] = mu[m] > mu_floor ? shrink mu[m] : 0;  iters[m] += 1;  status[m] = 1 if cost_old - J <= tol |cost_old|, else it
 *      stays 0 (with tol == 0 nothing ever converges)
 *   6. where the trajectory is active and nothing is accepted: t = max(grow mu[m], mu_start); if t > mu_max, or mu[m] is negative
 *      or not finite, status[m] = 2 and mu[m] is left as it is; otherwise mu[m] = t
 *   7. where status[m] != 0 on entry, choice is -1 and the index entries are -1; cand_cost is still written; nothing else of the
 *      trajectory is touched
 * Errors, each with a text of its own that starts with "os2rt_ilqr_steer: ", all found before the first HIP call (a refused call
 * writes nothing): those of os2rs_ilqr_line_search without the one about flags, and OS2R_ERR_INVALID for a null dv_dev,
 * alpha_host, rule_host, mu_dev or status_dev; an alpha that is not finite; a rule member that is not finite; armijo < 0; shrink
 * outside 0..1; grow < 1; mu_floor < 0; mu_start <= 0; mu_max < mu_start; tol < 0.  OS2R_ERR_NO_DEVICE where layout->device is
 * no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rt_ilqr_steer(const Os2rControlLayout* layout, int32_t nknots, int64_t ntraj, int32_t nalpha,
                              const void* knot_obs_dev, const void* end_obs_dev, const void* act_dev, const uint8_t* done_dev,
                              const void* target_dev, const double* q_host, const double* r_host, const double* qf_host,
                              const void* dv_dev, const double* alpha_host, const Os2rSteerRule* rule_host,
                              void* cost_dev, void* act_nom_dev, void* obs_nom_dev, void* end_nom_dev, void* lx_dev, void* lu_dev,
                              void* pvec_final_dev, void* mu_dev, int32_t* status_dev, int32_t* iters_dev,
                              int32_t* choice_dev, int32_t* index_dev, void* cand_cost_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_STEER_H_ */
