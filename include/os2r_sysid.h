/*
 * os2r_sysid.h — C-ABI of libos2r_sysid.so, the companion library of libos2r.so for system identification: which per-environment
 * parameters (mass scale, damping, friction, contact friction, gravity) make the simulator reproduce a logged trajectory.  The
 * route is central finite differences over lanes of the stepper and a Gauss-Newton system with a Levenberg-Marquardt step
 * (Levenberg 1944, Marquardt 1963) per parameter set: before a rollout os2ri_perturb writes, for every logged segment, a nominal
 * parameter lane and a raised and a lowered lane per identified parameter; after the rollout of the logged actions os2ri_update
 * forms the normal equations from the lanes' observations and the measured ones, accepts or rejects the point the lanes were
 * made at, adapts the damping lam of every set on the device and writes the point the next os2ri_perturb takes.  No host decision
 * is in the loop.  A rejected iteration has therefore spent its 2 P perturbed lanes on a point that is thrown away: that is the
 * price of a loop without a host, and it is paid knowingly.
 *
 * Like the other companion headers it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are
 * theirs: every entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed
 * as `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller, all `*_host`
 * pointers host memory that is read before the call returns.  The error text belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 *
 * Out of scope: the periodic wrap of an angle residual (use the raw-observation tasks, or small residuals); bounds, steps or
 * constants per set; forward (one-sided) differences with P + 1 lanes; parameters outside the five fields (link lengths,
 * inertias, centres of mass); a covariance / Cramer-Rao output; robust losses; an active-set treatment of the bounds instead of
 * the clamp; segments of unequal length; analytic parameter derivatives; identifying across a reset; and in-place state
 * updates: an output may not overlap an input or another output, so the caller swaps two state sets.
 */
#ifndef OS2R_SYSID_H_
#define OS2R_SYSID_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_PARAM_*, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_SYSID_ABI_VERSION 1
#define OS2RI_MAX_PARAMS 21 /* 4 OS2R_MAX_DOF + 1: every entry of the five parameter fields */
/* The partial sums every sum over the segments of a set is defined in (update, step 3). */
#define OS2RI_CHUNKS 64
#define OS2RI_MAX_SETS 67108863 /* 2^26 - 1: a wave per set, and a grid holds fewer than 2^32 threads */

/* The scalars of the update, on the host; each is rounded once to T.  gym_os2r_amd.sysid.constants() fills it. */
typedef struct Os2riConstants {
  double shrink, grow;     /* lam <- max(lam shrink, lam_min) behind an accepted point, lam grow behind a rejected one */
  double lam_min, lam_max; /* lam_min >= 0; a rejected point whose lam passes lam_max freezes the set (status 2) */
  double diag_floor;       /* > 0: the damping of parameter p is lam max(H_pp, diag_floor) */
  double tol;              /* an accepted point whose decrease is at most tol times the old cost freezes the set (status 1) */
  double cost_floor;       /* and so does one whose cost is at most cost_floor */
} Os2riConstants;

OS2R_API int os2ri_abi_version(void);
OS2R_API const char* os2ri_last_error(void); /* of the calling thread's last failed call */

/* Common to both calls.  P = nparams identified parameters (1..OS2RI_MAX_PARAMS), T = nsets parameter sets (one per robot being
 * identified, 1..OS2RI_MAX_SETS), M = nsegments logged segments, a multiple of T: segment m belongs to set m mod T.  S = 2 P + 1 lanes per segment,
 * N = S M <= 2^31 - 1 lanes in all; lane s M + m of segment m is the nominal one (s = 0), the one with parameter p raised
 * (s = 1 + p) or lowered (s = 1 + P + p).  Every floating-point device array is in layout->dtype (T below).  Of the layout dtype,
 * nq (2..5, as everywhere), device and obs_dim are read; slot_col is not.
 * sel_host, int32 [P][2]: parameter p is entry sel[p][1] of the field sel[p][0] (OS2R_PARAM_MASS_SCALE .. OS2R_PARAM_GRAVITY; the
 * entry is 0..nq-1, 0 for gravity).  No pair may appear twice.  Parameters travel as one packed array of F = 4 nq + 1 rows in
 * field order (mass scale, damping, friction, mu, gravity), so that the rows of field f are, without a copy, the [count][lanes]
 * array os2r_set_params takes for f; row(p) = sel[p][0] nq + sel[p][1].
 * h_host, lo_host, hi_host, double [P]: the finite-difference step of parameter p, finite and > 0 also when rounded to T, and its
 * bounds, lo <= hi, -inf and +inf allowed; each is rounded once to T.
 * The points of parameter p about theta: plus = min(theta + h, hi), minus = max(theta - h, lo), the sum and the difference
 * rounded, min(a, b) = (a > b ? b : a), max(a, b) = (a < b ? b : a); Delta = plus - minus.  At a bound the difference quotient
 * turns one-sided on its own, and a parameter with lo = hi = theta has Delta = 0 and is held (update, step 4).
 * Arithmetic (part of the contract of both calls): T throughout, every product, sum, difference and quotient rounded on its own
 * (NOT contracted: no fused multiply-add), the division and the square root correctly rounded.  "Finite" and "> 0" are decided
 * on bit patterns.  The sign of a zero is not part of the contract. */

/* The parameter lanes of an iteration (one launch, a thread per row and lane, the lane index fastest).
 * Inputs (read only):
 *   theta_dev   [T][P], required: the point of every set
 *   base_dev    [F][M], required: the parameters of every segment apart from the identified ones
 * Output:
 *   params_dev  [F][N], required: params[r][s M + m] = base[r][m], but where r = row(p): theta[m mod T][p], or plus in the lane
 *               s = 1 + p and minus in the lane s = 1 + P + p
 * Errors, each with a text of its own that starts with "os2ri_perturb: ", all found before the first HIP call (a refused call
 * writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype or nq; nparams outside 1..OS2RI_MAX_PARAMS; nsets outside
 * 1..OS2RI_MAX_SETS; nsegments < 1 or no multiple of nsets; (2 nparams + 1) nsegments above 2^31 - 1; (4 nq + 1) (2 nparams + 1)
 * nsegments, the entries of params_dev (a thread each), above 2^32 - 1; a null sel_host, h_host, lo_host or hi_host;
 * a field or an entry of sel_host out of range, or a pair that appears twice; an h that is not finite and > 0; a bound that is
 * a NaN, or lo > hi; a null theta_dev, base_dev or params_dev; an output that overlaps an input.  OS2R_ERR_NO_DEVICE where
 * layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2ri_perturb(const Os2rControlLayout* layout, int32_t nparams, int64_t nsets, int64_t nsegments, const int32_t* sel_host,
                           const double* h_host, const double* lo_host, const double* hi_host, const void* theta_dev,
                           const void* base_dev, void* params_dev, void* stream);

/* The update of every set from the rollout of its lanes (three stream-ordered launches: per segment its sums; per set and sum
 * the total over the set's valid segments; per set the verdict on the point, the new damping and the next point.  Each reads
 * what the one before wrote into sums_dev and counts_dev).  K = nsteps env-steps per segment, D = layout->obs_dim
 * (1..OS2R_MAX_OBS), E = P (P + 1) / 2 + P + 1 sums.
 * Inputs (read only):
 *   obs_dev     [K][N][D], required: the observations of the lanes, as os2r_rollout wrote them
 *   meas_dev    [K][M][D], required: the measured observations of the segments; a reading that is not finite did not arrive
 *   done_dev    uint8 [K][N], nullable: the done flags of the rollout
 *   prec_dev    [D], required: the weight of every observation slot; a slot whose prec is not finite and > 0 is dropped
 *   theta_dev   [T][P], required, and h_host, lo_host, hi_host: those of the os2ri_perturb call that made the lanes
 *   theta_best_dev [T][P], cost_best_dev [T], hess_dev [T][P][P], grad_dev [T][P], lam_dev [T], status_dev int32 [T],
 *   iters_dev int32 [T]: the state before, required.  A fresh state has cost_best = +inf, status = 0 and iters = 0
 *   constants   on the host, required, every field finite: lam_min >= 0, diag_floor > 0
 * Outputs (null: not wanted; every entry of a given output is written on every successful call):
 *   theta_best_out_dev, cost_best_out_dev, hess_out_dev, grad_out_dev, lam_out_dev, status_out_dev, iters_out_dev: the state
 *               after, required
 *   theta_next_dev [T][P], required: the point the next os2ri_perturb takes
 *   cost_dev    [T], nullable: the cost J of the point, cost_best where the set did not run
 *   valid_dev   int32 [T], nullable: the valid segments of the set
 *   accepted_dev uint8 [T], nullable
 *   failed_dev  int32 [T], nullable: 0, or the column + 1 at which the factor of the damped system failed
 *   delta_dev   [T][P], nullable: the step that was added to theta_best
 * Scratch, owned by the caller, written and read by the call:
 *   sums_dev    E (M + T) elements, required: [E][M], the sums of every segment, and behind it [E][T], those of every set
 *   counts_dev  int32 [M + T], required: whether segment m is valid, and behind the M segments the valid segments of every set
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 *   1. per segment m, for every step k ascending and within it every kept slot d ascending whose meas[k][m][d] is finite, with
 *      w = prec[d]: r = obs[k][m][d] - meas[k][m][d] (the nominal lane); d_p = obs[k][(1 + p) M + m][d] - obs[k][(1 + P + p) M + m][d];
 *      wr = w r; wd_p = w d_p; the chains, each onto 0:  c = c + wr r;  b_p = b_p + wd_p r;  G_pq = G_pq + wd_p d_q for q <= p.
 *      Sum 0 is c, sum 1 + p is b_p, sum 1 + P + p (p + 1) / 2 + q is G_pq.
 *   2. segment m is valid iff no lane of it has a non-zero done byte in the K steps and every one of its E sums is finite
 *   3. a sum over the segments of set t is in OS2RI_CHUNKS = 64 partials: partial i adds the terms of the valid segments
 *      j T + t with j = i, i + 64, ... in ascending order onto 0 (an empty partial is 0), and the total is the adjacent-pair tree
 *      ((p0 + p1) + (p2 + p3)) + ... to depth 6
 *   4. a set whose status is not 0 passes its state through bit for bit, and theta_next = theta_best; so does a set without a
 *      valid segment, except that its theta_next = theta.  Otherwise, with the totals: J = c / 2; Delta_p as above from theta;
 *      a parameter with Delta_p = 0 is held: g_p = 0, H_pp = 1 and the rest of its row and column 0; for the others
 *      g_p = b_p / Delta_p and H_pq = G_pq / (Delta_p Delta_q), the product rounded first, H_qp the same bits
 *   5. the point is accepted iff J < cost_best, both read as the bit patterns of numbers that are not negative (so that a
 *      fresh +inf loses against every finite cost and against nothing else).  Accepted: theta_best = theta, cost_best = J, the
 *      stored hess and grad become H and g, lam = max(lam shrink, lam_min), and status = 1 where J <= cost_floor or, with a
 *      finite old cost, old - J <= tol old.  Rejected: theta_best, cost_best, hess and grad stay, lam = lam grow, and status = 2
 *      where that lam > lam_max
 *   6. from the stored system and the new lam: A = hess, but A_pp = hess_pp + lam max(hess_pp, diag_floor), the product rounded
 *      first.  Its Cholesky factor by columns j ascending: acc = A[j][j]; for k < j ascending acc = acc - L[j][k] L[j][k]; the
 *      column is refused if acc is not finite or not > 0, then failed = j + 1 and delta = 0; else L[j][j] = sqrt(acc) and below
 *      it, for i > j: acc = A[i][j]; for k < j ascending acc = acc - L[i][k] L[j][k]; L[i][j] = acc / L[j][j].
 *      Forward, i ascending: acc = -grad_i (the sign bit flipped); for k < i ascending acc = acc - L[i][k] y_k; y_i = acc / L[i][i].
 *      Backward, i descending: acc = y_i; for k > i descending acc = acc - L[k][i] delta_k; delta_i = acc / L[i][i]
 *   7. theta_next_p = min(max(theta_best_p + delta_p, lo_p), hi_p); iters = iters + 1
 * Errors, each with a text of its own that starts with "os2ri_update: ", all found before the first HIP call (a refused call
 * writes nothing): those of os2ri_perturb about the layout, the counts, h_host, lo_host and hi_host; a bad obs_dim; nsteps < 1;
 * null constants, a field of it that is not finite, lam_min < 0 or diag_floor <= 0; a null required pointer; an output or a
 * scratch array that overlaps an input, another output or the other scratch array.  OS2R_ERR_NO_DEVICE where layout->device is
 * no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2ri_update(const Os2rControlLayout* layout, int32_t nparams, int64_t nsets, int64_t nsegments, int32_t nsteps,
                          const double* h_host, const double* lo_host, const double* hi_host, const Os2riConstants* constants,
                          const void* obs_dev, const void* meas_dev, const uint8_t* done_dev, const void* prec_dev, const void* theta_dev,
                          const void* theta_best_dev, const void* cost_best_dev, const void* hess_dev, const void* grad_dev,
                          const void* lam_dev, const int32_t* status_dev, const int32_t* iters_dev, void* theta_best_out_dev,
                          void* cost_best_out_dev, void* hess_out_dev, void* grad_out_dev, void* lam_out_dev, int32_t* status_out_dev,
                          int32_t* iters_out_dev, void* theta_next_dev, void* cost_dev, int32_t* valid_dev, uint8_t* accepted_dev,
                          int32_t* failed_dev, void* delta_dev, void* sums_dev, int32_t* counts_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_SYSID_H_ */
