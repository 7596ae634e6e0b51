/*
 * os2r_ukf.h — C-ABI of libos2r_ukf.so, the companion library of libos2r.so for the unscented Kalman filter of many robots: the
 * two launches that make a handle of (4 nq + 1) M forked lanes a Gaussian filter without a Jacobian.  os2ru_ukf_points turns
 * (x, P) into the 2n + 1 sigma points of every robot (a Cholesky factor per robot) in the layout os2r_set_state takes;
 * os2r_step pushes them through the real step; os2ru_ukf_update turns what os2r_get_state returns back into (x, P), updates both
 * against the measurement and, if asked, writes the sigma points of the result: one launch of this library per filter step.
 *
 * Like os2r_ekf.h it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are the same: every
 * entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed as
 * `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller, all `*_host`
 * pointers host memory that is read before the call returns.  The error text belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 *
 * Common to both entry points.  M = nrobots, n = 2 layout->nq, S = 2 n + 1, D = layout->obs_dim.  The lane of point s of robot m
 * is s M + m -- the order in which copy_envs_from(real, arange(S M) % M) forks --, so a sigma handle has N = S M lanes.  Every
 * floating-point device array is in layout->dtype with the robot (or lane) index fastest.  Of the layout dtype, nq (2..5),
 * device and, in os2ru_ukf_update, obs_dim and slot_col are read.
 * The scalars gamma, wm0, wc0 and wi (gym_os2r_amd/ukf.py: weights()) are doubles, each rounded once to the dtype and passed as
 * a kernel argument: the spread of the points, the weight of point 0 in the mean, its weight in the covariance, and the weight
 * of every other point in both.  All must be finite, gamma > 0 and wi > 0; wm0 and wc0 may have either sign.
 * Arithmetic (part of the contract): layout->dtype throughout, every product rounded on its own (no fused multiply-add), every
 * sum of products sum_l x_l y_l formed as ((x_0 y_0 + x_1 y_1) + x_2 y_2) + ... with l ascending, every sum of values likewise
 * from the left, every division one IEEE division and every square root one correctly rounded IEEE square root, in fp32 too.
 * The sign of a zero and the sign and payload of a NaN are not part of the contract.  "Finite" and "> 0" are decided on bit
 * patterns.
 * Out of scope: the periodic wrap of an innovation or of the sigma mean (an angle is averaged and compared as a number), slots
 * that are not raw (slot_col -1 carries no update), an augmented state or noise that is not additive, the square-root form of the
 * filter, weights per robot, and several filter steps per launch.
 */
#ifndef OS2R_UKF_H_
#define OS2R_UKF_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_UKF_ABI_VERSION 1

OS2R_API int os2ru_abi_version(void);
OS2R_API const char* os2ru_last_error(void); /* of the calling thread's last failed call */

/* The sigma points of many robots in one launch.
 * Inputs (read only):
 *   x_dev       [n][M]: the state, q rows then qd rows
 *   p_dev       [n][n][M]: the covariance; only the upper triangle (i <= j) is read
 *   gamma       the spread: sqrt(n + lambda)
 * Outputs (each written completely on every call):
 *   points_dev  [n][S M], required: row i of point s of robot m at [i][s M + m].  Rows 0..nq-1 are q and rows nq..n-1 are qd:
 *               points_dev and points_dev + nq S M are what os2r_set_state takes on a handle of S M lanes, without a copy
 *   failed_dev  nullable, [M] int32: 0, or j + 1 where the factor failed at column j
 * For robot m, P[i][j] (i <= j) read from p_dev, the lower triangular factor L with L L' = P is built column by column,
 * j = 0 .. n-1:
 *   t = P[j][j] - sum_{l<j} L[j][l] L[j][l]   (j = 0: t = P[0][0]; otherwise the sum is formed first and subtracted once)
 *   if t is not finite or not > 0: failed = j + 1 and the factor stops
 *   L[j][j] = sqrt(t)
 *   for i > j: L[i][j] = (P[j][i] - sum_{l<j} L[i][l] L[j][l]) / L[j][j]   (j = 0: P[0][i] / L[0][0])
 *   for i < j: L[i][j] = 0 exactly
 * The points, with g = gamma L[i][j] rounded once: chi_0 = x; chi_{1+j}[i] = x_i + g; chi_{1+n+j}[i] = x_i - g  (so
 * chi_{1+j}[i] = chi_{1+n+j}[i] = x_i for i < j).  A robot whose factor failed gets all S points equal to x and
 * failed[m] = j + 1 of the first column that failed; otherwise failed[m] = 0.
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Errors, each with a text of its own that starts with "os2ru_ukf_points: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype or nq; nrobots < 1; n S nrobots above 2^31 - 1; a null
 * x_dev, p_dev or points_dev; a gamma that is not finite or not > 0; a points_dev that overlaps x_dev or p_dev.
 * OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2ru_ukf_points(const Os2rControlLayout* layout, int64_t nrobots, const void* x_dev, const void* p_dev, double gamma,
                              void* points_dev, int32_t* failed_dev, void* stream);

/* The unscented Kalman filter update of many robots in one launch: the prediction of mean and covariance from the propagated
 * sigma points, the measurement update of os2re_ekf_update (include/os2r_ekf.h, steps 2 and 3) on them -- the raw observation
 * slots are selections of state columns, so the unscented measurement update on P- is exactly that sequence of scalar updates
 * --, and the sigma points of the result.
 * Inputs (read only):
 *   q_dev, qd_dev  [nq][S M] each: os2r_get_state's two arrays of the sigma handle after the step; chi_s[i] of robot m is
 *                q_dev[i][s M + m] for i < nq and qd_dev[i - nq][s M + m] otherwise
 *   done_dev     nullable, [S M] uint8: that step's done flags
 *   p_in_dev     [n][n][M]: the covariance before the step; only the upper triangle is read, and it is used for lost robots only
 *   q_host       [n][n] row-major doubles, required, the additive process noise: finite and exactly symmetric, rounded once to the
 *                dtype and passed as kernel arguments, as in os2re_ekf_update
 *   gamma, wm0, wc0, wi   as above; gamma is used in step 4 only
 *   meas_dev     [M][D], prec_dev [D], gate: exactly as in os2re_ekf_update (a reading that is not finite did not arrive; a prec
 *                entry that is not finite or not > 0 drops the slot; gate finite and >= 0, 0: no gate, a value above the
 *                dtype's largest finite number is taken as that number)
 * Outputs (each written completely on every call; null: not wanted):
 *   x_out_dev    [n][M], required
 *   p_out_dev    [n][n][M], required, both triangles written; may be the very pointer p_in_dev, any other overlap is refused
 *   nis_dev      nullable, [M];  used_dev, refused_dev  nullable, [M] int32;  innov_dev  nullable, [M][D]: as in os2re_ekf_update
 *   lost_dev     nullable, [M] int32: 1 for a lost robot (step 1), else 0
 *   points_out_dev  nullable, [n][S M]: the sigma points of (x_out, p_out) (step 4); may overlap neither q_dev nor qd_dev
 *   failed_dev   nullable, [M] int32, only together with points_out_dev: as in os2ru_ukf_points
 * For robot m:
 *   1. The robot is lost when any of its S lanes has done != 0 or a component of chi_s that is not finite; lost[m] = 1.
 *      Lost: x = chi_0 and P- = p_in made symmetric from its upper triangle; no Q is added.  (If chi_0 itself is not finite, x is
 *      whatever it holds and the slots refuse themselves in step 2b / 2c.)
 *      Otherwise, for every i: acc_i = ((chi_1[i] + chi_2[i]) + chi_3[i]) + ... + chi_2n[i];
 *      xbar_i = wm0 chi_0[i] + wi acc_i;  d_s[i] = chi_s[i] - xbar_i for s = 0 .. 2n;  and for i <= j
 *      P-[i][j] = Q[i][j] + (wc0 (d_0[i] d_0[j]) + wi sum_{s=1..2n} d_s[i] d_s[j]),  P-[j][i] = P-[i][j];  x = xbar.
 *      In both cases nis = 0, used = refused = 0
 *   2., 3. steps 2 and 3 of os2re_ekf_update, word for word, on this x and P-: the slots d = 0 .. D-1 with c = slot_col[d], the
 *      skips, the refusals, the gate, k_i = P[i][c] / s, x_i <- x_i + k_i v, P[i][j] <- P[i][j] - k_i P[c][j] for i <= j mirrored,
 *      nis, used, innov; then x_out = x, p_out = P, nis_dev[m] = nis
 *   4. with points_out_dev: the points of (x_out, p_out) by the arithmetic of os2ru_ukf_points with gamma, and failed_dev as
 *      there: bit for bit what a separate os2ru_ukf_points call on the outputs writes
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Errors, each with a text of its own that starts with "os2ru_ukf_update: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype or nq; an obs_dim outside 1..OS2R_MAX_OBS; a slot_col
 * entry outside -1..n-1; nrobots < 1; n S nrobots above 2^31 - 1 (which bounds n n nrobots too); a null q_dev, qd_dev, p_in_dev,
 * q_host, meas_dev, prec_dev, x_out_dev or p_out_dev; a Q that is not finite or not symmetric; a gate that is not finite or is
 * negative; a gamma, wm0, wc0 or wi that is not finite; gamma or wi not > 0; a p_out_dev that overlaps p_in_dev without being
 * equal to it; a points_out_dev that overlaps q_dev or qd_dev; failed_dev without points_out_dev.
 * OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2ru_ukf_update(const Os2rControlLayout* layout, int64_t nrobots, const void* q_dev, const void* qd_dev,
                              const uint8_t* done_dev, const void* p_in_dev, const double* q_host, double gamma, double wm0, double wc0,
                              double wi, const void* meas_dev, const void* prec_dev, double gate, void* x_out_dev, void* p_out_dev,
                              void* nis_dev, int32_t* used_dev, int32_t* refused_dev, void* innov_dev, int32_t* lost_dev,
                              void* points_out_dev, int32_t* failed_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_UKF_H_ */
