/*
 * os2r_ekf.h — C-ABI of libos2r_ekf.so, the companion library of libos2r.so for Gaussian state estimation: the Kalman filter
 * update of many robots in one launch -- the covariance prediction P- = A P A' + Q from the Jacobian os2r_linearize wrote, and
 * the measurement update of the state and the covariance against a measured observation, one raw observation slot after the
 * other.  With os2r_linearize before it and os2r_set_state behind it, it is the extended Kalman filter of an estimate handle.
 *
 * Like os2r_pf.h it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are the same: every
 * entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed as
 * `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller, all `*_host`
 * pointers host memory that is read before the call returns.  The error text belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 */
#ifndef OS2R_EKF_H_
#define OS2R_EKF_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_EKF_ABI_VERSION 1

OS2R_API int os2re_abi_version(void);
OS2R_API const char* os2re_last_error(void); /* of the calling thread's last failed call */

/* The Kalman filter update of many independent robots in one launch.  The measurement matrix is a selection of state columns
 * (layout->slot_col) and the measurement noise diagonal, so the update is a sequence of scalar updates: no matrix is inverted,
 * the sequence gives the joint update, and the sum of its scalar normalised innovations squared is the joint one.
 * With M = nrobots, n = 2 layout->nq, D = layout->obs_dim: every floating-point device array is in layout->dtype and
 * struct-of-arrays with the robot index fastest, as in os2r_linearize; meas_dev and innov_dev are [M][D], as os2r_step returns
 * observations.  Of the layout dtype, nq (2..5, as everywhere), device, obs_dim and slot_col are read.
 * Inputs (read only):
 *   x_pred_dev   [n][M]: the predicted state, q rows then qd rows: os2r_linearize's next_dev, or os2r_get_state's two arrays in one
 *   p_in_dev     [n][n][M]: the covariance; only the upper triangle (i <= j) is read
 *   a_dev        nullable, [n][n][M]: os2r_linearize's a_dev.  Null: no time update, P- = P, and q_host is not read
 *   q_host       [n][n] row-major doubles, the process noise: finite and exactly symmetric, rounded once to the dtype and passed as
 *                kernel arguments, as the q_host of os2r_lqr_gains.  Required when a_dev is given
 *   meas_dev     [M][D]: the measured observation of every robot; an entry that is not finite is a reading that did not arrive
 *   prec_dev     [D]: one inverse variance per slot, the prec of os2rp_pf_update; an entry that is not finite or not > 0 drops
 *                the slot
 *   gate         finite and >= 0, rounded once to the dtype (a value above the dtype's largest finite number is taken as that
 *                number).  0: no gate; otherwise a slot whose normalised innovation squared exceeds it is left out for that robot
 * Outputs (each written completely on every call; null: not wanted):
 *   x_out_dev    [n][M], required; may be the very pointer x_pred_dev, any other overlap is refused
 *   p_out_dev    [n][n][M], required, both triangles written; may be the very pointer p_in_dev, any other overlap is refused
 *   nis_dev      nullable, [M]: the sum of the normalised innovations squared of the applied slots (step 3)
 *   used_dev     nullable, [M] int32: bit d set for each slot applied
 *   refused_dev  nullable, [M] int32: bit d set for each slot refused
 *   innov_dev    nullable, [M][D]: the innovation of every applied slot, exactly 0 elsewhere
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Arithmetic (part of the contract): layout->dtype throughout, every product rounded on its own (no fused multiply-add), every
 * sum of products sum_l x_l y_l formed as ((x_0 y_0 + x_1 y_1) + x_2 y_2) + ... with l ascending, every division one IEEE
 * division, in fp32 too.  The sign of a zero and the sign and payload of a NaN are not part of the contract.  "Finite" and
 * "> 0" are decided on bit patterns.  For robot m, with P made symmetric from the upper triangle of p_in:
 *   1. with a_dev: AP[i][j] = sum_l A[i][l] P[l][j]; then for i <= j, P-[i][j] = Q[i][j] + sum_l AP[i][l] A[j][l] and
 *      P-[j][i] = P-[i][j].  Without a_dev: P- = P.  In both cases x = x_pred, nis = 0, used = refused = 0
 *   2. for the slot d = 0 .. D-1 in ascending order, with c = slot_col[d]:
 *      a. the slot is skipped, neither bit set, if c < 0, if prec_d is not finite or not > 0, or if y_d = meas[m][d] is not finite
 *      b. r = 1 / prec_d and s = P[c][c] + r; if s is not finite or not > 0, bit d of refused is set and the slot skipped
 *      c. v = y_d - x_c and z = (v v) / s; if z is not finite, bit d of refused is set and the slot skipped; if gate > 0 and
 *         z > gate, the slot is skipped with neither bit set
 *      d. with the values of P and x from before this slot: k_i = P[i][c] / s for every i; x_i <- x_i + k_i v; for i <= j,
 *         P[i][j] <- P[i][j] - k_i P[c][j], mirrored into P[j][i]; nis <- nis + z; bit d of used is set and innov[m][d] = v
 *   3. x_out = x, p_out = P, nis_dev[m] = nis
 * Two slots may show the same column -- two sensors on one state --: they are applied one after the other.
 * Out of scope: the periodic wrap of an innovation (an angle is compared as a number), slots that are not raw (slot_col -1
 * carries no update), correlated measurement noise, a log-likelihood output, the Joseph form of the covariance update (the
 * simple form above is what is computed; p_out stays bitwise symmetric, its positive definiteness is the caller's to watch
 * through refused_dev), and several filter steps per launch.
 * Errors, each with a text of its own that starts with "os2re_ekf_update: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype or nq; an obs_dim outside 1..OS2R_MAX_OBS; a slot_col
 * entry outside -1..n-1; nrobots < 1; n n nrobots above 2^31 - 1; a null x_pred_dev, p_in_dev, meas_dev, prec_dev, x_out_dev or
 * p_out_dev; a_dev without q_host; a Q that is not finite or not symmetric; a gate that is not finite or is negative; an
 * x_out_dev that overlaps x_pred_dev without being equal to it, and the same for p_out_dev against p_in_dev.
 * OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2re_ekf_update(const Os2rControlLayout* layout, int64_t nrobots, const void* x_pred_dev, const void* p_in_dev,
                              const void* a_dev, const double* q_host, const void* meas_dev, const void* prec_dev, double gate,
                              void* x_out_dev, void* p_out_dev, void* nis_dev, int32_t* used_dev, int32_t* refused_dev,
                              void* innov_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_EKF_H_ */
