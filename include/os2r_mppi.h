/*
 * os2r_mppi.h — C-ABI of libos2r_mppi.so, the companion library of libos2r.so for sampling planners: the MPPI update (Williams et
 * al. 2017) of many robots in one launch, on the device arrays a noisy os2r_rollout_policy_scheduled returned, writing the table
 * the next one reads.
 *
 * Like os2r_control.h it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are the same: every
 * entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed as
 * `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller.  The error text
 * belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 */
#ifndef OS2R_MPPI_H_
#define OS2R_MPPI_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_MPPI_ABI_VERSION 1
#define OS2RM_TAIL_ZERO 1u /* flags: the slots the shift uncovers are 0; else the last mean is held */
#define OS2RM_CHUNKS 8     /* the partial sums every sum over the samples is defined in (step 4) */

OS2R_API int os2rm_abi_version(void);
OS2R_API const char* os2rm_last_error(void); /* of the calling thread's last failed call */

/* The MPPI update of many independent robots in one launch: the softmax weights of every robot's samples, the weighted mean of
 * their action sequences, the action to apply now, the shifted nominal, and the bias entries of the per-environment table with
 * which os2r_rollout_policy_scheduled applies clip(nominal + sigma eps) in the next control step.
 * With K = nknots, M = nrobots, S = nsamples, N = S M, D = layout->obs_dim: lane j = s M + m is sample s of robot m, the
 * environment order of a planner handle forked by os2r_copy_envs with index[j] = j mod M (the candidate-major order of
 * os2rs_ilqr_line_search).  Every floating-point device array is in layout->dtype.  Of the layout dtype, nq (2..5, as everywhere),
 * device and, with table_dev, obs_dim are read; slot_col is not.
 * Inputs (read only):
 *   returns_dev     [N]: the return of every lane (higher is better), e.g. the returns of the rollout under
 *                   OS2R_POLICY_FIRST_EPISODE
 *   actions_dev     [K][N][2]: the applied actions of the rollout (its act_out); aligned to a pair of its elements
 *   nominal_in_dev  [K][M][2]: the nominal the samples were drawn about; read only for a robot none of whose lanes is valid
 *   beta            the inverse temperature, finite and > 0; rounded once to the dtype (for OS2R_F32 a value outside the normal
 *                   range of fp32 is refused)
 *   shift           0..K: by how many slots the new nominal moves towards the present
 *   flags           OS2RM_TAIL_ZERO or 0
 * Outputs (every entry written on every call; null: not wanted):
 *   nominal_out_dev [K][M][2], required; must not overlap nominal_in_dev (the workgroup of slot k reads its source slot itself)
 *   applied_dev     nullable, [M][2]
 *   table_dev       nullable, [K][2][D+1][N]: the OS2R_POLICY_PER_ENV table of os2r_rollout_policy_scheduled with period = K for a
 *                   handle of N environments.  ONLY the bias entries [k][j][D][lane] are written; the weight columns are the
 *                   caller's (zero for plain MPPI, a stabilising gain if wanted) and no byte of them is touched
 *   weights_dev     nullable, [S][M]: the unnormalised weight w of every lane (step 3)
 *   ess_dev         nullable, [M]: the effective sample size
 *   count_dev       nullable, [M] int32: the number of valid lanes
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Arithmetic (part of the contract): layout->dtype throughout, every product and sum rounded on its own (no fused multiply-add),
 * every division correctly rounded.  The sign of a zero is not part of the contract.  For robot m:
 *   1. lane s M + m is valid iff its return r is finite (tested on the bit pattern); count[m] is the number of valid lanes
 *   2. rmax is the maximum of r over the valid lanes
 *   3. w_s = exp((r - rmax) beta) for a valid lane, with the device library's exp (within a few ulp of the exact value, exactly 1
 *      at the maximum); w_s = 0 exactly for an invalid lane
 *   4. a sum over s is formed in OS2RM_CHUNKS = 8 partials: partial c adds its terms s = c, c + 8, ... in ascending order onto 0
 *      (an empty partial is 0), and the total is ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)).  The sums are wsum of w_s,
 *      A[k][j] of the rounded products w_s actions[k][s M + m][j], and Q of the rounded products w_s w_s
 *   5. mean[k][m][j] = clamp(A[k][j] / wsum, -1, 1) if count[m] > 0, else nominal_in[k][m][j]
 *   6. ess[m] = (wsum wsum) / Q if count[m] > 0, else 0
 *   7. applied[m][j] = mean[0][m][j]
 *   8. nominal_out[k][m][j] = mean[min(k + shift, K - 1)][m][j]; with OS2RM_TAIL_ZERO it is 0 where k + shift >= K
 *   9. table[k][j][D][s M + m] = nominal_out[k][m][j] for every s
 * Errors, each with a text of its own that starts with "os2rm_mppi_update: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype or nq; nknots, nrobots or nsamples < 1; more than 65535
 * knots; nsamples nrobots above 2^31 - 1; shift outside 0..nknots; unknown flag bits; a beta that is not finite, not > 0, or
 * outside the normal range of fp32 for an fp32 layout; a null returns_dev, actions_dev, nominal_in_dev or nominal_out_dev; an
 * actions_dev that is not aligned to a pair of its elements; overlapping nominals; with table_dev, an obs_dim outside
 * 1..OS2R_MAX_OBS.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device,
 * OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rm_mppi_update(const Os2rControlLayout* layout, int32_t nknots, int64_t nrobots, int32_t nsamples,
                               const void* returns_dev, const void* actions_dev, const void* nominal_in_dev, double beta, int32_t shift,
                               uint32_t flags, void* nominal_out_dev, void* applied_dev, void* table_dev, void* weights_dev,
                               void* ess_dev, int32_t* count_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_MPPI_H_ */
