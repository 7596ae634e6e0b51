/*
 * os2r_cem.h — C-ABI of libos2r_cem.so, the companion library of libos2r.so for the cross-entropy method (CEM; Rubinstein 1999, as
 * PETS and PlaNet plan with it): the update of many robots in one call, on the device arrays a noisy
 * os2r_rollout_policy_scheduled returned -- the best E of every robot's S lanes, the mean and the width of the sampling
 * distribution refitted from them --, writing the table and the per-lane sigma the next rollout reads.
 *
 * Like os2r_mppi.h it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are the same: every
 * entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed as
 * `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller.  The error text
 * belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 *
 * Out of scope: a sigma per knot (the rollout kernels take one per lane; var_out is there for the day they take more), a full
 * covariance, a number of elites per robot, cost-valued inputs (negate them), elites kept across iterations, coloured or
 * smoothed noise.
 */
#ifndef OS2R_CEM_H_
#define OS2R_CEM_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_CEM_ABI_VERSION 1
#define OS2RX_TAIL_ZERO 1u /* flags: the slots the shift uncovers are 0; else the last mean is held */
#define OS2RX_CHUNKS 8     /* the partial sums every sum over the elites is defined in (step 3) */

OS2R_API int os2rx_abi_version(void);
OS2R_API const char* os2rx_last_error(void); /* of the calling thread's last failed call */

/* The CEM update of many independent robots in one call (two stream-ordered launches): the elite set of every robot's samples,
 * the mean and the variance of the elites' action sequences, the action to apply now, the shifted nominal, the pooled standard
 * deviation as the next sampling width, the bias entries of the per-environment table and the per-lane sigma with which
 * os2r_rollout_policy_scheduled applies clip(nominal + sigma eps) in the next iteration or control step.
 * With K = nknots, M = nrobots, S = nsamples, E = nelite, N = S M, D = layout->obs_dim: lane s M + m is sample s of robot m, the
 * order of os2rm_mppi_update.  Every floating-point device array is in layout->dtype (T below).  Of the layout dtype, nq (2..5,
 * as everywhere), device and, with table_dev, obs_dim are read; slot_col is not.
 * Inputs (read only):
 *   returns_dev     [N]: the return of every lane (higher is better)
 *   actions_dev     [K][N][2]: the applied actions of the rollout (its act_out); aligned to a pair of its elements
 *   nominal_in_dev  [K][M][2]: the nominal the samples were drawn about
 *   sigma_in_dev    [2][M]: the width they were drawn with
 *   gain            in (0, 1]: how far the nominal moves towards the elite mean (1: all the way)
 *   sigma_gain      in (0, 1]: the same for the width
 *   sigma_min, sigma_max   finite, 0 <= sigma_min <= sigma_max: the bounds of the new width
 *                   the four are rounded once to T (for OS2R_F32 a non-zero value outside the normal range of fp32 is refused)
 *   shift           0..K: by how many slots the new nominal moves towards the present
 *   flags           OS2RX_TAIL_ZERO or 0
 * Outputs (every entry written on every successful call; null: not wanted):
 *   nominal_out_dev [K][M][2], required; must not overlap nominal_in_dev
 *   var_out_dev     [K][M][2], required: the variance of the elites at every knot, and the workspace of the pooling (the
 *                   second launch reads it); must not overlap any input
 *   sigma_out_dev   [2][M], required.  It MAY be sigma_in_dev: each robot's entry is read and written by one thread only
 *   applied_dev     nullable, [M][2]
 *   table_dev       nullable, [K][2][D+1][N]: the OS2R_POLICY_PER_ENV table of os2r_rollout_policy_scheduled with period = K for a
 *                   handle of N environments.  ONLY the bias entries [k][j][D][lane] are written, as by os2rm_mppi_update
 *   lane_sigma_dev  nullable, [2][N]: sigma_out of the lane's robot, the layout the rollout kernels read under
 *                   OS2R_POLICY_SIGMA_PER_ENV
 *   elite_dev       nullable, [S][M] int32: 1 for an elite lane, else 0
 *   threshold_dev   nullable, [M]: the lowest elite return, 0 for a robot without a valid lane
 *   count_dev       nullable, [M] int32: the number of valid lanes
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Arithmetic (part of the contract): T throughout, every product, sum and difference rounded on its own (no fused
 * multiply-add), every division and the square root correctly rounded.  The sign of a zero is not part of the contract.  For
 * robot m:
 *   1. lane s M + m is valid iff its return is finite (tested on the bit pattern); count[m] is the number of valid lanes and
 *      e = min(E, count[m])
 *   2. the valid lanes are ordered by return descending, equal returns (-0 and +0 are equal) by sample index ascending; the first
 *      e of them are the elites, threshold[m] is the return of the last elite
 *   3. a sum over the elites is formed in OS2RX_CHUNKS = 8 partials: partial c adds the terms of its elite samples
 *      s = c, c + 8, ... in ascending order onto 0 (lanes that are not elite are skipped, an empty partial is 0), and the total
 *      is ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))
 *   4. mu_e[k][j] = A[k][j] / T(e), A the sum of actions[k][lane][j]; var[k][m][j] = V[k][j] / T(e), V the sum of the rounded
 *      squares d d, d = actions[k][lane][j] - mu_e[k][j]
 *   5. mean[k][j] = clamp(mu_e, -1, 1) if gain == 1, else clamp(nom + gain (mu_e - nom), -1, 1), nom = nominal_in[k][m][j];
 *      with count[m] == 0, mean = nom itself and var = 0
 *   6. nominal_out[k] = mean[min(k + shift, K - 1)]; with OS2RX_TAIL_ZERO it is 0 where k + shift >= K
 *   7. applied[m][j] = mean[0][j]
 *   8. table[k][j][D][s M + m] = nominal_out[k][m][j] for every s
 *   9. sd[j] = sqrt((var[0][m][j] + var[1][m][j] + ... in ascending k onto 0) / T(K))
 *  10. sigma_out[j][m] = clamp(sig, sigma_min, sigma_max), sig = sd[j] if sigma_gain == 1, else
 *      sigma_in[j][m] + sigma_gain (sd[j] - sigma_in[j][m]); with count[m] == 0, sigma_out = sigma_in, unchanged and unclamped
 *  11. lane_sigma[j][s M + m] = sigma_out[j][m] for every s
 * Errors, each with a text of its own that starts with "os2rx_cem_update: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype or nq; nknots, nrobots, nsamples or nelite < 1; nelite
 * above nsamples; more than 65535 knots; nsamples nrobots above 2^31 - 1; shift outside 0..nknots; unknown flag bits; a gain or
 * sigma_gain that is not finite or outside (0, 1]; a sigma_min or sigma_max that is not finite or negative; sigma_min above
 * sigma_max; for an fp32 layout any of the four that is non-zero and outside the normal range of fp32; a null returns_dev,
 * actions_dev, nominal_in_dev, sigma_in_dev, nominal_out_dev, var_out_dev or sigma_out_dev; an actions_dev that is not aligned
 * to a pair of its elements; overlapping nominals; a var_out_dev that overlaps an input; with table_dev, an obs_dim outside
 * 1..OS2R_MAX_OBS.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rx_cem_update(const Os2rControlLayout* layout, int32_t nknots, int64_t nrobots, int32_t nsamples, int32_t nelite,
                              const void* returns_dev, const void* actions_dev, const void* nominal_in_dev, const void* sigma_in_dev,
                              double gain, double sigma_gain, double sigma_min, double sigma_max, int32_t shift, uint32_t flags,
                              void* nominal_out_dev, void* var_out_dev, void* sigma_out_dev, void* applied_dev, void* table_dev,
                              void* lane_sigma_dev, int32_t* elite_dev, void* threshold_dev, int32_t* count_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_CEM_H_ */
