/*
 * os2r_pf.h — C-ABI of libos2r_pf.so, the companion library of libos2r.so for state estimation: the particle-filter update of many
 * robots in one launch -- the weights of every robot's particles against a measurement, the weighted estimate, the effective
 * sample size and, where a robot resamples, the systematic-resampling index that os2r_copy_envs takes.
 *
 * Like os2r_mppi.h it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are the same: every
 * entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed as
 * `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller.  The error text
 * belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 */
#ifndef OS2R_PF_H_
#define OS2R_PF_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_PF_ABI_VERSION 1
#define OS2RP_CHUNKS 8 /* the partial sums every sum over the particles is defined in (step 6) */

OS2R_API int os2rp_abi_version(void);
OS2R_API const char* os2rp_last_error(void); /* of the calling thread's last failed call */

/* The particle-filter update of many independent robots in one launch: the Gaussian log-likelihood of a measurement under every
 * particle's observation, added to the accumulated log-weights; the normalised weights' estimate of the observation and their
 * effective sample size; and for every robot whose effective sample size has fallen below resample_ratio S, or that holds a
 * diverged particle, the ancestor of every lane by systematic resampling -- as the index of os2r_copy_envs from the particle
 * handle into itself, -1 ("keep") in every lane of a robot that does not resample.
 * With M = nrobots, S = nparticles, N = S M, D = layout->obs_dim: lane j = s M + m is particle s of robot m, the environment
 * order of a particle handle forked by os2r_copy_envs with index[j] = j mod M (the order of os2rm_mppi_update).  Every
 * floating-point device array is in layout->dtype.  Of the layout dtype, nq (2..5, as everywhere), device and obs_dim are read;
 * slot_col is not.
 * Inputs (read only):
 *   obs_dev         [N][D]: every particle's observation, as os2r_step, a one-step rollout or os2r_copy_envs returned it
 *   meas_dev        [M][D]: the measurement of every robot
 *   prec_dev        [D]: one inverse variance per observation entry; an entry equal to 0 drops that dimension
 *   logw_in_dev     nullable, [S][M]: the accumulated log-weights; null: all zero
 *   u_dev           nullable, [M]: the systematic-resampling offset of every robot, in [0, 1); null: 0.5 for every robot.  A
 *                   value outside [0, 1), or not finite, is used as 0.5
 *   resample_ratio  finite and >= 0; rounded once to the dtype (a value above the dtype's largest finite number is taken as that
 *                   number)
 * Outputs (each written completely on every call; null: not wanted):
 *   logw_out_dev    [S][M], required; must not overlap logw_in_dev.  Between the passes of the launch it holds the weights
 *   index_dev       [N] int32, required
 *   est_dev         nullable, [M][D]
 *   weights_dev     nullable, [S][M]: the unnormalised weight w of every particle (step 5)
 *   ess_dev         nullable, [M]
 *   count_dev       nullable, [M] int32
 *   resampled_dev   nullable, [M] int32: 1 where the robot resampled, else 0
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Arithmetic (part of the contract): layout->dtype throughout, every product and sum rounded on its own (no fused multiply-add),
 * every division correctly rounded.  The sign of a zero is not part of the contract.  For robot m, with o the observation of
 * particle s (lane s M + m) and y = meas[m]:
 *   1. d2_s = sum over i of ((o_i - y_i) (o_i - y_i)) prec_i, added in ascending i onto 0
 *   2. l_s = logw_in[s][m] - 0.5 d2_s
 *   3. particle s is valid iff l_s is finite (tested on the bit pattern); count[m] is the number of valid particles
 *   4. lmax is the maximum of l_s over the valid particles
 *   5. w_s = exp(l_s - lmax) for a valid particle, with the device library's exp (within a few ulp of the exact value, exactly 1
 *      at the maximum); w_s = 0 exactly for an invalid particle
 *   6. a sum over s is formed in OS2RP_CHUNKS = 8 partials: partial c adds its terms s = c, c + 8, ... in ascending order onto 0
 *      (an empty partial is 0), and the total is ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)).  The sums are wsum of w_s, Q of
 *      the rounded products w_s w_s and E_i of the rounded products w_s o_i, for every i < D (an invalid particle adds 0 to
 *      E_i, whatever its observation holds)
 *   7. ess[m] = (wsum wsum) / Q if count[m] > 0, else 0
 *   8. est[m][i] = E_i / wsum if count[m] > 0, else meas[m][i]
 *   9. resampled[m] = 1 iff count[m] > 0 and (ess[m] < resample_ratio S or count[m] < S), the product rounded once: a robot with
 *      any diverged particle resamples, and resample_ratio = 0 resamples for that reason only
 *  10. not resampled: logw_out[s][m] = l_s - lmax for a valid particle and -infinity (as its bit pattern) for an invalid one, and
 *      index[s M + m] = -1 for every s, the "keep" of os2r_copy_envs.  With count[m] = 0 the robot is lost: logw_out[s][m] = 0
 *      for every s, index -1
 *  11. resampled, systematic resampling: the cumulative weights are the sequential prefix c_0 = w_0, c_s = c_(s-1) + w_s
 *      (ascending, one rounded add each: deliberately not the tree of step 6); step = c_(S-1) / S; for the output slot
 *      n = 0 .. S-1, t_n = (n + u) step (n converted to the dtype, one add, one product), a_n is the smallest s with c_s > t_n
 *      or, if there is none, the largest s with w_s > 0; index[n M + m] = a_n M + m and logw_out[n][m] = 0
 * Errors, each with a text of its own that starts with "os2rp_pf_update: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype or nq; an obs_dim outside 1..OS2R_MAX_OBS; nrobots or
 * nparticles < 1; nparticles nrobots above 2^31 - 1; a resample_ratio that is not finite or is negative; a null obs_dev,
 * meas_dev, prec_dev, logw_out_dev or index_dev; a logw_out_dev that overlaps logw_in_dev.  OS2R_ERR_NO_DEVICE where
 * layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rp_pf_update(const Os2rControlLayout* layout, int64_t nrobots, int32_t nparticles, const void* obs_dev,
                             const void* meas_dev, const void* prec_dev, const void* logw_in_dev, const void* u_dev,
                             double resample_ratio, void* logw_out_dev, int32_t* index_dev, void* est_dev, void* weights_dev,
                             void* ess_dev, int32_t* count_dev, int32_t* resampled_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_PF_H_ */
