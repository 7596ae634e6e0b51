/*
 * os2r_record.h -- C-ABI of libos2r_record.so, the companion of libos2r.so that records the knots of a policy rollout.
 *
 * libos2r.so's dynamic symbol table is the entry points of os2r.h and nothing else, and ABI 6 is closed: this entry point lives
 * in a library of its own, as os2rc_ilqr_backward does (os2r_control.h).  libos2r_record.so is linked from the same objects as
 * libos2r.so and exports the two functions below; it works on the handles libos2r.so creates (os2r_create) -- the two libraries
 * must come from one build -- and a caller that links libos2r.so alone loses nothing.
 */
#ifndef OS2R_RECORD_H_
#define OS2R_RECORD_H_

#include "os2r.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_RECORD_ABI_VERSION 1

/* The same rollout, recording its knots : everything from `nsteps` on
 * is os2r_rollout_policy_scheduled, argument for argument, and `sim` and every output of that entry point are, bit for bit, what it
 * leaves with the same arguments.  With N = num_envs of `sim`, in the same launch:
 *   knots         nullable: another handle.  At the top of env-step k of the call (k = 0 .. nsteps-1), before the action is formed,
 *                 environment e of `sim` -- as it stands then: after the reset, if the previous env-step auto-reset it -- is copied
 *                 to environment (first_knot + k) N + e of `knots`: the arrays `what` selects (OS2R_COPY_STATE, OS2R_COPY_PARAMS),
 *                 bit for bit, exactly the rows os2r_copy_envs(knots, sim, index, what) moves; what stays the destination's is what
 *                 stays there under os2r_copy_envs.  Every other environment of `knots`, its step counter, violation count, mirror
 *                 and buffers are untouched.  `knots` afterwards is what this loop leaves: for each k, os2r_copy_envs(knots, sim,
 *                 index_k, what) with index_k[j] = j - (first_knot + k) N inside the knot's lanes and -1 elsewhere, then one env-step
 *                 of os2r_rollout_policy_scheduled (first_slot + k on the window clock).  `knots` must agree with `sim` in dtype,
 *                 device and robot (os2r_copy_envs' rule) and have at least (first_knot + nsteps) N environments; task, auto_reset
 *                 and solver settings may differ.  After OS2R_COPY_PARAMS from a `sim` with per-environment parameters (or another
 *                 gravity) its kernels read the parameter arrays per lane, as after os2r_copy_envs.  It is the handle
 *                 os2r_linearize takes for the Jacobians of every knot, knot-major.
 *   first_knot    >= 0: lets a window be split as first_slot does: K env-steps equal K1 and K - K1, the second call with
 *                 first_knot + K1 (and first_slot + K1 on the window clock)
 *   knot_obs_dev  nullable, [nsteps][N][D] in the handle's dtype: the observation the policy evaluates at the top of env-step k --
 *                 for equal tasks what os2r_copy_envs(..., obs_dev) reports for that knot --: the obs_dev [L][D] of os2r_lqr_gains
 *                 with L = nsteps N, knot-major
 * At least one of knots and knot_obs_dev is required; what and first_knot are checked only with knots.  One fused launch where
 * os2r_rollout_policy has one; in the launch loop one os2r_copy_envs launch per env-step more (same results).
 * Errors, all OS2R_ERR_INVALID, found before the device is touched (a refused call writes nothing; os2r_last_error(sim) names the
 * cause; for a null sim: os2rr_last_error()): every cause of os2r_rollout_policy_scheduled; knots and knot_obs_dev both null; knots == sim; a dtype, device or model
 * mismatch; what == 0 or an unknown bit; first_knot < 0; knots with fewer than (first_knot + nsteps) N environments.                */
OS2R_API int os2rr_rollout_policy_recorded(Os2rSim* sim, Os2rSim* knots, int32_t first_knot, int32_t what, void* knot_obs_dev,
                                           int nsteps, const void* weights_dev, int32_t period, int32_t first_slot, int32_t flags,
                                           const void* sigma_dev, uint32_t salt, void* return_dev, int32_t* length_dev,
                                           void* obs_dev, void* reward_dev, uint8_t* done_dev, void* term_obs_dev,
                                           uint16_t* reason_dev, void* action_dev, void* noise_dev, void* stream);

/* What the last refused call of this thread without a handle said (a call with a handle writes os2r_last_error(sim)). */
OS2R_API const char* os2rr_last_error(void);
OS2R_API int os2rr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif  /* OS2R_RECORD_H_ */
