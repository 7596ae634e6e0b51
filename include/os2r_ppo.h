/*
 * os2r_ppo.h — C-ABI of libos2r_ppo.so, the companion library of libos2r.so for the clipped-surrogate gradient (PPO; Schulman et
 * al. 2017) of the linear-Gaussian policy the rollout kernels evaluate: the gradient of min(rho psi, clip(rho, 1 - c, 1 + c) psi)
 * of many policies in one call, evaluated at new weights on a stored batch -- the device arrays a noisy
 * os2r_rollout_policy_noisy returned (observations, applied actions, noise, lengths) and the advantages of every step, each read
 * once, in the layouts they were written in.  It is what lets one batch pay for several updates: the first epoch is the
 * score-function gradient bit for bit, every later one carries the importance ratio rho and PPO's clip.
 *
 * Like the other companion headers it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are
 * theirs: every entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed
 * as `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller.  The error text
 * belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 *
 * Out of scope: MLP policies, scheduled policies, the optimiser step and the entropy bonus (one torch line each), advantage
 * normalisation inside the call, a value-loss clip, minibatching within a policy's lanes, the density of a component on which
 * the action clip bound (it is left out of the ratio just as the score-function gradient leaves it out of the score),
 * natural-gradient and Fisher terms (since built as `libos2r_npg.so`), a fused advantage + gradient launch.
 */
#ifndef OS2R_PPO_H_
#define OS2R_PPO_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_PPO_ABI_VERSION 1
#define OS2RO_TANH 1u           /* flags: the rollout squashed with tanh (no action clip binds; action_dev is not read) */
#define OS2RO_SIGMA_PER_LANE 2u /* flags: sigma_dev is [2][N], lane index fastest; else [2] */
/* The partial sums every sum over the samples of a policy is defined in (step 16): the 64 of the score-function library, a
 * partial a lane of a wave. */
#define OS2RO_CHUNKS 64
#define OS2RO_LANE_COUNTS 5 /* the rows of lane_count_dev: len, clip_0, clip_1, gated, valid */
#define OS2RO_STATS 3       /* the rows of stat_dev and lane_stat_dev: surr, dev, logr */

OS2R_API int os2ro_abi_version(void);
OS2R_API const char* os2ro_last_error(void); /* of the calling thread's last failed call */

/* The gradient of the clipped surrogate of many linear-Gaussian policies in one call (two stream-ordered launches): per lane the
 * sums over the steps of its first episode, per policy the sums over its valid lanes.
 * With K = nsteps (1..65535), P = npolicies, S = nsamples, N = S P <= 2^31 - 1, S K <= 2^31 - 1, D = layout->obs_dim
 * (1..OS2R_MAX_OBS): lane s P + p is sample s of policy p, the order copy_envs_from(real, arange(N) % P) forks in.  Every
 * floating-point device array is in layout->dtype (T below).  Of the layout dtype, nq (2..5, as everywhere), device and obs_dim
 * are read; slot_col is not.
 * Inputs (read only):
 *   obs_dev         [K][N][D], required
 *   obs0_dev        [N][D], nullable.  Given: the observation x_k that step k's action saw is obs0 for k = 0 and obs[k-1] after
 *                   it (reset()'s or the previous window's last observation, then the rollout's obs).  Null: x_k = obs[k] (the
 *                   knot observations of a recorded rollout, which already are what the policy saw)
 *   noise_dev       [K][N][2], required: the rollout's eps; aligned to a pair of its elements
 *   action_dev      [K][N][2]: the rollout's applied actions; aligned to a pair of its elements.  Required unless OS2RO_TANH, not
 *                   read with it
 *   sigma_dev       [2], or [2][N] with OS2RO_SIGMA_PER_LANE, required: the width the batch was sampled with
 *   sigma_new_dev   [2][P], nullable: the width of the policy being evaluated.  Null: it is the behaviour width
 *   weight_dev      [2][D+1][P], required: the weights being evaluated; policy index fastest, column D is the bias (the layout
 *                   of grad_dev)
 *   weight_old_dev  [2][D+1][P], required: the weights the batch was sampled with
 *   length_dev      int32 [N], nullable (null: K): the rollout's length under OS2R_POLICY_FIRST_EPISODE.  An entry below 0 counts
 *                   as 0, one above K as K: len.  Steps k >= len of a lane are never read into any sum
 *   adv_dev         [K][N], required: the weight of every step (the advantages of the critic's library, normalised or not)
 *   clip            finite and in (0, 1).  The host forms lo = 1 - clip and hi = 1 + clip in double and rounds each once to T
 * Outputs (null: not wanted; every entry of a given output is written on every successful call):
 *   grad_dev        [2][D+1][P], required: the gradient of the clipped surrogate with respect to weight_dev
 *   lane_grad_dev   [2][D+1][N], required: the per-lane sums L
 *   lsig_grad_dev   nullable, [2][P]: the gradient with respect to the log of the evaluated width
 *   lane_lsig_dev   [2][N]: the per-lane sums V; required exactly when lsig_grad_dev is given
 *   stat_dev        nullable, [3][P]: the sums of surr, dev and logr
 *   lane_stat_dev   [3][N], required: the lane's sums surr (the clipped surrogate itself), dev (of rho - 1) and logr (of log rho
 *                   before the widths' factor, h below).  Where the widths are unchanged (dev - logr) / steps is the k3 estimate
 *                   of the KL divergence between the two policies
 *   steps_dev       nullable, int32 [P]
 *   clipped_dev     nullable, int32 [2][P]: how often the action clip bound
 *   gated_dev       nullable, int32 [P]: how often the ratio's clip was active (the step adds no gradient)
 *   valid_dev       nullable, int32 [P]
 *   ratio_dev       nullable, [K][N]: rho of every counted step, 0 where k >= len
 *   lane_count_dev  int32 [5][N], required: len, clip_0, clip_1, gated and 1 for a valid lane (else 0) of every lane.  The second
 *                   launch reads it beside lane_grad_dev, lane_lsig_dev and lane_stat_dev
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Arithmetic (part of the contract): T throughout, every product, sum, difference and division rounded on its own (no fused
 * multiply-add), every division correctly rounded.  The sign of a zero is not part of the contract.  Positivity, |a| < 1 and
 * finiteness are tested on bit patterns.  Once per lane l = s P + p: dW[j][d] = weight[j][d][p] - weight_old[j][d][p] for
 * d = 0..D; r_j = sigma_j / sigma_new[j][p] and snew_j = sigma_new[j][p], or r_j = 1 and snew_j = sigma_j with sigma_new_dev
 * null; component j is enabled iff sigma_j > 0 and snew_j > 0 (a NaN is not positive).  Then, every sum starting at 0, k walks
 * from len - 1 down to 0:
 *   1.  psi = adv[k][l]; x_k as obs0_dev says
 *   2.  for j = 0, 1 a component is open iff it is enabled and, without OS2RO_TANH, |action[k][l][j]| < 1 (a NaN action is not).
 *       Without OS2RO_TANH a component whose action is not below 1 in magnitude adds 1 to the lane's clip_j, whatever the widths
 *   3.  the mean shift dmu_j = ((q_0 + q_1) + (q_2 + q_3)) + dW[j][D], where q_h is the sum, onto 0 and in ascending d, of
 *       dW[j][d] x_kd over d = 3h, 3h + 1, 3h + 2 with d < D
 *   4.  for an open j: z_j = (eps_j - dmu_j / sigma_j) r_j and t_j = (eps_j eps_j) - (z_j z_j)
 *   5.  for a component that is not open t_j = 0
 *   6.  h = 0.5 (t_0 + t_1)
 *   7.  rho = exp(h) (r'_0 r'_1), r'_j = r_j if j is open, else 1
 *   8.  exp is the device's: within 8 ulp of the correctly rounded value, exp(0) = 1 exactly
 *   9.  ratio[k][l] = rho
 *   10. the gate is closed iff (psi > 0 and rho > hi) or (psi < 0 and rho < lo); a NaN closes nothing.  A closed gate adds 1
 *       to the lane's gated
 *   11. surr adds psi hi where the gate is closed with psi > 0, psi lo where it is closed with psi < 0, rho psi where it is open
 *   12. dev adds rho - 1
 *   13. logr adds h
 *   14. with the gate open, w = psi rho and for every open j: e = z_j / snew_j, c = w e; L[j][d] += c x_kd for d < D,
 *       L[j][D] += c; V[j] += w ((z_j z_j) - 1)
 *   15. the lane is valid iff all of its 2 (D + 1) + 2 + 3 sums are finite; lane_grad, lane_lsig and lane_stat hold the sums as
 *       computed, valid or not
 *   16. a sum over the samples of policy p runs over its valid lanes only, in OS2RO_CHUNKS = 64 partials: partial c adds the
 *       terms of s = c, c + 64, ... in ascending order onto 0 (an empty partial is 0), and the total is the adjacent-pair tree
 *       ((p0 + p1) + (p2 + p3)) + ... to depth 6
 *   17. the sums are grad (of L), lsig_grad (of V), stat (of surr, dev and logr) and the integers steps (of len), clipped (of
 *       clip_j), gated and valid (the count of valid lanes)
 * The gate of step 10 is the gradient of min(rho psi, clip(rho, lo, hi) psi): that of rho psi where the minimum is the unclipped
 * term, none where the clip is active.  rho is the likelihood ratio of the pre-squash sample u = mu_old + sigma eps over the open
 * components, written with eps and the weight difference: with weight == weight_old element for element and sigma_new_dev null
 * every z_j is eps_j, every rho is 1, no gate closes, and grad, lane_grad, lsig_grad, lane_lsig, steps, clipped and valid are bit
 * for bit those of the score-function gradient weighted with adv.
 * Errors, each with a text of its own that starts with "os2ro_ppo_gradient: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; nsteps outside 1..65535; npolicies or
 * nsamples < 1; nsamples npolicies or nsamples nsteps above 2^31 - 1; unknown flag bits; a clip that is not finite or outside
 * (0, 1); a null obs_dev, noise_dev, sigma_dev, weight_dev, weight_old_dev, adv_dev, grad_dev, lane_grad_dev, lane_stat_dev or
 * lane_count_dev; a null action_dev without OS2RO_TANH; lsig_grad_dev without lane_lsig_dev, or the reverse; a noise_dev or
 * action_dev that is not aligned to a pair of its elements; an output that overlaps an input or another output.
 * OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2ro_ppo_gradient(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, uint32_t flags,
                                const void* obs_dev, const void* obs0_dev, const void* noise_dev, const void* action_dev,
                                const void* sigma_dev, const void* sigma_new_dev, const void* weight_dev, const void* weight_old_dev,
                                const int32_t* length_dev, const void* adv_dev, double clip, void* grad_dev, void* lane_grad_dev,
                                void* lsig_grad_dev, void* lane_lsig_dev, void* stat_dev, void* lane_stat_dev, int32_t* steps_dev,
                                int32_t* clipped_dev, int32_t* gated_dev, int32_t* valid_dev, void* ratio_dev, int32_t* lane_count_dev,
                                void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_PPO_H_ */
