/*
 * os2r_pg.h — C-ABI of libos2r_pg.so, the companion library of libos2r.so for the score-function policy gradient (REINFORCE;
 * Williams 1992) of the linear-Gaussian policy the rollout kernels evaluate: the gradient of many policies in one call, on the
 * device arrays a noisy os2r_rollout_policy_noisy returned (observations, done flags, rewards, applied actions, noise, lengths),
 * each read once, in the layouts the rollout wrote them.
 *
 * Like the other companion headers it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are
 * theirs: every entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed
 * as `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller.  The error text
 * belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 *
 * Out of scope: MLP policies, value-function bootstrapping and GAE(lambda), the optimiser step, importance ratios and PPO
 * clipping, natural-gradient and Fisher terms (since built as `libos2r_npg.so`), a weight per policy on the baseline, scheduled
 * policies (the tables of os2r_rollout_policy_scheduled, whose gradient would carry a slot index).
 */
#ifndef OS2R_PG_H_
#define OS2R_PG_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_PG_ABI_VERSION 1
#define OS2RG_TANH 1u           /* flags: the rollout squashed with tanh (no clip binds; action_dev is not read) */
#define OS2RG_SIGMA_PER_LANE 2u /* flags: sigma_dev is [2][N], lane index fastest; else [2] */
/* The partial sums every sum over the samples of a policy is defined in (step 5).  64 and not the eight of the sampling
 * planners' libraries: at one policy and 8 192 samples eight chains of 1 024 dependent additions would be the whole launch, and
 * an xor butterfly across the 64 lanes of a wave gives lane 0 exactly the adjacent-pair tree of 64 partials. */
#define OS2RG_CHUNKS 64

OS2R_API int os2rg_abi_version(void);
OS2R_API const char* os2rg_last_error(void); /* of the calling thread's last failed call */

/* The score-function gradient of many linear-Gaussian policies in one call (two stream-ordered launches): per lane the sums
 * over the steps of its first episode, per policy the sums over its valid lanes.
 * With K = nsteps (1..65535), P = npolicies, S = nsamples, N = S P <= 2^31 - 1, S K <= 2^31 - 1, D = layout->obs_dim
 * (1..OS2R_MAX_OBS): lane s P + p is sample s of policy p, the order copy_envs_from(real, arange(N) % P) forks in.  Every
 * floating-point device array is in layout->dtype (T below).  Of the layout dtype, nq (2..5, as everywhere), device and obs_dim
 * are read; slot_col is not.
 * Inputs (read only):
 *   obs_dev       [K][N][D], required
 *   obs0_dev      [N][D], nullable.  Given: the observation x_k that step k's action saw is obs0 for k = 0 and obs[k-1] after
 *                 it (reset()'s or the previous window's last observation, then the rollout's obs).  Null: x_k = obs[k] (the
 *                 knot observations of a recorded rollout, which already are what the policy saw)
 *   noise_dev     [K][N][2], required: the rollout's eps; aligned to a pair of its elements
 *   action_dev    [K][N][2]: the rollout's applied actions; aligned to a pair of its elements.  Required unless OS2RG_TANH, not
 *                 read with it
 *   sigma_dev     [2], or [2][N] with OS2RG_SIGMA_PER_LANE, required
 *   length_dev    int32 [N], nullable (null: K): the rollout's length under OS2R_POLICY_FIRST_EPISODE.  An entry below 0 counts
 *                 as 0, one above K as K: len.  Steps k >= len of a lane are never read into any sum
 *   the weight, in exactly one of two ways:
 *   adv_dev       [N]: one number per lane (the return minus a batch baseline, say)
 *   reward_dev    [K][N] with done_dev uint8 [K][N] (required with it), gamma (finite, in [0, 1], rounded once to T) and a
 *                 nullable baseline_dev [K][P]: the discounted reward-to-go of every step
 * Outputs (null: not wanted; every entry of a given output is written on every successful call):
 *   grad_dev        [2][D+1][P], required: policy index fastest; row j, column D is the bias.  At S = 1 this is the
 *                   OS2R_POLICY_PER_ENV weight layout
 *   lane_grad_dev   [2][D+1][N], required: the per-lane sums L
 *   lsig_grad_dev   nullable, [2][P]: the gradient with respect to log sigma_j
 *   lane_lsig_dev   [2][N]: the per-lane sums V; required exactly when lsig_grad_dev is given
 *   steps_dev       nullable, int32 [P]
 *   clipped_dev     nullable, int32 [2][P]
 *   valid_dev       nullable, int32 [P]
 *   rtg_dev         nullable, [K][N], only with reward_dev: the reward-to-go G, 0 where k >= len
 *   lane_count_dev  int32 [4][N], required: len, clip_0, clip_1 and 1 for a valid lane (else 0) of every lane.  What the first
 *                   launch knows of a lane and its sums do not say (whether V is finite where lane_lsig_dev is null, how often
 *                   the clip bound): the second launch reads it beside lane_grad_dev
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Arithmetic (part of the contract): T throughout, every product, sum and difference rounded on its own (no fused
 * multiply-add), every division correctly rounded.  The sign of a zero is not part of the contract.  For lane l = s P + p,
 * every sum starting at 0, k walks from len - 1 down to 0:
 *   1. with rewards: G = r_k if done[k][l] != 0, else G = r_k + (gamma G), G = 0 before the first step; psi = G - baseline[k][p],
 *      or psi = G without a baseline.  With adv_dev: psi = adv[l]
 *   2. for j = 0, 1 a component is open iff sigma_j > 0 (a NaN sigma is not) and, without OS2RG_TANH, |action[k][l][j]| < 1 (a
 *      NaN action is not).  Without OS2RG_TANH a component whose action is not below 1 in magnitude adds 1 to the lane's clip_j
 *   3. for an open component: e = eps / sigma_j, c = psi e; L[j][d] += c x_kd for d < D, L[j][D] += c;
 *      V[j] += psi ((eps eps) - 1)
 *   4. the lane is valid iff all of its 2 (D + 1) + 2 sums are finite (tested on the bit pattern); lane_grad and lane_lsig hold
 *      the sums as computed, valid or not
 *   5. a sum over the samples of policy p runs over its valid lanes only, in OS2RG_CHUNKS = 64 partials: partial c adds the
 *      terms of s = c, c + 64, ... in ascending order onto 0 (an empty partial is 0), and the total is the adjacent-pair tree
 *      ((p0 + p1) + (p2 + p3)) + ... to depth 6.  The sums are grad (of L), lsig_grad (of V) and the integers steps (of len),
 *      clipped (of clip_j) and valid (the count of valid lanes)
 * Errors, each with a text of its own that starts with "os2rg_policy_gradient: ", all found before the first HIP call (a
 * refused call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; nsteps outside 1..65535;
 * npolicies or nsamples < 1; nsamples npolicies or nsamples nsteps above 2^31 - 1; unknown flag bits; a gamma that is not finite
 * or outside [0, 1]; a null obs_dev, noise_dev, sigma_dev, grad_dev, lane_grad_dev or lane_count_dev; a null action_dev without
 * OS2RG_TANH; both of adv_dev and reward_dev, or neither; reward_dev without done_dev; baseline_dev or rtg_dev without
 * reward_dev; lsig_grad_dev without lane_lsig_dev, or the reverse; a noise_dev or action_dev that is not aligned to a pair of its
 * elements; an output that overlaps an input or another output.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950
 * device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rg_policy_gradient(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, uint32_t flags,
                                   const void* obs_dev, const void* obs0_dev, const void* noise_dev, const void* action_dev,
                                   const void* sigma_dev, const int32_t* length_dev, const void* adv_dev, const void* reward_dev,
                                   const uint8_t* done_dev, double gamma, const void* baseline_dev, void* grad_dev, void* lane_grad_dev,
                                   void* lsig_grad_dev, void* lane_lsig_dev, int32_t* steps_dev, int32_t* clipped_dev,
                                   int32_t* valid_dev, void* rtg_dev, int32_t* lane_count_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_PG_H_ */
