/*
 * os2r_critic.h — C-ABI of libos2r_critic.so, the companion library of libos2r.so for the critic of an actor-critic iteration of
 * many linear-Gaussian policies: a value function V_p(x) = w_p . [x; 1] per policy, linear in the observation like the policy
 * itself, the generalised advantage estimate GAE(lambda) (Schulman et al. 2016) of every step of every lane under it, and the
 * ridge least-squares refit of w_p on the batch.  Both calls work on the device arrays a rollout of policies returned
 * (observations, rewards, done flags, terminal observations, lengths), in the layouts the rollout wrote them: reset ->
 * rollout -> os2rv_gae -> the policy gradient (rewards = adv, done = done, gamma = 0: psi = adv[k][l]) -> os2rv_value_fit is one
 * iteration with no tensor reshuffled in between.
 *
 * Like the other companion headers it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are
 * theirs: every entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed
 * as `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller.  The error text
 * belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 *
 * Common to both entry points.  K = nsteps (1..65535), P = npolicies, S = nsamples, N = S P <= 2^31 - 1, S K <= 2^31 - 1,
 * D = layout->obs_dim (1..OS2R_MAX_OBS): lane s P + p is sample s of policy p.  Every floating-point device array is in
 * layout->dtype (T below).  Of the layout dtype, nq (2..5, as everywhere), device and obs_dim are read; slot_col is not.
 *   obs_dev     [K][N][D], required: the rollout's observations
 *   obs0_dev    [N][D], required: the observation x_k that step k's action saw is obs0[l] for k = 0 and obs[k-1][l] after it
 *   length_dev  int32 [N], nullable (null: K): an entry below 0 counts as 0, one above K as K: len.  Steps k >= len of a lane
 *               are never read into any sum and get 0 in the per-step outputs.  With the lengths of a first-episode rollout
 *               only the first episode counts; without them the whole window counts, across auto-resets
 *   the value weights (value_w_dev, prev_w_dev, w_dev) are [D+1][P], policy index fastest, the bias last, and
 *   val(x; w) = (((w_D + w_0 x_0) + w_1 x_1) + ... + w_{D-1} x_{D-1}), the chain of the rollout's policy
 * Arithmetic (part of the contract): T throughout, every product, sum and difference rounded on its own (no fused
 * multiply-add), every division and square root correctly rounded.  The sign of a zero is not part of the contract.  "Finite"
 * and "> 0" are decided on bit patterns.
 *
 * Out of scope: anything but a linear value function, advantage normalisation, importance ratios and PPO clipping, a weight
 * per sample in the fit, explained-variance outputs, the knot-observation form (a null obs0_dev), fusing the fit into the
 * gradient call.
 */
#ifndef OS2R_CRITIC_H_
#define OS2R_CRITIC_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_CRITIC_ABI_VERSION 1
/* The partial sums every sum over the samples of a policy is defined in (os2rv_value_fit, step 3): the 64 of the
 * policy-gradient library, OS2RG_CHUNKS there, and its kernels. */
#define OS2RV_CHUNKS 64
#define OS2RV_LANE_COUNTS 2 /* the rows of lane_count_dev: len, valid */

OS2R_API int os2rv_abi_version(void);
OS2R_API const char* os2rv_last_error(void); /* of the calling thread's last failed call */

/* Advantages and lambda-returns of every step of every lane in one call (two stream-ordered launches: the values of all K N
 * steps, parallel over (k, lane); then the backward scan of every lane, which reads value_dev as the first launch wrote it).
 * Inputs (read only), beside the common ones:
 *   term_obs_dev  [K][N][D], nullable: the rollout's terminal observations, read where a step was truncated only
 *   reward_dev    [K][N], required
 *   done_dev      uint8 [K][N], required: the step kernels' flags; bit 0 done, bit 1 TimeLimit truncation, bit 2 the
 *                 non-finite guard
 *   value_w_dev   [D+1][P], required
 *   gamma, lambda doubles, finite, in [0, 1], each rounded once to T; c = gamma lambda is formed in T
 * Outputs (every entry of a given output is written on every successful call):
 *   adv_dev       [K][N], required
 *   ret_dev       [K][N], nullable: the lambda-return adv + value, the target of os2rv_value_fit
 *   value_dev     [K][N], required (the second launch reads it): val(x_k) of every counted step
 * For lane l = s P + p with w = value_w[.][p], trace = 0, k walks from len - 1 down to 0:
 *   v = val(x_k);  f = done[k][l]
 *   f & 5 (done or the guard):             nv = 0,                                            cut
 *   else f & 2 (a truncation and no more): nv = term_obs_dev ? val(term_obs[k][l]) : 0,        cut
 *   else:                                  nv = val(obs[k][l]),                               no cut
 *   delta = (r_k + (gamma nv)) - v
 *   trace = cut ? delta : delta + (c trace)
 *   adv[k][l] = trace;  ret[k][l] = trace + v;  value[k][l] = v
 * val(obs[k][l]) of step k and v of step k + 1 are the same chain on the same numbers.  After a done step obs[k] is the
 * post-reset observation that step k + 1 saw, and the cut keeps the episodes apart.  A value that is not finite stays inside
 * its lane.
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Errors, each with a text of its own that starts with "os2rv_gae: ", all found before the first HIP call (a refused call
 * writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; nsteps outside 1..65535; npolicies or
 * nsamples < 1; nsamples npolicies or nsamples nsteps above 2^31 - 1; a gamma or lambda that is not finite or outside [0, 1];
 * a null obs_dev, obs0_dev, reward_dev, done_dev, value_w_dev, adv_dev or value_dev; an output that overlaps an input or
 * another output.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rv_gae(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, const void* obs_dev,
                       const void* obs0_dev, const void* term_obs_dev, const void* reward_dev, const uint8_t* done_dev,
                       const int32_t* length_dev, const void* value_w_dev, double gamma, double lambda, void* adv_dev, void* ret_dev,
                       void* value_dev, void* stream);

/* The ridge least-squares fit of every policy's value weights on the batch in one call (three stream-ordered launches: the
 * moments of every lane; their sums over the samples of every policy; the solve of every policy.  The second reads
 * lane_mom_dev and lane_count_dev as the first wrote them, the third mom_dev as the second wrote it).
 * Inputs (read only), beside the common ones:
 *   target_dev   [K][N], required: the ret of os2rv_gae, or the reward-to-go of the policy-gradient library
 *   prev_w_dev   [D+1][P], nullable: the weights the ridge term pulls towards (null: towards 0)
 *   ridge        a double, finite, >= 0, rounded once to T
 * Outputs (null: not wanted; every entry of a given output is written on every successful call).  E = (D+1)(D+2)/2 + (D+1):
 *   w_dev           [D+1][P], required
 *   lane_mom_dev    [E][N], required: the per-lane sums of step 1.  Entry order: the upper triangle of M row by row -- M[i][j],
 *                   i <= j <= D, at i (D + 1) - i (i - 1) / 2 + (j - i) -- then b[0] .. b[D]
 *   mom_dev         [E][P], required: their sums over the valid lanes of every policy (step 3), in the same order
 *   lane_count_dev  int32 [2][N], required: len and 1 for a valid lane (else 0) of every lane
 *   failed_dev      nullable, int32 [P]: 0, or j + 1 where the factor failed at column j
 *   steps_dev       nullable, int32 [P]: the sum of len over the policy's valid lanes
 *   valid_dev       nullable, int32 [P]: the count of valid lanes
 * Arithmetic, with phi = [x_k; 1] and y = target[k][l]:
 *   1. per lane, every sum starting at 0, k walks from len - 1 down to 0: M[i][j] += phi_i phi_j for i <= j < D (the product
 *      is rounded, then added); M[i][D] += x_i; M[D][D] += 1; b[i] += x_i y for i < D; b[D] += y
 *   2. the lane is valid iff all of its E sums are finite (tested on the bit pattern); lane_mom holds the sums as computed,
 *      valid or not
 *   3. a sum over the samples of policy p runs over its valid lanes only, in OS2RV_CHUNKS = 64 partials: partial c adds the
 *      terms of s = c, c + 64, ... in ascending order onto 0 (an empty partial is 0), and the total is the adjacent-pair tree
 *      ((p0 + p1) + (p2 + p3)) + ... to depth 6: step 5 of the policy-gradient library's header, word for word.  The sums are
 *      mom (of each of the E entries) and the integers steps (of len) and valid
 *   4. per policy, n = D + 1, M and b the sums of step 3: A[i][i] = M[i][i] + ridge, A[i][j] = M[i][j] for i < j;
 *      rhs_i = b_i + (ridge prev_i), or rhs_i = b_i without prev_w_dev.  The lower triangular factor L with L L' = A is built
 *      column by column, j = 0 .. n-1, in the order and with the failure rule of os2ru_ukf_points (os2r_ukf.h):
 *        t = A[j][j] - sum_{l<j} L[j][l] L[j][l]   (j = 0: t = A[0][0]; otherwise the sum is formed first and subtracted once)
 *        if t is not finite or not > 0: failed = j + 1 and the factor stops
 *        L[j][j] = sqrt(t)
 *        for i > j: L[i][j] = (A[j][i] - sum_{l<j} L[i][l] L[j][l]) / L[j][j]   (j = 0: A[0][i] / L[0][0])
 *      then z_i = (rhs_i - sum_{l<i} L[i][l] z_l) / L[i][i] for i = 0 .. n-1, and w_i = (z_i - sum_{l>i} L[l][i] w_l) / L[i][i]
 *      for i = n-1 .. 0.  Every sum of products is ((x_0 y_0 + x_1 y_1) + x_2 y_2) + ... with l ascending, formed first and
 *      subtracted once; an empty sum subtracts nothing.  A policy whose factor failed gets w = prev (0 without prev_w_dev) and
 *      failed = j + 1 of the column that failed; otherwise failed = 0.  A policy without a valid lane has M = 0 and b = 0: it
 *      fails at column 0 under ridge = 0 and gets w close to prev under ridge > 0
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Errors, each with a text of its own that starts with "os2rv_value_fit: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; nsteps outside 1..65535; npolicies or
 * nsamples < 1; nsamples npolicies or nsamples nsteps above 2^31 - 1; a ridge that is not finite or is negative; a null
 * obs_dev, obs0_dev, target_dev, w_dev, lane_mom_dev, mom_dev or lane_count_dev; an output that overlaps an input or another
 * output.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rv_value_fit(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, const void* obs_dev,
                             const void* obs0_dev, const void* target_dev, const int32_t* length_dev, const void* prev_w_dev,
                             double ridge, void* w_dev, void* lane_mom_dev, void* mom_dev, int32_t* lane_count_dev, int32_t* failed_dev,
                             int32_t* steps_dev, int32_t* valid_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_CRITIC_H_ */
