/*
 * os2r_norm.h — C-ABI of libos2r_norm.so, the companion library of libos2r.so for running observation whitening (z-scores) of
 * the linear policy the rollout kernels evaluate, for many policies at once: the running mean and deviation of every
 * observation component, kept on the device across batches; the fold of a policy given in whitened coordinates into weights on
 * raw observations; and the chain rule back, from a gradient with respect to those weights to one with respect to the policy.
 * The policy is linear, so whitening changes no rollout kernel: theta . [(x - mu) r; 1] equals W . [x; 1] in algebra with
 * W_d = theta_d r_d and b = theta_D - sum_d W_d mu_d, r_d = 1 / the deviation of component d.  This is the observation
 * normalisation of ARS V2 (Mania et al. 2018) and the running standardisation every policy-gradient learner's textbook
 * version has.
 *
 * Like the other companion headers it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are
 * theirs: every entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed
 * as `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller.  The error text
 * belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 *
 * Common to the three entry points.  P = npolicies, D = layout->obs_dim (1..OS2R_MAX_OBS).  Every floating-point device array
 * is in layout->dtype (T below).  Of the layout dtype, nq (2..5, as everywhere), device and obs_dim are read; slot_col is not.
 * The running state of policy p is three arrays: count int64 [P], the observations seen; mean [P][D]; m2 [P][D], the sum of
 * squared deviations from the mean.  A policy with count <= 0 is empty: its mean and m2 are not read.  Where a state is an
 * input its three pointers are all null (every policy is empty) or all given.
 * Arithmetic (part of the contract): T throughout, every product, sum, difference and quotient rounded on its own (no fused
 * multiply-add), every division and square root correctly rounded.  The sign of a zero is not part of the contract.  "Finite"
 * is decided on bit patterns.  An integer "converted to T" is rounded once.
 *
 * Out of scope: clipping of the whitened observation (it is not linear and would need the rollout kernels), a forgetting
 * factor, a full covariance, whitening of rewards or returns, mapping a step (a contravariant vector) back -- the
 * natural-gradient step is invariant under the reparametrisation and needs none --, MLP policies and scheduled policies, a fit
 * of the value function in whitened coordinates, and updating a state in place: an output may not overlap an input, so the
 * caller swaps two buffers.
 */
#ifndef OS2R_NORM_H_
#define OS2R_NORM_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_NORM_ABI_VERSION 1
#define OS2RZ_PER_LANE 1u       /* os2rz_fold: theta and weights hold one set per lane, lane l under the statistics of policy l mod P */
#define OS2RZ_POLICY_FASTEST 2u /* theta, weights and gradients are [rows][D+1][.], the policy or lane index fastest; else [.][rows][D+1] */
/* The partial sums every sum over the samples of a policy is defined in (os2rz_obs_stats, step 3): the 64 of the
 * score-function gradient's library.  Above 64 samples the sum is that library's kernel body, included unedited.  Up to 64 it
 * is not: that body holds the 64 partials of one sum in a thread's registers, the merge needs two sums in one thread, and two of
 * them side by side spill; the same partials and tree are formed as the samples arrive, written once, as the
 * evolution-strategy library did. */
#define OS2RZ_CHUNKS 64
#define OS2RZ_LANE_COUNTS 2 /* the rows of lane_count_dev: len, valid */

OS2R_API int os2rz_abi_version(void);
OS2R_API const char* os2rz_last_error(void); /* of the calling thread's last failed call */

/* One batch of observations merged into the running state of every policy (two stream-ordered launches: per lane and
 * component the two sums over the steps; per policy and component the sums over its valid lanes and the merge, which reads
 * lane_sum_dev and lane_count_dev as the first launch wrote them).
 * With K = nsteps (1..65535), S = nsamples, N = S P <= 2^31 - 1, S K <= 2^31 - 1: lane s P + p is sample s of policy p.
 * flags: no bit is defined, it must be 0.
 * Inputs (read only):
 *   obs_dev       [K][N][D], required: the rollout's observations
 *   obs0_dev      [N][D], nullable.  Given: the observation x_k that step k's action saw is obs0 for k = 0 and obs[k-1] after
 *                 it.  Null: x_k = obs[k]
 *   length_dev    int32 [N], nullable (null: K): an entry below 0 counts as 0, one above K as K: len.  Steps k >= len of a
 *                 lane are never read
 *   count_in_dev, mean_in_dev, m2_in_dev   the state before the batch (all null: empty)
 * Outputs (null: not wanted; every entry of a given output is written on every successful call):
 *   count_out_dev int64 [P], mean_out_dev [P][D], m2_out_dev [P][D], all required: the state after the batch
 *   steps_dev       nullable, int32 [P]: nb, the steps of the policy's valid lanes
 *   valid_dev       nullable, int32 [P]: its valid lanes
 *   lane_sum_dev    [2 D][N], required: scratch, row d the sum A and row D + d the sum B of every lane, valid or not
 *   lane_count_dev  int32 [OS2RZ_LANE_COUNTS][N], required: scratch, len and 1 for a valid lane (else 0)
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Arithmetic:
 *   1. the pivot c[p][d], chosen on the device: mean_in[p][d] where count_in[p] > 0; else x_0 of lane p (sample 0 of the
 *      policy) where that lane's len > 0 and the value is finite, else 0.  This is the shifted-data form: the plain
 *      sum x^2 - (sum x)^2 / n cancels in fp32 as soon as a component's mean is large beside its deviation, which is where
 *      whitening is wanted
 *   2. per lane l = s P + p and component d, both sums starting at 0, k ascending from 0 to len - 1: dk = x_kd - c[p][d],
 *      A = A + dk, B = B + dk dk (the square rounded first).  The lane is valid iff all of its 2 D sums are finite
 *   3. a sum over the samples of policy p runs over its valid lanes only, in OS2RZ_CHUNKS = 64 partials: partial q adds the
 *      terms of s = q, q + 64, ... in ascending order onto 0 (an empty partial is 0), and the total is the adjacent-pair tree
 *      ((p0 + p1) + (p2 + p3)) + ... to depth 6.  The sums are A[d], B[d] and the integers nb (of len) and valid (the count of
 *      valid lanes)
 *   4. the merge, with na = count_in[p] (0 for an empty state) and nb, na + nb each converted to T where T is asked:
 *      nb = 0            the state goes through: count_out = na, mean_out = mean_in, m2_out = m2_in (0, 0, 0 for an empty one)
 *      else              off = A / nb, m2b = B - A off (the product rounded first), 0 where that is below 0
 *        empty state     mean_out = c + off, m2_out = m2b, count_out = nb
 *        else            w = nb / (na + nb), mean_out = mean_in + off w, m2_out = (m2_in + m2b) + (off off) (na w),
 *                        count_out = na + nb (in int64).  off already is the distance between the batch's mean and the
 *                        running one, because the pivot is the running mean (Chan et al. 1979)
 * Errors, each with a text of its own that starts with "os2rz_obs_stats: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; nsteps outside 1..65535; npolicies or
 * nsamples < 1; nsamples npolicies or nsamples nsteps above 2^31 - 1; unknown flag bits; a null obs_dev; a state of which some
 * but not all of count_in_dev, mean_in_dev and m2_in_dev are given; a null count_out_dev, mean_out_dev, m2_out_dev,
 * lane_sum_dev or lane_count_dev; an output that overlaps an input or another output.  OS2R_ERR_NO_DEVICE where layout->device
 * is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rz_obs_stats(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, uint32_t flags,
                             const void* obs_dev, const void* obs0_dev, const int32_t* length_dev, const int64_t* count_in_dev,
                             const void* mean_in_dev, const void* m2_in_dev, int64_t* count_out_dev, void* mean_out_dev, void* m2_out_dev,
                             int32_t* steps_dev, int32_t* valid_dev, void* lane_sum_dev, int32_t* lane_count_dev, void* stream);

/* Common to os2rz_fold and os2rz_unfold: the scale of policy p.  std_floor is a double, finite and > 0, rounded once to T (a
 * value that rounds to 0 in T is refused).  A policy with count < 2 -- an empty state, or a null one -- has r_d = 1 and
 * mu_d = 0, and its sets are copied through unchanged.  Otherwise mu_d = mean[p][d] and
 *   v = m2[p][d] / count (converted to T), sd = sqrt(v), sd = std_floor where sd is below it, r_d = 1 / sd.
 * rows is 2 for a policy (row j is the motor) or 1 for value weights; a set is rows rows of D weights and a bias, [rows][D+1].
 * Without OS2RZ_POLICY_FASTEST an array of Q sets is [Q][rows][D+1], the layout the per-environment policy rollout takes; with
 * it [rows][D+1][Q], the layout of the score-function gradient and of the value weights. */

/* theta in whitened coordinates -> weights on raw observations, in one launch, a thread per (set, row).
 * Q = npolicies sets, set p under the statistics of policy p; with OS2RZ_PER_LANE Q = nlanes (a multiple of P, <= 2^31 - 1)
 * sets, set l under those of policy l mod P.  Without the flag nlanes is not read.
 *   W[j][d] = theta[j][d] r_d for d < D
 *   W[j][D] = theta[j][D] - s, where s = W[j][0] mu_0 and then s = s + W[j][d] mu_d for d = 1 .. D - 1, each product rounded
 * Errors, each with a text of its own that starts with "os2rz_fold: ", all found before the first HIP call (a refused call
 * writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; npolicies < 1 or above 2^31 - 1; rows that
 * is neither 1 nor 2; unknown flag bits; with OS2RZ_PER_LANE an nlanes < 1, above 2^31 - 1 or no multiple of npolicies; a
 * std_floor that is not finite, is not > 0 or rounds to 0 in T; a state given in part; a null theta_dev or weights_dev; an
 * output that overlaps an input.  OS2R_ERR_NO_DEVICE and OS2R_ERR_HIP as above. */
OS2R_API int os2rz_fold(const Os2rControlLayout* layout, int64_t npolicies, int64_t nlanes, int32_t rows, uint32_t flags,
                        const int64_t* count_dev, const void* mean_dev, const void* m2_dev, double std_floor, const void* theta_dev,
                        void* weights_dev, void* stream);

/* A gradient with respect to the folded weights -> the gradient with respect to theta, in one launch, a thread per (policy,
 * row); per policy only (OS2RZ_PER_LANE is refused).  grad_dev is what the score-function and the clipped-surrogate gradient
 * return, with OS2RZ_POLICY_FASTEST as they lay it out.
 *   gtheta[j][d] = (g[j][d] - g[j][D] mu_d) r_d for d < D, the product g[j][D] mu_d rounded first
 *   gtheta[j][D] = g[j][D]
 * Errors, each with a text of its own that starts with "os2rz_unfold: ", all found before the first HIP call (a refused call
 * writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; npolicies < 1 or above 2^31 - 1; rows that
 * is neither 1 nor 2; OS2RZ_PER_LANE or unknown flag bits; a std_floor that is not finite, is not > 0 or rounds to 0 in T; a
 * state given in part; a null grad_dev or grad_theta_dev; an output that overlaps an input.  OS2R_ERR_NO_DEVICE and
 * OS2R_ERR_HIP as above. */
OS2R_API int os2rz_unfold(const Os2rControlLayout* layout, int64_t npolicies, int32_t rows, uint32_t flags, const int64_t* count_dev,
                          const void* mean_dev, const void* m2_dev, double std_floor, const void* grad_dev, void* grad_theta_dev,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_NORM_H_ */
