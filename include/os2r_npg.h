/*
 * os2r_npg.h — C-ABI of libos2r_npg.so, the companion library of libos2r.so for the natural-gradient step (Kakade 2002) of the
 * linear-Gaussian policy the rollout kernels evaluate: from a plain gradient of the mean weights (and, where wanted, of the log
 * widths) to a step of a stated Kullback-Leibler divergence, for many policies in one call, on the device arrays a noisy
 * rollout returned (observations, applied actions, lengths), in the layouts the rollout wrote them.  The Fisher matrix of the
 * mean weights of row j is sum phi phi' / sigma_j^2 over the steps on which component j was open, phi = [x; 1]; with the widths
 * unchanged the mean divergence of a step Delta is exactly 1/2 Delta' F Delta, so the trust-region step (the step of TRPO,
 * Schulman et al. 2015, without its conjugate gradients: the matrices are 13 x 13 at most) is a closed form.
 *
 * Like the other companion headers it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are
 * theirs: every entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed
 * as `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller.  The error text
 * belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 *
 * Out of scope: MLP policies and scheduled policies, a full Fisher matrix across the two components and the widths, conjugate
 * gradients, a backtracking line search on the surrogate, a kl or a damping per policy, fusing the moments into the gradient
 * call.
 */
#ifndef OS2R_NPG_H_
#define OS2R_NPG_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_NPG_ABI_VERSION 1
#define OS2RN_TANH 1u           /* flags: the rollout squashed with tanh (no action clip binds; action_dev is not read) */
#define OS2RN_SIGMA_PER_LANE 2u /* flags: sigma_dev is [2][N], lane index fastest; else [2] */
/* The partial sums every sum over the samples of a policy is defined in (step 2): the 64 of the score-function library, a
 * partial a lane of a wave. */
#define OS2RN_CHUNKS 64
#define OS2RN_LANE_COUNTS 4 /* the rows of lane_count_dev: len, n_0, n_1, valid */

OS2R_API int os2rn_abi_version(void);
OS2R_API const char* os2rn_last_error(void); /* of the calling thread's last failed call */

/* The natural-gradient step of many linear-Gaussian policies in one call (three stream-ordered launches: the Fisher moments of
 * every lane; their sums over the samples of every policy; the solve and the scaling of every policy.  The second reads
 * lane_mom_dev and lane_count_dev as the first wrote them, the third mom_dev -- and steps_dev and open_dev where given -- as
 * the second wrote them).
 * With K = nsteps (1..65535), P = npolicies, S = nsamples, N = S P <= 2^31 - 1, S K <= 2^31 - 1, D = layout->obs_dim
 * (1..OS2R_MAX_OBS), n = D + 1 and Tri = n (n + 1) / 2: lane s P + p is sample s of policy p.  Every floating-point device array
 * is in layout->dtype (T below).  Of the layout dtype, nq (2..5, as everywhere), device and obs_dim are read; slot_col is not.
 * Inputs (read only):
 *   obs_dev        [K][N][D], required
 *   obs0_dev       [N][D], nullable.  Given: the observation x_k that step k's action saw is obs0 for k = 0 and obs[k-1] after
 *                  it.  Null: x_k = obs[k] (the knot observations of a recorded rollout, which already are what the policy saw)
 *   action_dev     [K][N][2]: the rollout's applied actions; aligned to a pair of its elements.  Required unless OS2RN_TANH, not
 *                  read with it
 *   sigma_dev      [2], or [2][N] with OS2RN_SIGMA_PER_LANE, required: the width the batch was sampled with
 *   length_dev     int32 [N], nullable (null: K): an entry below 0 counts as 0, one above K as K: len.  Steps k >= len of a lane
 *                  are never read into any sum
 *   grad_dev       [2][D+1][P], required: a gradient with respect to the mean weights as the score-function or the
 *                  clipped-surrogate call wrote it -- policy index fastest, row j, column D the bias
 *   lsig_grad_dev  [2][P], nullable: the gradient with respect to log sigma_j
 *   damping, kl    doubles, finite, >= 0, each rounded once to T
 * Outputs (null: not wanted; every entry of a given output is written on every successful call):
 *   step_dev        [2][D+1][P], required: beta d, in the layout of grad_dev: weights + step is what the next rollout takes
 *   dir_dev         nullable, [2][D+1][P]: the natural-gradient direction d itself
 *   lsig_step_dev   [2][P]: beta d_ls, the step of log sigma; required exactly when lsig_grad_dev is given
 *   beta_dev        nullable, [P]
 *   quad_dev        nullable, [P]: q
 *   failed_dev      nullable, int32 [3][P]: for j = 0, 1 the failing column + 1 of the factor of component j, or 0; row 2 is 1
 *                   where q was not finite or not > 0, else 0
 *   steps_dev       nullable, int32 [P]: the sum of len over the policy's valid lanes
 *   open_dev        nullable, int32 [2][P]: the sum of n_j
 *   valid_dev       nullable, int32 [P]: the count of valid lanes
 *   lane_mom_dev    [2 Tri][N], required: the per-lane sums of step 1 -- the upper triangle of F_0 row by row, F[i][m],
 *                   i <= m <= D, at i (D + 1) - i (i - 1) / 2 + (m - i), then that of F_1
 *   mom_dev         [2 Tri][P], required: their sums over the valid lanes of every policy, in the same order
 *   lane_count_dev  int32 [4][N], required: len, n_0, n_1 and 1 for a valid lane (else 0) of every lane
 * Where steps_dev or open_dev is null the third launch forms that integer total itself, a policy's thread adding its S lanes
 * one after the other (an integer sum does not depend on its order): give both where S is large.
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Arithmetic (part of the contract): T throughout, every product, sum, difference and quotient rounded on its own (no fused
 * multiply-add), every division and square root correctly rounded.  The sign of a zero is not part of the contract.  "Finite",
 * "> 0" and |a| < 1 are decided on bit patterns.
 *   1. per lane l = s P + p, every sum starting at 0, k walks from len - 1 down to 0 with phi = [x_k; 1].  For j = 0, 1 a
 *      component is open iff sigma_j > 0 (a NaN sigma is not; with OS2RN_SIGMA_PER_LANE sigma_j is the lane's own) and, without
 *      OS2RN_TANH, |action[k][l][j]| < 1 (a NaN action is not).  Each product x_i x_m, i <= m < D, is rounded once and added to
 *      F_j[i][m] of every open component j; F_j[i][D] += x_i; n_j += 1 (an integer), and F_j[D][D] is n_j converted to T.  After
 *      the walk every one of the Tri sums of a component whose sigma is > 0 is divided once by s2 = sigma_j sigma_j; a
 *      component whose sigma is not > 0 has all sums 0 and n_j = 0.  The lane is valid iff all of its 2 Tri sums, as divided,
 *      are finite; lane_mom holds them, valid or not
 *   2. a sum over the samples of policy p runs over its valid lanes only, in OS2RN_CHUNKS = 64 partials: partial c adds the
 *      terms of s = c, c + 64, ... in ascending order onto 0 (an empty partial is 0), and the total is the adjacent-pair tree
 *      ((p0 + p1) + (p2 + p3)) + ... to depth 6.  The sums are mom (of each of the 2 Tri entries) and the integers steps (of
 *      len), open (of n_j) and valid
 *   3. per policy, c = steps converted to T.  With steps = 0 every d and d_ls is 0, failed[0] = failed[1] = 1 and q = 0.
 *      Otherwise, for j = 0, 1: Fm[i][m] = mom_j[i][m] / c and g_i = grad[j][i][p] / c, entry by entry; A[i][i] = Fm[i][i] +
 *      damping, A[i][m] = Fm[i][m] for i < m.  The lower triangular factor L with L L' = A is built column by column,
 *      m = 0 .. n-1:
 *        t = A[m][m] - sum_{l<m} L[m][l] L[m][l]   (m = 0: t = A[0][0]; otherwise the sum is formed first and subtracted once)
 *        if t is not finite or not > 0: failed[j] = m + 1 and the factor stops
 *        L[m][m] = sqrt(t)
 *        for i > m: L[i][m] = (A[m][i] - sum_{l<m} L[i][l] L[m][l]) / L[m][m]   (m = 0: A[0][i] / L[0][0])
 *      then z_i = (g_i - sum_{l<i} L[i][l] z_l) / L[i][i] for i = 0 .. n-1, and d_i = (z_i - sum_{l>i} L[l][i] d_l) / L[i][i] for
 *      i = n-1 .. 0.  Every sum of products is ((x_0 y_0 + x_1 y_1) + x_2 y_2) + ... with l ascending, formed first and
 *      subtracted once; an empty sum subtracts nothing.  A component whose factor failed gets d_j = 0; otherwise failed[j] = 0.
 *      With lsig_grad_dev: nn = n_j (the total of open) converted to T, den = ((nn + nn) / c) + damping, g_ls = lsig_grad[j][p] / c
 *      and d_ls,j = g_ls / den, or 0 where den is not finite or not > 0.
 *      q = (((g_0[0] d_0[0] + g_0[1] d_0[1]) + ... + g_0[D] d_0[D]) + g_1[0] d_1[0]) + ... + g_1[D] d_1[D], j then i ascending,
 *      each product rounded, and with lsig_grad_dev then + g_ls,0 d_ls,0 and + g_ls,1 d_ls,1.
 *      If q is not finite or not > 0: beta = 0 and failed[2] = 1.  Otherwise failed[2] = 0 and beta = 1 where the kl passed is 0
 *      (the double, before it is rounded), else beta = sqrt((kl + kl) / q).  step[j][i][p] = beta d_j[i], lsig_step[j][p] = beta d_ls,j, dir = d, quad = q.
 * With damping = 0, no lsig_grad_dev, no failure and kl > 0 the mean over the counted steps of the valid lanes of
 * 1/2 sum_j (step_j . phi)^2 / sigma_j^2, taken over the open components, is kl up to rounding.
 * Errors, each with a text of its own that starts with "os2rn_natural_step: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; nsteps outside 1..65535; npolicies or
 * nsamples < 1; nsamples npolicies or nsamples nsteps above 2^31 - 1; unknown flag bits; a damping or kl that is not finite or
 * is negative; a null obs_dev, sigma_dev, grad_dev, step_dev, lane_mom_dev, mom_dev or lane_count_dev; a null action_dev without
 * OS2RN_TANH; lsig_step_dev without lsig_grad_dev, or the reverse; an action_dev that is not aligned to a pair of its elements;
 * an output that overlaps an input or another output.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device,
 * OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rn_natural_step(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, uint32_t flags,
                                const void* obs_dev, const void* obs0_dev, const void* action_dev, const void* sigma_dev,
                                const int32_t* length_dev, const void* grad_dev, const void* lsig_grad_dev, double damping, double kl,
                                void* step_dev, void* dir_dev, void* lsig_step_dev, void* beta_dev, void* quad_dev, int32_t* failed_dev,
                                int32_t* steps_dev, int32_t* open_dev, int32_t* valid_dev, void* lane_mom_dev, void* mom_dev,
                                int32_t* lane_count_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_NPG_H_ */
