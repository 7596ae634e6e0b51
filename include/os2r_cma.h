/*
 * os2r_cma.h — C-ABI of libos2r_cma.so, the companion library of libos2r.so for covariance-matrix-adaptation evolution
 * strategies (CMA-ES, Hansen and Ostermeier 2001) of many populations of the linear policy the rollout kernels evaluate: before a
 * rollout the Cholesky factor of every population's covariance and its correlated samples, one weight set per lane; after it,
 * from one return per lane, the rank-mu / rank-one / path update of mean, step size, covariance and both evolution paths.  The
 * step-size path is driven by the weighted sum of the standard normals themselves, which is what the factor's own inverse makes
 * of the weighted step (Cholesky-CMA-ES, Suttorp, Hansen and Igel 2009): no eigendecomposition and no matrix root is formed.  The
 * normals never exist as an array unless asked for: they are a pure function of (seed, population, sample, generation) under the
 * counter RNG of the stepper (Philox4x32-10 and its Box-Muller pair, DESIGN.md "Random streams"), and the update regenerates
 * exactly the bits the sample call used.
 *
 * Like the other companion headers it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are
 * theirs: every entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed
 * as `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller.  The error text
 * belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 *
 * Out of scope: mirrored or antithetic sampling, active (negative-weight) CMA, sep- and LM-CMA, restarts and population-size
 * schedules (IPOP / BIPOP), constants per population, an eigendecomposition or condition-number output, MLP and scheduled
 * policies, cost-valued (minimising) inputs, and in-place state updates: an output may not overlap an input or another output,
 * so the caller swaps two state sets.
 */
#ifndef OS2R_CMA_H_
#define OS2R_CMA_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_CMA_ABI_VERSION 1
/* The stream of the counter RNG the normals are drawn from (1..5 are the stepper's, 6 is the evolution-strategy library's). */
#define OS2RK_STREAM 7
/* The partial sums every sum over the parents of a population is defined in (update, step 3). */
#define OS2RK_CHUNKS 64
#define OS2RK_MAX_SAMPLES 134217727 /* 2^27 - 1: 16 s + 15 is a 32-bit counter word */

/* The scalars of the update, on the host; each is rounded once to T.  gym_os2r_amd.cma.constants() fills it with Hansen's
 * defaults. */
typedef struct Os2rkCmaConstants {
  double a_sigma, b_sigma;      /* p_sigma <- a_sigma p_sigma + b_sigma zw: 1 - c_sigma, sqrt(c_sigma (2 - c_sigma) mu_eff) */
  double hsig_bound;            /* h = (|p_sigma| < hsig_bound) */
  double a_c, b_c;              /* p_c <- a_c p_c + h b_c yw: 1 - c_c, sqrt(c_c (2 - c_c) mu_eff) */
  double k0_moving, k0_stalled; /* the factor on C where h holds (1 - c_1 - c_mu) and where it does not (that + c_1 c_c (2 - c_c)) */
  double c_1, c_mu;             /* the rank-one and rank-mu learning rates */
  double g_sigma;               /* c_sigma / d_sigma */
  double chi;                   /* E |N(0, I)| */
  double sigma_min, sigma_max;  /* the clamp of the new step size */
} Os2rkCmaConstants;

OS2R_API int os2rk_abi_version(void);
OS2R_API const char* os2rk_last_error(void); /* of the calling thread's last failed call */

/* Common to both calls.  M = npops populations, S = nsamples samples each (2..OS2RK_MAX_SAMPLES), N = S M <= 2^31 - 1 lanes,
 * D = layout->obs_dim (1..OS2R_MAX_OBS), E = 2 (D + 1) entries of one policy: row j (the motor) of D weights and a bias, entry
 * e = j (D + 1) + i.  Lane s M + m holds sample s of population m.  Every floating-point device array is in layout->dtype (T
 * below).  Of the layout dtype, nq (2..5, as everywhere), device and obs_dim are read; slot_col is not.  flags: no bit is
 * defined, it must be 0.  The state of population m: mean [M][E], sigma [M], cov [M][E][E] (both triangles stored), p_sigma
 * [M][E], p_c [M][E].
 * The normals: z[m][s][e] is output (e & 1) of the Box-Muller pair of the stepper's counter RNG with the key `seed`, the counter
 * words ((uint32) (pop_offset + m), OS2RK_STREAM, generation, 16 s + (e >> 1)): with (u0, u1) the two 53-bit uniforms of the
 * Philox block, r = sqrt(-2 log(1 - u0)), th = 2 pi u1, output 0 = r cos th, output 1 = r sin th, all in double, and rounded
 * once to T (the float samples are the double ones, rounded).  pop_offset lets a shard of populations draw what one call over
 * all of them would draw.
 * Arithmetic (part of the contract of both calls): T throughout, every product, sum, difference and quotient rounded on its own
 * (NOT contracted: no fused multiply-add), the division and the square root correctly rounded.  "Finite" and "> 0" are decided
 * on bit patterns.  The sign of a zero is not part of the contract. */

/* The factors and the samples of a generation (two stream-ordered launches: a wave per population factors its covariance; then
 * a thread owns one Philox block of one (m, s) and the two entries of the lane's weights it gives).
 * Inputs (read only):
 *   mean_dev     [M][E], required
 *   sigma_dev    [M], required
 *   cov_dev      [M][E][E], required: only the lower triangle (i >= j) is read
 * Outputs (every entry of a given output is written on every successful call):
 *   factor_dev   [M][E][E], required: A with A A' = C, lower triangle, zeros above
 *   failed_dev   int32 [M], required
 *   weights_dev  [N][E], required: one weight set per lane, what the per-environment policy rollout takes
 *   z_dev        [S M][E], nullable: the normals themselves, row s M + m
 *   1. the factor, by columns j ascending.  The diagonal: acc = C[j][j]; for k < j ascending acc = acc - A[j][k] A[j][k]; the
 *      column is refused if acc is not finite or not > 0, then failed[m] = j + 1; else A[j][j] = sqrt(acc).  Below it, for
 *      i > j: acc = C[i][j]; for k < j ascending acc = acc - A[i][k] A[j][k]; A[i][j] = acc / A[j][j].  Where every column
 *      stands, a sigma[m] that is not finite or not > 0 gives failed[m] = E + 1; otherwise failed[m] = 0.  A failed population
 *      gets an all-zero factor.
 *   2. y[e] = the chain acc = A[e][0] z[0]; acc = acc + A[e][j] z[j] for j = 1 .. e
 *   3. weights[s M + m][e] = mean[m][e] + sigma[m] y[e], the product rounded first.  Every lane of a failed population gets
 *      mean[m] (z_dev is written all the same).
 * Errors, each with a text of its own that starts with "os2rk_cma_sample: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; npops < 1; nsamples < 2 or above
 * OS2RK_MAX_SAMPLES; nsamples npops above 2^31 - 1; unknown flag bits; a null mean_dev, sigma_dev, cov_dev, factor_dev,
 * failed_dev or weights_dev; a mean_dev, weights_dev or z_dev that is not aligned to a pair of its elements; an output that
 * overlaps an input or another output.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for
 * a failed HIP call. */
OS2R_API int os2rk_cma_sample(const Os2rControlLayout* layout, int64_t npops, int32_t nsamples, uint32_t flags, uint64_t seed,
                              uint32_t pop_offset, uint32_t generation, const void* mean_dev, const void* sigma_dev,
                              const void* cov_dev, void* factor_dev, int32_t* failed_dev, void* weights_dev, void* z_dev,
                              void* stream);

/* The update of every population from the returns of its S lanes, larger is better (two stream-ordered launches: per lane its
 * rank among the lanes of its population, per population count and status; then per population the sums over its parents and
 * the new state.  The second reads rank_dev and status_dev as the first wrote them).
 * Inputs (read only):
 *   returns_dev  [N], required: the return of every lane, as the rollout wrote it
 *   rankw_dev    [mu] in T, required: the recombination weight of rank r; 1 <= mu <= S
 *   mean_dev, sigma_dev, cov_dev, p_sigma_dev, p_c_dev   the state, required (cov: only the lower triangle is read)
 *   factor_dev, failed_dev   as the sample call wrote them, required
 *   seed, pop_offset, generation   those of the sample call whose returns these are
 *   constants    on the host, required, every field finite
 * Outputs (null: not wanted; every entry of a given output is written on every successful call):
 *   mean_out_dev, sigma_out_dev, cov_out_dev, p_sigma_out_dev, p_c_out_dev   the new state, required
 *   count_dev    int32 [M], required: the valid lanes
 *   status_dev   int32 [M], required
 *   rank_dev     int32 [S M], required (an output and the scratch the sums read): the rank of sample s of population m, at s M + m
 *   yw_dev       [M][E], nullable: the weighted step, (mean_out - mean) / sigma
 *   ps_norm_dev  [M], nullable: |p_sigma_out|
 *   growth_dev   [M], nullable: the factor on sigma before the clamp
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 *   1. a lane is valid iff its return is finite; count is the number of valid lanes of the population.  status is 2 where
 *      failed != 0, else 1 where count < mu, else 0.  Where status != 0 every state output is the input, bit for bit, and
 *      yw = 0, ps_norm = 0, growth = 1.
 *   2. rank(s) of a valid lane: the number of valid lanes of its population with a larger return, or with an equal return (-0
 *      and +0 are equal) and a lower s; of an invalid lane: count plus the number of invalid lanes below s.  Parents are the
 *      lanes with rank < mu, each with w = rankw[rank].
 *   3. a sum over the parents of population m is in OS2RK_CHUNKS = 64 partials: partial c adds the terms of s = c, c + 64, ...
 *      in ascending order onto 0 (an empty partial is 0), and the total is the adjacent-pair tree ((p0 + p1) + (p2 + p3)) + ...
 *      to depth 6.  With z and y regenerated exactly as in the sample call: zw[e] sums w z[e]; yw[e] sums t[e] = w y[e];
 *      R[i][j] (i >= j) sums t[i] y[j].
 *   4. mean_out[e] = mean[e] + sigma yw[e], the product rounded first
 *   5. p_sigma_out[e] = a_sigma p_sigma[e] + b_sigma zw[e] (the factor's own inverse makes zw of yw exactly; no root of C is
 *      formed); nrm = sqrt(sum of p_sigma_out[e]^2), the squares rounded and added in ascending e onto 0; h = (nrm < hsig_bound)
 *   6. p_c_out[e] = a_c p_c[e] + b_c yw[e] where h holds, a_c p_c[e] where it does not
 *   7. for i >= j: cov_out[i][j] = ((k0 C[i][j]) + (c_1 (p_c_out[i] p_c_out[j]))) + (c_mu R[i][j]) with k0 = k0_moving where h
 *      holds and k0_stalled where it does not; cov_out[j][i] is the same bits
 *   8. growth = exp(g_sigma (nrm / chi - 1)); sigma_out = min(max(sigma growth, sigma_min), sigma_max).  exp is the device's,
 *      within 8 ulp of the correctly rounded value; everything else is bit-exact given growth.
 * Errors, each with a text of its own that starts with "os2rk_cma_update: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; npops < 1; nsamples < 2 or above
 * OS2RK_MAX_SAMPLES; nsamples npops above 2^31 - 1; mu < 1 or above nsamples; unknown flag bits; null constants or a field of
 * it that is not finite; a null required pointer; a mean_dev, mean_out_dev or yw_dev that is not aligned to a pair of its
 * elements; an output that overlaps an input or another output.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950
 * device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rk_cma_update(const Os2rControlLayout* layout, int64_t npops, int32_t nsamples, int32_t mu, uint32_t flags,
                              uint64_t seed, uint32_t pop_offset, uint32_t generation, const void* returns_dev, const void* rankw_dev,
                              const void* mean_dev, const void* sigma_dev, const void* cov_dev, const void* p_sigma_dev,
                              const void* p_c_dev, const void* factor_dev, const int32_t* failed_dev, const Os2rkCmaConstants* constants,
                              void* mean_out_dev, void* sigma_out_dev, void* cov_out_dev, void* p_sigma_out_dev, void* p_c_out_dev,
                              int32_t* count_dev, int32_t* status_dev, int32_t* rank_dev, void* yw_dev, void* ps_norm_dev,
                              void* growth_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_CMA_H_ */
