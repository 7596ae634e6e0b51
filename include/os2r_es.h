/*
 * os2r_es.h — C-ABI of libos2r_es.so, the companion library of libos2r.so for evolution-strategy (parameter-space) search of
 * the linear policy the rollout kernels evaluate: antithetic perturbations of many policies before a rollout, and after it the
 * update of augmented random search (ARS V1-t, Mania et al. 2018) of every policy from one return per lane.  The directions
 * never exist as an array unless asked for: they are a pure function of (seed, population, direction, generation) under the
 * counter RNG of the stepper (Philox4x32-10 and its Box-Muller pair, DESIGN.md "Random streams"), and the update regenerates
 * exactly the bits the perturbation added.
 *
 * Like the other companion headers it needs nothing of a simulator handle but an Os2rControlLayout, and its conventions are
 * theirs: every entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed
 * as `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller.  The error text
 * belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 *
 * Out of scope: MLP policies and scheduled policies, one-sided (non-antithetic) sampling, centred-rank or other fitness
 * shaping, the observation normalisation of ARS V2 (since built as `libos2r_norm.so`), a nu, step_size or top per population,
 * covariance adaptation (CMA-ES) (since built as `libos2r_cma.so`),
 * weight decay and the optimiser itself (grad_dev is there for the caller's own), a shared noise table, and updating theta in
 * place: an output may not overlap an input, so the caller swaps two buffers.
 */
#ifndef OS2R_ES_H_
#define OS2R_ES_H_

#include "os2r_control.h" /* Os2rControlLayout; through it os2r.h: OS2R_API, the dtypes, the status codes, OS2R_MAX_OBS */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_ES_ABI_VERSION 1
/* The stream of the counter RNG the directions are drawn from (streams 1..5 are the stepper's). */
#define OS2RA_STREAM 6
/* The partial sums every sum over the directions of a population is defined in (update, step 3): the 64 of the score-function
 * library, a partial a lane of a wave. */
#define OS2RA_CHUNKS 64
#define OS2RA_MAX_DIRECTIONS 134217727 /* 2^27 - 1: 16 s + 15 is a 32-bit counter word */

OS2R_API int os2ra_abi_version(void);
OS2R_API const char* os2ra_last_error(void); /* of the calling thread's last failed call */

/* Common to both calls.  M = npops populations (policies), S = ndirs directions each (1..OS2RA_MAX_DIRECTIONS), N = 2 S M
 * <= 2^31 - 1 lanes, D = layout->obs_dim (1..OS2R_MAX_OBS), E = 2 (D + 1) entries of one policy: row j (the motor) of D
 * weights and a bias, entry e = j (D + 1) + i.  Lane (h S + s) M + m holds direction s of population m, h = 0 for
 * theta + nu delta and h = 1 for theta - nu delta.  Every floating-point device array is in layout->dtype (T below).  Of the
 * layout dtype, nq (2..5, as everywhere), device and obs_dim are read; slot_col is not.  flags: no bit is defined, it must be 0.
 * The directions: entry e of delta[m][s] is output (e & 1) of the Box-Muller pair of the stepper's counter RNG with the key
 * `seed`, the counter words ((uint32) (pop_offset + m), OS2RA_STREAM, generation, 16 s + (e >> 1)): with (u0, u1) the two
 * 53-bit uniforms of the Philox block, r = sqrt(-2 log(1 - u0)), th = 2 pi u1, output 0 = r cos th, output 1 = r sin th, all in
 * double, and rounded once to T.  pop_offset lets a shard of populations draw what one call over all of them would draw. */

/* The perturbed policies of a generation, in one launch: a thread owns one Philox block of one (m, s) and writes the two
 * adjacent entries of the plus lane and of the minus lane as aligned pairs.
 * Inputs (read only):
 *   theta_dev    [M][E], required
 *   nu           a double, finite, >= 0, rounded once to T
 * Outputs:
 *   weights_dev  [N][E], required: one weight set per lane, what the per-environment policy rollout takes
 *   delta_dev    [S M][E], nullable: the directions themselves, row s M + m
 * Arithmetic (part of the contract): p = nu delta[e], rounded; weights[(s M + m)][e] = theta[m][e] + p and
 * weights[(S M + s M + m)][e] = theta[m][e] - p, each rounded on its own: the product is NOT contracted into the sum or the
 * difference (no fused multiply-add), so both lanes move by the same p.
 * Errors, each with a text of its own that starts with "os2ra_es_perturb: ", all found before the first HIP call (a refused
 * call writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; npops or ndirs < 1; ndirs above
 * OS2RA_MAX_DIRECTIONS; 2 ndirs npops above 2^31 - 1; unknown flag bits; a nu that is not finite or is negative; a null
 * theta_dev or weights_dev; an array that is not aligned to a pair of its elements; an output that overlaps an input or another
 * output.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2ra_es_perturb(const Os2rControlLayout* layout, int64_t npops, int32_t ndirs, uint32_t flags, uint64_t seed,
                              uint32_t pop_offset, uint32_t generation, const void* theta_dev, double nu, void* weights_dev,
                              void* delta_dev, void* stream);

/* The update of every population from the returns of its 2 S lanes (two or three stream-ordered launches: per direction its
 * validity and its score; where top selects, the rank of every direction among those of its population; per (population,
 * Philox block) the sums.  Each reads kept_dev -- and score_dev -- as the one before it wrote them).
 * Inputs (read only):
 *   returns_dev  [N], required: the return of every lane, as the rollout wrote it
 *   theta_dev    [M][E], required
 *   top          int32 >= 0: the directions kept per population; 0 or >= S: all, and no select launch runs
 *   step_size, sigma_floor   doubles, finite, >= 0, each rounded once to T
 *   seed, pop_offset, generation   those of the perturbation whose returns these are
 * Outputs (null: not wanted; every entry of a given output is written on every successful call):
 *   theta_out_dev  [M][E], required
 *   sigma_r_dev    [M], required
 *   count_dev      int32 [M], required: the valid directions
 *   used_dev       int32 [M], required: b', the directions kept
 *   grad_dev       [M][E], nullable: g / (b' sigma_R), the step without its step_size; 0 where count = 0
 *   kept_dev       int32 [S M], required (an output and the scratch the sums read): 1 where direction s of population m, at
 *                  s M + m, is kept, else 0
 *   score_dev      [S M] elements of the size of T, required where 0 < top < S (else not touched, may be null): scratch, the
 *                  order-preserving integer key of every valid direction's score
 * The call does no host synchronisation, no allocation and no write outside these arrays.
 * Arithmetic (part of the contract): T throughout, every product, sum, difference and quotient rounded on its own (no fused
 * multiply-add), the division and the square root correctly rounded.  The sign of a zero is not part of the contract.
 * "Finite" is decided on bit patterns.  With r+ = returns[s M + m] and r- = returns[S M + s M + m]:
 *   1. direction s is valid iff r+ and r- are both finite; count is the number of valid directions of the population.  Its
 *      score is the larger of r+ and r- (-0 and +0 are equal)
 *   2. b' = min(top, count) where 0 < top < S, else count.  Kept are the b' valid directions of the largest score; among equal
 *      scores the lower s goes first.  (A valid direction is kept iff fewer than top valid directions of its population have
 *      a larger score, or an equal score and a lower s.)
 *   3. a sum over the directions of population m runs over its kept directions only, in OS2RA_CHUNKS = 64 partials: partial c
 *      adds the terms of s = c, c + 64, ... in ascending order onto 0 (an empty partial is 0), and the total is the adjacent-pair
 *      tree ((p0 + p1) + (p2 + p3)) + ... to depth 6.  used = b' is the integer sum of kept.
 *      A population with b' = 0 keeps theta (theta_out = theta), sigma_R = 0 and grad = 0.  Otherwise, with n2 = 2 b' converted
 *      to T and nb = b' converted to T:
 *        mean    the sum whose partial adds r+ and then r- of each of its directions (acc = acc + r+; acc = acc + r-), divided by n2
 *        var     the sum whose partial adds d+ d+ and then d- d- with d+ = r+ - mean, d- = r- - mean, each square rounded,
 *                divided by n2
 *        sigma_R = sqrt(var), or sigma_floor where that is larger (with sigma_floor = 0 a population whose kept returns are all
 *                equal divides 0 by 0: grad and theta_out are NaN there)
 *        g[e]    the sum of the terms (r+ - r-) delta[m][s][e], the difference and the product each rounded; delta regenerated
 *                as above, rounded once to T before the product
 *        grad[e] = g[e] / (nb sigma_R), the product nb sigma_R rounded first
 *        theta_out[e] = theta[e] + step_size grad[e], the product rounded first
 * Errors, each with a text of its own that starts with "os2ra_es_update: ", all found before the first HIP call (a refused call
 * writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq or obs_dim; npops or ndirs < 1; ndirs above
 * OS2RA_MAX_DIRECTIONS; 2 ndirs npops above 2^31 - 1; top < 0; unknown flag bits; a step_size or sigma_floor that is not finite
 * or is negative; a null returns_dev, theta_dev, theta_out_dev, sigma_r_dev, count_dev, used_dev or kept_dev; a null score_dev
 * where 0 < top < ndirs; a theta_dev, theta_out_dev or grad_dev that is not aligned to a pair of its elements; an output that
 * overlaps an input or another output.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for
 * a failed HIP call. */
OS2R_API int os2ra_es_update(const Os2rControlLayout* layout, int64_t npops, int32_t ndirs, int32_t top, uint32_t flags, uint64_t seed,
                             uint32_t pop_offset, uint32_t generation, const void* returns_dev, const void* theta_dev, double step_size,
                             double sigma_floor, void* theta_out_dev, void* sigma_r_dev, int32_t* count_dev, int32_t* used_dev,
                             void* grad_dev, int32_t* kept_dev, void* score_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_ES_H_ */
