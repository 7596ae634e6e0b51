/*
 * os2r_control.h — C-ABI of libos2r_control.so, the companion library of libos2r.so for trajectory optimisation on the
 * device arrays that os2r_linearize writes and os2r_rollout_policy_scheduled reads.
 *
 * It holds what needs nothing of a simulator handle but a dtype, a chain length, a device ordinal and an observation layout:
 * those four travel in an Os2rControlLayout, and no Os2rSim appears in a signature.  The conventions are those of os2r.h:
 * every entry point returns an int status (OS2R_OK = 0), never throws, and is stream-ordered on the hipStream_t passed as
 * `void* stream` (NULL = the default stream); all `*_dev` pointers are device pointers owned by the caller, all `*_host`
 * pointers host memory that is read before the call returns.  The error text belongs to the calling thread.
 *
 * Plain C: no torch / pybind / HIP types appear in any signature.
 */
#ifndef OS2R_CONTROL_H_
#define OS2R_CONTROL_H_

#include "os2r.h" /* OS2R_API, OS2R_F32 / OS2R_F64, OS2R_MAX_OBS, OS2R_MAX_DOF, the status codes */

#ifdef __cplusplus
extern "C" {
#endif

#define OS2R_CONTROL_ABI_VERSION 1
#define OS2RC_MAX_ALPHAS 16 /* line-search candidates of one os2rc_ilqr_backward call */

typedef struct Os2rControlLayout {
  int32_t dtype;                  /* OS2R_F32 / OS2R_F64 */
  int32_t nq;                     /* 2..5; n = 2 nq */
  int32_t device;                 /* HIP device ordinal */
  int32_t obs_dim;                /* D; read only when a weight table is asked for (then 1..OS2R_MAX_OBS) */
  int32_t slot_col[OS2R_MAX_OBS]; /* state column a raw observation slot shows (os2r_lqr_gains, step 6), -1: none */
} Os2rControlLayout;

OS2R_API int os2rc_abi_version(void);
OS2R_API const char* os2rc_last_error(void); /* of the calling thread's last failed call */

/* The backward pass of iLQR for many independent trajectories in one launch: os2r_lqr_gains (one sweep) with its affine terms
 * -- cost gradients, the value gradient, the feed-forward step --, a control-space regularisation mu, the two numbers per knot
 * a line search is judged by, and one weight table for a batch of line-search candidates.
 * With K = nknots, M = ntraj, L = K M, n = 2 layout->nq, lane of (knot k, trajectory m) = k M + m; every device array in
 * layout->dtype, the trajectory index fastest, exactly as in os2r_lqr_gains:
 *   a_dev          [n][n][L], b_dev [n][2][L]: os2r_linearize's outputs of a handle whose environments are ordered knot-major
 *   lx_dev         nullable, [n][L]: the cost gradient with respect to the state at each knot; NULL: zeros
 *   lu_dev         nullable, [2][L]: ... with respect to the action; NULL: zeros
 *   q_host         [n][n] row-major doubles, r_host [2][2]: the cost Hessians, as in os2r_lqr_gains: finite, exactly symmetric,
 *                  rounded once to the dtype, passed as kernel arguments
 *   mu             control-space regularisation, finite and >= 0, rounded once
 *   pmat_final_dev nullable, [n][n][M]: the value Hessian behind the last knot, upper triangle (i <= j) read; NULL: Q
 *   pvec_final_dev nullable, [n][M]: the value gradient behind the last knot; NULL: zeros
 *   gain_dev       nullable, [K][2][n][M]: K_k
 *   ff_dev         nullable, [K][2][M]: the feed-forward step k_k
 *   pmat_out_dev   nullable, [n][n][M]: P after knot 0, both triangles; may alias pmat_final_dev
 *   pvec_out_dev   nullable, [n][M]: p after knot 0; may alias pvec_final_dev
 *   flag_dev       nullable, [K][M] uint8: 1 where the knot's 2 x 2 system was refused (below), else 0
 *   dv_dev         nullable, [K][2][M]: the knot's two terms of the expected cost change (step 9)
 *   weights_dev    nullable, [K][2][D+1][nalpha M]: the OS2R_POLICY_PER_ENV table of os2r_rollout_policy_scheduled with
 *                  period = K for a handle of nalpha M environments, environment i M + m being trajectory m under step size
 *                  alpha_host[i]; needs actions_dev [L][2] (the array given to os2r_linearize; clamped to [-1, 1] as there),
 *                  obs_dev [L][D] (the observation at each knot) and alpha_host [nalpha], finite, 1 <= nalpha <= OS2RC_MAX_ALPHAS
 * At least one of gain_dev, ff_dev, pmat_out_dev, pvec_out_dev, dv_dev, weights_dev is required.  The call does no host
 * synchronisation, no allocation and no write outside the outputs.
 * Arithmetic (part of the contract): layout->dtype throughout, every product rounded on its own (no fused multiply-add), every
 * sum of products sum_l x_l y_l evaluated as ((x_0 y_0 + x_1 y_1) + x_2 y_2) + ... with l ascending.  Per knot, from k = K-1 down
 * to 0, with P the symmetric value Hessian, p the value gradient, A = A_k, B = B_k, lx, lu:
 *   1. PB, S00, S01, S11 as in os2r_lqr_gains step 1 (S is unregularised);  T00 = S00 + mu, T11 = S11 + mu, T01 = S01; with
 *      mu == 0, T is S itself
 *   2. det = T00 T11 - T01 T01;  ok = T00 > 0 and det > 0 and det finite
 *   3. PA, G as in os2r_lqr_gains step 3
 *   4. K[0][j] = (T11 G[0][j] - T01 G[1][j]) / det,  K[1][j] = (T00 G[1][j] - T01 G[0][j]) / det
 *   5. Qx[j] = lx[j] + sum_l A[l][j] p[l];  Qu[c] = lu[c] + sum_l B[l][c] p[l]
 *   6. k0 = -((T11 Qu0 - T01 Qu1) / det),  k1 = -((T00 Qu1 - T01 Qu0) / det), the minus flipping the sign bit; a knot that is
 *      not ok gets K = 0, k = 0 and flag 1, and the recursion goes on with those values
 *   7. for i <= j: P'[i][j] = ((Q[i][j] + sum_l A[l][i] PA[l][j]) - (G[0][i] K[0][j] + G[1][i] K[1][j]))
 *                             - mu (K[0][i] K[0][j] + K[1][i] K[1][j]),  the last term skipped when mu == 0;  P'[j][i] = P'[i][j]
 *   8. p'[j] = (Qx[j] + (G[0][j] k0 + G[1][j] k1)) + mu (K[0][j] k0 + K[1][j] k1),  the last term skipped when mu == 0
 *   9. dv[k][0] = k0 Qu0 + k1 Qu1;  dv[k][1] = 0.5 (((S00 k0) k0 + (S11 k1) k1) + 2 ((S01 k0) k1)): the model of the cost change
 *      under step size alpha is alpha sum_k dv[k][0] + alpha^2 sum_k dv[k][1]; the caller sums over k
 *  10. weights: W[k][j][d] as in os2r_lqr_gains step 6, the same for every alpha;
 *      W[k][j][D][i M + m] = (a0_j + alpha_i k_j) - acc, acc being step 6's sum, alpha_i rounded once, the product rounded on
 *      its own
 * Steps 7 and 8 are the regularised updates of Tassa, Erez and Todorov (2012) written out with K = T^-1 G, k = -T^-1 Qu and
 * S = T - mu I.  The sign of a zero is not part of the contract.  With mu = 0, NULL gradients and a NULL pvec_final_dev the gains,
 * pmat_out and flags are those of os2r_lqr_gains(sweeps = 1) bit for bit, and with alpha = 0 so is the weight table.
 * Errors, each with a text of its own that names os2rc_ilqr_backward, all found before the device is touched (a refused call
 * writes nothing): OS2R_ERR_INVALID for a null layout; a bad dtype, nq, obs_dim or slot_col entry (outside -1..n-1); nknots or
 * ntraj < 1; a null a_dev, b_dev, q_host or r_host; a Q or R that is not finite or not symmetric; a mu that is not finite or is
 * negative; all outputs null; weights_dev without actions_dev, obs_dev or alpha_host; nalpha out of range or an alpha that is
 * not finite.  OS2R_ERR_NO_DEVICE where layout->device is no visible gfx950 device, OS2R_ERR_HIP for a failed HIP call. */
OS2R_API int os2rc_ilqr_backward(const Os2rControlLayout* layout, int32_t nknots, int64_t ntraj,
                                 const void* a_dev, const void* b_dev, const void* lx_dev, const void* lu_dev,
                                 const double* q_host, const double* r_host, double mu,
                                 const void* pmat_final_dev, const void* pvec_final_dev,
                                 void* gain_dev, void* ff_dev, void* pmat_out_dev, void* pvec_out_dev, uint8_t* flag_dev, void* dv_dev,
                                 const void* actions_dev, const void* obs_dev, const double* alpha_host, int32_t nalpha, void* weights_dev,
                                 void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OS2R_CONTROL_H_ */
