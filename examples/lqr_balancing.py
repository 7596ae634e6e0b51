#!/usr/bin/env python3
"""Discrete-time LQR about a held posture of Monopod-nonorm-balance-v1, from the simulator's own step Jacobians.

  python examples/lqr_balancing.py [--envs 1024] [--steps 500] [--settle 300] [--riccati-iters 500] [--eps 1e-4]
                                   [--riccati {torch,device}]

  1. every environment runs a simple posture PD on hip and knee (the on-device linear policy of os2r_rollout_policy, written
     onto the raw observation slots) for --settle env-steps: the posture it holds is the linearisation point;
  2. one os2r_linearize launch (HipSim.linearize) returns A = dx'/dx and B = dx'/da of every environment's env-step about
     its own state and the PD's action there -- finite differences of the full step, ground contact included;
  3. the discrete Riccati recursion P <- Q + A'P(A - BK), K = (R + B'PB)^-1 B'PA runs batched in torch, one problem per
     environment;
  4. the gain goes back onto the observation slots as per-environment [2, D+1] weights, a = clip(a0 - K(x - x0)); state
     components the task does not observe (the boom's yaw, the pitch rate) drop out of the law;
     with --riccati device, 3. and 4. are one os2r_lqr_gains launch (HipSim.lqr_gains: every iteration of every environment
     and the weights); the torch recursion then runs only to print the largest difference between the two gains;
  5. from the same start, --steps env-steps run closed-loop on the device under the PD alone and under the LQR law.
Nothing but the printed numbers leaves the device.  The script prints what happened; it claims no control quality: a
quotient across a change of contact mode is a secant, the default eps is not tuned, and the truncated law is not the
optimal one.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gym_os2r_amd as g
from gym_os2r_amd import abi


def state_column_of_slot(cfg_task, nq):
    """For every observation slot the column of x = (q, qd) it shows raw, or -1 (torque slots, normalised slots)."""
    cols = []
    for d in range(cfg_task.obs_dim):
        kind, src = cfg_task.obs_kind[d], cfg_task.obs_src[d]
        if kind in (abi.OBS_POS_RAW, abi.OBS_POS_PERIODIC_RAW):
            cols.append(src)
        elif kind == abi.OBS_VEL_RAW:
            cols.append(nq + src)
        else:
            cols.append(-1)
    return cols


def weights_of_gain(K, a0, obs0, cols):
    """a = a0 - K (x - x0) on the observation slots: [N, 2, D+1] weights with W[:, :, d] = -K[:, :, col(d)] and the bias
    a0 - W.o0 (o0: the observation at the linearisation point)."""
    N, D = obs0.shape
    W = torch.zeros(N, 2, D + 1, dtype=K.dtype, device=K.device)
    for d, c in enumerate(cols):
        if c >= 0:
            W[:, :, d] = -K[:, :, c]
    W[:, :, D] = a0 - torch.einsum("njd,nd->nj", W[:, :, :D], obs0)
    return W.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=500, help="env-steps of each closed loop")
    ap.add_argument("--settle", type=int, default=300, help="env-steps under the PD before linearising")
    ap.add_argument("--riccati-iters", type=int, default=500)
    ap.add_argument("--eps", type=float, default=None, help="finite-difference step (default: HipSim.linearize's)")
    ap.add_argument("--kp", type=float, default=8.0)
    ap.add_argument("--kd", type=float, default=0.15)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--riccati", choices=("torch", "device"), default="torch",
                    help="where the Riccati recursion runs: a torch loop, or one os2r_lqr_gains launch")
    args = ap.parse_args()
    N = args.envs
    env = g.make("Monopod-nonorm-balance-v1", num_envs=N, seed=args.seed)
    env.reset()
    sim = env.sim
    dev, dt, nq, D = sim.device, sim.dtype, sim.nq, sim.D
    n2 = 2 * nq
    cols = state_column_of_slot(sim.cfg.task, nq)
    unobserved = sorted(set(range(n2)) - set(cols))
    ih, ik = env.model["act_dof"]
    print(f"LQR on Monopod-nonorm-balance-v1: {N} environments, nq {nq}, observation slots -> state columns {cols}, "
          f"unobserved columns {unobserved}", flush=True)

    # 1. the posture PD as a linear policy on the observation slots (torque = max_torque * a; 2.5 scales N m to action units)
    q0, _ = sim.get_state()
    obs0 = sim.copy_envs_from(sim, want_obs=True)                    # the observation of the stored state
    K_pd = torch.zeros(N, 2, n2, dtype=dt, device=dev)
    for j, dof in enumerate((ih, ik)):
        K_pd[:, j, dof] = args.kp / 2.5
        K_pd[:, j, nq + dof] = args.kd / 2.5
    W_pd = weights_of_gain(K_pd, torch.zeros(N, 2, dtype=dt, device=dev), obs0, cols)
    sim.rollout_policy(args.settle, W_pd)
    start = sim.checkpoint()

    # 2. Jacobians about the held posture and the PD's action there
    obs_s = sim.copy_envs_from(sim, want_obs=True)
    a_s = (torch.einsum("njd,nd->nj", W_pd[:, :, :D], obs_s) + W_pd[:, :, D]).clamp(-1.0, 1.0)
    _, _, A_lin, B_lin = sim.linearize(a_s, args.eps, want_next=False)
    A, B = A_lin.contiguous(), B_lin.contiguous()
    rho = torch.linalg.eigvals(A).abs().max(dim=1).values
    print(f"linearised {N} env-steps in one launch: spectral radius of A median {float(rho.median()):.4f} max {float(rho.max()):.4f}, "
          f"|B| max {float(B.abs().max()):.3e}", flush=True)

    # 3. Riccati recursion, one problem per environment
    qdiag = torch.zeros(n2, dtype=dt, device=dev)
    for c in range(n2):
        if c not in unobserved:
            qdiag[c] = 1.0 if c < nq else 0.01
    Q = torch.diag(qdiag).expand(N, n2, n2)
    R = 0.1 * torch.eye(2, dtype=dt, device=dev).expand(N, 2, 2)
    P = Q.clone()
    At, Bt = A.transpose(1, 2), B.transpose(1, 2)
    K = torch.zeros(N, 2, n2, dtype=dt, device=dev)
    for _ in range(args.riccati_iters):
        K = torch.linalg.solve(R + Bt @ P @ B, Bt @ P @ A)
        P = Q + At @ P @ (A - B @ K)
        P = 0.5 * (P + P.transpose(1, 2))
    ok = torch.isfinite(K).flatten(1).all(1)
    K = torch.where(ok[:, None, None], K, K_pd)                     # a recursion that blew up falls back to the PD gain
    print(f"Riccati: {args.riccati_iters} iterations, {int(ok.sum())} of {N} gains finite, |K| median {float(K.abs().flatten(1).max(1).values.median()):.3e}",
          flush=True)

    # 4. + 5. both laws from the same start, closed-loop on the device
    if args.riccati == "device":
        # 3. + 4. again, in one launch: Q and R are host values there, the weights come back in the policy's layout
        Kd, _, flags, Wd = sim.lqr_gains(A_lin, B_lin, torch.diag(qdiag).cpu(), 0.1 * torch.eye(2, dtype=torch.float64),
                                         knots=1, sweeps=args.riccati_iters, actions=a_s, obs=obs_s, want_weights=True)
        Kd, refused = Kd[0], flags[0] != 0
        both = ok & ~refused
        diff = float((Kd - K)[both].abs().max()) if bool(both.any()) else float("nan")
        print(f"Riccati on the device: one launch of {args.riccati_iters} sweeps, {int(refused.sum())} of {N} environments refused in "
              f"the last sweep; largest |K_device - K_torch| {diff:.3e} (|K_torch| max {float(K[both].abs().max()) if bool(both.any()) else 0.0:.3e})",
              flush=True)
        W_lqr = torch.where(refused[:, None, None], W_pd, Wd[:, 0]).contiguous()        # a refused problem falls back to the PD
    else:
        W_lqr = weights_of_gain(K, a_s, obs_s, cols)
    results = {}
    for name, W in (("PD only", W_pd), ("LQR", W_lqr)):
        sim.restore(start)
        ret, length, _ = sim.rollout_policy(args.steps, W, first_episode=True)
        results[name] = (ret, length)
        print(f"{name:8s}: return mean {float(ret.mean()):9.2f} min {float(ret.min()):9.2f}; first-episode length mean "
              f"{float(length.float().mean()):7.1f} of {args.steps}, {int((length == args.steps).sum())} of {N} environments never ended",
              flush=True)
    env.close()


if __name__ == "__main__":
    main()
