#!/usr/bin/env python3
"""Time-varying LQR tracking of a recorded trajectory of Monopod-nonorm-balance-v1, gains from the simulator's own Jacobians.

  python examples/tvlqr_tracking.py [--envs 1024] [--steps 100] [--settle 300] [--pulse 0.4] [--perturb 0.02] [--eps 1e-4]
                                    [--riccati {torch,device}]

  1. one environment runs the posture PD of lqr_balancing.py plus a hip-torque pulse for K = --steps env-steps: the nominal
     trajectory x_k, a_k (a_k the applied, clipped action);
  2. before each of those env-steps the state of knot k is forked into lane k of a K-lane handle (copy_envs_from: one launch);
  3. one os2r_linearize launch (HipSim.linearize) on that handle returns A_k = dx'/dx and B_k = dx'/da of every knot;
  4. the backward Riccati recursion K_k = (R + B_k'P B_k)^-1 B_k'P A_k, P <- Q + A_k'P(A_k - B_k K_k) runs in torch;
  5. the law a = a_k - K_k (x - x_k) goes onto the observation slots as a [K, 2, D+1] table of weights, one set per knot, and
     --envs copies of knot 0, each perturbed, track the nominal in ONE launch (HipSim.rollout_schedule, window clock) -- against
     the open-loop replay of the nominal actions from the same starts (HipSim.rollout);
  6. both deviations from the nominal observations are printed.
With --riccati device, 4. and the table of 5. are one os2r_lqr_gains launch (HipSim.lqr_gains) on the linearize output as it
is; the torch recursion then runs only to print the largest difference between the two sets of gains.
Nothing but the printed numbers leaves the device.  The script prints what happened; it claims no control quality: a quotient
across a change of contact mode is a secant, the default eps is not tuned, state components the task does not observe drop out
of the law, and the actions saturate.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gym_os2r_amd as g
from lqr_balancing import state_column_of_slot, weights_of_gain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024, help="perturbed starts that track the nominal")
    ap.add_argument("--steps", type=int, default=100, help="K: env-steps of the nominal trajectory")
    ap.add_argument("--settle", type=int, default=300, help="env-steps under the PD before the nominal starts")
    ap.add_argument("--pulse", type=float, default=0.4, help="hip action added over the first third of the nominal")
    ap.add_argument("--perturb", type=float, default=0.02, help="standard deviation of the start perturbation [rad, rad/s]")
    ap.add_argument("--eps", type=float, default=None, help="finite-difference step (default: HipSim.linearize's)")
    ap.add_argument("--kp", type=float, default=8.0)
    ap.add_argument("--kd", type=float, default=0.15)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--riccati", choices=("torch", "device"), default="torch",
                    help="where the Riccati recursion runs: a torch loop, or one os2r_lqr_gains launch")
    args = ap.parse_args()
    N, K = args.envs, args.steps
    # one task, three handles: the nominal (1 environment), the knots (K lanes), the trackers (N environments); no TimeLimit
    nom_env, knot_env, trk_env = (g.make("Monopod-nonorm-balance-v1", num_envs=n, seed=args.seed) for n in (1, K, N))
    for e in (nom_env, knot_env, trk_env):
        e.reset()
    nom, knots, trk = nom_env.sim, knot_env.sim, trk_env.sim
    dev, dt, nq, D = nom.device, nom.dtype, nom.nq, nom.D
    n2 = 2 * nq
    cols = state_column_of_slot(nom.cfg.task, nq)
    unobserved = sorted(set(range(n2)) - set(cols))
    ih, ik = nom_env.model["act_dof"]
    print(f"TVLQR on Monopod-nonorm-balance-v1: nominal of {K} env-steps, {N} trackers, nq {nq}, unobserved state columns {unobserved}",
          flush=True)

    # 1. + 2. the nominal under the posture PD (settled first) plus a hip pulse; knot k forked into lane k before env-step k
    obs0 = nom.copy_envs_from(nom, want_obs=True)
    K_pd = torch.zeros(1, 2, n2, dtype=dt, device=dev)
    for j, dof in enumerate((ih, ik)):
        K_pd[:, j, dof] = args.kp / 2.5
        K_pd[:, j, nq + dof] = args.kd / 2.5
    W_pd = weights_of_gain(K_pd, torch.zeros(1, 2, dtype=dt, device=dev), obs0, cols)
    nom.rollout_policy(args.settle, W_pd)
    obs = nom.copy_envs_from(nom, want_obs=True)
    lanes = torch.arange(K, dtype=torch.int32, device=dev)
    a_nom, o_nom, ended = [], [], 0
    for k in range(K):
        knots.copy_envs_from(nom, torch.where(lanes == k, 0, -1).to(torch.int32))     # (a negative entry keeps the lane)
        a = torch.einsum("njd,nd->nj", W_pd[:, :, :D], obs) + W_pd[:, :, D]
        if k < K // 3:
            a[:, 0] += args.pulse
        a = a.clamp(-1.0, 1.0)
        obs, _, done, _ = nom.step(a, want_terminal=False)
        ended += int(done[0] != 0)
        a_nom.append(a[0])
        o_nom.append(obs[0])
    a_nom, o_nom = torch.stack(a_nom), torch.stack(o_nom)                             # [K, 2], [K, D]
    print(f"nominal recorded: |a| max {float(a_nom.abs().max()):.3f}, {ended} episode ends inside it", flush=True)

    # 3. every knot's Jacobians in one launch
    obs_k = knots.copy_envs_from(knots, want_obs=True)                                # the observation at each knot
    _, _, A_lin, B_lin = knots.linearize(a_nom, args.eps, want_next=False)
    A, B = A_lin.contiguous(), B_lin.contiguous()
    print(f"linearised {K} knots in one launch: |A| max {float(A.abs().max()):.3e}, |B| max {float(B.abs().max()):.3e}", flush=True)

    # 4. backward Riccati recursion
    qdiag = torch.zeros(n2, dtype=dt, device=dev)
    for c in range(n2):
        if c not in unobserved:
            qdiag[c] = 1.0 if c < nq else 0.01
    Q, R = torch.diag(qdiag), 0.1 * torch.eye(2, dtype=dt, device=dev)
    P = Q.clone()
    gains = torch.zeros(K, 2, n2, dtype=dt, device=dev)
    for k in range(K - 1, -1, -1):
        Ak, Bk = A[k], B[k]
        Kk = torch.linalg.solve(R + Bk.T @ P @ Bk, Bk.T @ P @ Ak)
        P = Q + Ak.T @ P @ (Ak - Bk @ Kk)
        P = 0.5 * (P + P.T)
        gains[k] = Kk
    ok = torch.isfinite(gains).flatten(1).all(1)
    gains = torch.where(ok[:, None, None], gains, K_pd.expand(K, 2, n2))              # a knot that blew up falls back to the PD gain
    print(f"Riccati: {int(ok.sum())} of {K} gains finite, |K_k| max {float(gains.abs().max()):.3e}", flush=True)

    # 5. the table of weights (one set per knot: weights_of_gain takes the knots as its batch) and the two runs
    if args.riccati == "device":
        # 4. + 5. again, in one launch: K knots of one trajectory, the table in rollout_schedule's layout
        Kd, _, flags, Wd = knots.lqr_gains(A_lin, B_lin, Q.cpu(), R.cpu(), knots=K, actions=a_nom, obs=obs_k, want_weights=True)
        Kd, refused = Kd[:, 0], flags[:, 0] != 0
        both = ok & ~refused
        diff = float((Kd - gains)[both].abs().max()) if bool(both.any()) else float("nan")
        print(f"Riccati on the device: one launch, {int(refused.sum())} of {K} knots refused; largest |K_device - K_torch| {diff:.3e}",
              flush=True)
        table = torch.where(refused[:, None, None], weights_of_gain(gains, a_nom, obs_k, cols), Wd[0]).contiguous()
    else:
        table = weights_of_gain(gains, a_nom, obs_k, cols)                            # [K, 2, D+1]
    trk.copy_envs_from(knots, 0)                                                      # every tracker starts as knot 0 ...
    q, qd = trk.get_state()
    gen = torch.Generator(device=dev).manual_seed(args.seed + 1)
    observed = torch.tensor([c not in unobserved for c in range(n2)], dtype=dt, device=dev)
    noise = args.perturb * torch.randn(n2, N, dtype=dt, device=dev, generator=gen) * observed[:, None]
    trk.set_state(q + noise[:nq], qd + noise[nq:])                                    # ... perturbed
    start = trk.checkpoint()
    _, _, (o_trk, _, d_trk, _, _), _ = trk.rollout_schedule(K, table, want_outputs=True)
    trk.restore(start)
    o_open, _, d_open, _, _ = trk.rollout(K, a_nom[:, None, :].expand(K, N, 2).contiguous())

    # 6. deviation from the nominal on the raw position and velocity slots
    raw = torch.tensor([c >= 0 for c in cols], device=dev)
    for name, o, d in (("open loop", o_open, d_open), ("tracking", o_trk, d_trk)):
        dev_k = (o[:, :, raw] - o_nom[:, None, raw]).abs().amax(dim=2)                # [K, N]
        print(f"{name:9s}: max |o - o_nominal| over the slots: mean over starts {float(dev_k.mean()):.4e} along the window, "
              f"{float(dev_k[-1].mean()):.4e} at its end (worst start {float(dev_k[-1].max()):.4e}); "
              f"{int((d != 0).any(dim=0).sum())} of {N} episodes ended", flush=True)
    for e in (nom_env, knot_env, trk_env):
        e.close()


if __name__ == "__main__":
    main()
