#!/usr/bin/env python3
"""An unscented Kalman filter on the observation of the free-hip monopod, for many robots at once, with the simulator itself as
the process model: no Jacobian -- beside the extended Kalman filter of examples/ekf_tracking.py on the same seeds.

  python examples/ukf_tracking.py [--filter both] [--robots 4] [--steps 100] [--sigma 0.02] [--gate 0] [--q-pos 1e-4] [--q-vel 1]

A real handle of M environments (free_hip, contact on, fp64, the non-normalised task, no auto-reset), stepped with small random
actions; its observation plus Gaussian noise of --sigma is the measurement.  --filter ukf: a sigma handle of S M lanes,
S = 4 nq + 1, forked once from the real handle for its parameters (copy_envs_from(real, arange(S M) % M): lane s M + m is point s
of robot m).  Every control step
  1. sig.set_state(points[:nq], points[nq:]) puts the 2n + 1 sigma points of every robot into its lanes,
  2. sig.step(action tiled S times) pushes them through the real step, contact solve and all,
  3. sig.get_state() returns them,
  4. sig.ukf_update(state, P, meas, prec, Q=Q, done=done, want_points=True) (one os2ru_ukf_update launch, include/os2r_ukf.h)
     forms their mean and covariance, adds Q, updates both against the measurement one raw observation slot after the other, and
     writes the sigma points of the result: the `points` of step 1.
The first points come from sig.ukf_points(x, P) (os2ru_ukf_points).  No tensor is reshuffled between the four.
--filter ekf is the loop of examples/ekf_tracking.py (linearize -> ekf_update -> set_state) with the same process noise; --filter
both runs one after the other on the same seeds: the same real trajectory, the same measurements, the same first estimate.
What set_state costs: it clears the contact solver's state, so the contact solve of every sigma lane starts cold in every step,
like the first step after a reset -- more solver sweeps per step, and, within the solver's tolerance, other impulses than a warm
start would give.  The script does not work round it.
The script prints each filter's error against the true state, how many slots were gated or refused, and how many robots the
unscented filter lost (a sigma lane done or not finite) or could not factor.  It claims nothing about which filter is better
beyond these numbers: angles are averaged and compared as numbers, and the process noise is not tuned.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gym_os2r_amd as g


def track(args, name):
    """One filter (`name`: "ekf" or "ukf") over args.steps control steps on the seeds of args -> its summary line(s), printed."""
    M = args.robots
    kw = dict(task_mode="free_hip", dtype="f64", contact=True, auto_reset=False)
    real_env = g.make("Monopod-nonorm-balance-v1", num_envs=M, seed=args.seed, **kw)
    real_env.reset()
    real = real_env.sim
    dev, dt, D, nq = real.device, real.dtype, real.D, real.nq
    n = 2 * nq
    S = 4 * nq + 1 if name == "ukf" else 1
    est_env = g.make("Monopod-nonorm-balance-v1", num_envs=S * M, seed=args.seed, **kw)
    est_env.reset()
    est = est_env.sim
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    cols = [int(c) for c in est._layout().slot_col[:D]]
    q, qd = real.get_state()
    x = torch.cat((q + 0.05 * torch.randn(nq, M, dtype=dt, device=dev, generator=gen), qd))      # the estimate starts off the truth
    P = (0.05 ** 2 * torch.eye(n, dtype=dt, device=dev)).repeat(M, 1, 1)
    # the process noise of examples/ekf_tracking.py: small on the positions, large on the velocities
    Q = torch.diag(torch.tensor([args.q_pos] * nq + [args.q_vel] * nq, dtype=torch.float64))
    prec = torch.full((D,), 1.0 / args.sigma ** 2, dtype=dt, device=dev)
    live = sum(c >= 0 for c in cols)
    if name == "ukf":
        est.copy_envs_from(real, torch.arange(S * M, dtype=torch.int32, device=dev) % M)           # forked once, for the parameters
        points, failed = est.ukf_points(x, P)
    else:
        est.set_state(x[:nq], x[nq:])
    err_sum = torch.zeros((), dtype=dt, device=dev)
    noise_sum = torch.zeros((), dtype=dt, device=dev)
    applied, refusals, lost_sum, failed_sum = (torch.zeros((), dtype=torch.int64, device=dev) for _ in range(4))
    bits = 2 ** torch.arange(D, device=dev, dtype=torch.int32)
    count = lambda mask: ((mask[:, None] & bits[None]) != 0).sum()
    torch.cuda.synchronize()
    t0 = time.time()
    for k in range(args.steps):
        action = 0.2 * (2.0 * torch.rand(M, 2, dtype=dt, device=dev, generator=gen) - 1.0)
        obs_real = real.step(action, want_terminal=False)[0]
        noise = args.sigma * torch.randn(M, D, dtype=dt, device=dev, generator=gen)
        meas = obs_real + noise
        if name == "ukf":
            failed_sum += (failed != 0).sum()
            est.set_state(points[:nq], points[nq:])
            done = est.step(action.repeat(S, 1), want_terminal=False)[2]
            x, P, nis, used, refused, _, lost, points, failed = est.ukf_update(est.get_state(), P, meas, prec, Q=Q, done=done, gate=args.gate)
            lost_sum += lost.sum()
        else:
            next_q, next_qd, A, _ = est.linearize(action, want_B=False)
            x, P, nis, used, refused, _ = est.ekf_update((next_q, next_qd), P, meas, prec, A=A, Q=Q, gate=args.gate)
            est.set_state(x[:nq], x[nq:])
        q, qd = real.get_state()
        err_sum += (x - torch.cat((q, qd))).pow(2).mean().sqrt()
        noise_sum += noise.pow(2).mean().sqrt()
        applied += count(used)
        refusals += count(refused)
        if (k + 1) % 25 == 0 or k + 1 == args.steps:
            print(f"{name}, control step {k + 1}: rms error of the estimate {float(err_sum) / (k + 1):.4f} (measurement noise "
                  f"{float(noise_sum) / (k + 1):.4f}), mean nis {float(nis.mean()):.2f} over {live} slots, largest variance "
                  f"{float(P.diagonal(dim1=1, dim2=2).max()):.3e}", flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    gated = args.steps * M * live - int(applied) - int(refusals)         # (every reading here is finite and every precision positive)
    print(f"{name}: rms error {float(err_sum) / args.steps:.4f} against a measurement noise of {float(noise_sum) / args.steps:.4f} over "
          f"{args.steps} control steps of {M} robots; {gated} slots gated, {int(refusals)} refused of {args.steps * M * live}; "
          f"{args.steps * M / wall:.0f} filter steps/s incl. the real handle's step and set_state")
    if name == "ukf":
        print(f"ukf: {int(lost_sum)} robots lost, {int(failed_sum)} factors failed over {args.steps} control steps of {M} robots "
              f"({S} sigma lanes each)")
    real_env.close(); est_env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filter", choices=["ekf", "ukf", "both"], default="both")
    ap.add_argument("--robots", type=int, default=4, help="real robots tracked at once")
    ap.add_argument("--steps", type=int, default=100, help="control steps")
    ap.add_argument("--sigma", type=float, default=0.02, help="standard deviation of the measurement noise, per observation entry")
    ap.add_argument("--gate", type=float, default=0.0, help="leave out a slot whose normalised innovation squared exceeds this (0: no gate)")
    ap.add_argument("--q-pos", type=float, default=1e-4, help="process noise variance of a position, per control step")
    ap.add_argument("--q-vel", type=float, default=1.0, help="process noise variance of a velocity, per control step")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    names = ("ukf", "ekf") if args.filter == "both" else (args.filter,)
    print(f"filters {', '.join(names)} on the free-hip monopod: {args.robots} robots, {args.steps} control steps", flush=True)
    for name in names:
        track(args, name)


if __name__ == "__main__":
    main()
