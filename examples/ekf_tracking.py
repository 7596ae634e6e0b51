#!/usr/bin/env python3
"""An extended Kalman filter on the observation of the free-hip monopod, for many robots at once, with the simulator as the
process model and its finite-difference Jacobian as the linearisation.

  python examples/ekf_tracking.py [--robots 4] [--steps 100] [--sigma 0.02] [--gate 0] [--q-pos 1e-4] [--q-vel 1]

Two handles of M environments each (free_hip, contact on, fp64, the non-normalised task, no auto-reset: a real robot that was
reset behind the filter's back would be a jump no process noise covers): a real handle, stepped with small random actions, and
an estimate handle that starts from a perturbed state.  Every control step
  1. real.step(action); its observation plus Gaussian noise of --sigma is the measurement,
  2. est.linearize(action) returns, without advancing the estimate handle, the predicted state `next` and A = dx'/dx,
  3. est.ekf_update((next_q, next_qd), P, meas, prec, A=A, Q=Q, gate=...) (one os2re_ekf_update launch, include/os2r_ekf.h) forms
     P- = A P A' + Q and updates state and covariance against the measurement, one raw observation slot after the other,
  4. est.set_state(x[:nq], x[nq:]) puts the estimate into the handle for the next linearisation.
No tensor is reshuffled between 2, 3 and 4: linearize()'s tensors and the P of the call before go on without a copy.
What set_state costs: it clears the contact solver's state, so every linearisation here starts its contact solve cold, like
the first step after a reset -- more solver sweeps per step, and, within the solver's tolerance, other impulses than a warm
start would give.  A caller that also steps the estimate handle (est.step in place of `next`) keeps the warm start by reading
get_solver_state() before set_state() and handing it back with set_solver_state() afterwards.
The script prints the estimate's error against the true state and how many slots were gated or refused; it claims no filtering
quality: across a change of contact mode A is a secant, and the innovation of an angle is not wrapped.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gym_os2r_amd as g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=4, help="real robots tracked at once")
    ap.add_argument("--steps", type=int, default=100, help="control steps")
    ap.add_argument("--sigma", type=float, default=0.02, help="standard deviation of the measurement noise, per observation entry")
    ap.add_argument("--gate", type=float, default=0.0, help="leave out a slot whose normalised innovation squared exceeds this (0: no gate)")
    ap.add_argument("--q-pos", type=float, default=1e-4, help="process noise variance of a position, per control step")
    ap.add_argument("--q-vel", type=float, default=1.0, help="process noise variance of a velocity, per control step")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    M = args.robots
    kw = dict(num_envs=M, task_mode="free_hip", dtype="f64", contact=True, auto_reset=False)
    real_env = g.make("Monopod-nonorm-balance-v1", seed=args.seed, **kw)
    est_env = g.make("Monopod-nonorm-balance-v1", seed=args.seed, **kw)
    real_env.reset(); est_env.reset()
    real, est = real_env.sim, est_env.sim
    dev, dt, D, nq = real.device, real.dtype, real.D, real.nq
    n = 2 * nq
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    cols = [int(c) for c in est._layout().slot_col[:D]]
    q, qd = real.get_state()
    est.set_state(q + 0.05 * torch.randn(nq, M, dtype=dt, device=dev, generator=gen), qd)      # the estimate starts off the truth
    P = (0.05 ** 2 * torch.eye(n, dtype=dt, device=dev)).repeat(M, 1, 1)
    # the process noise: small on the positions, large on the velocities -- with a foot on the ground the stiff contact turns a
    # position error of a hundredth of a radian into predicted joint velocities that are off by several rad/s, so the
    # velocities are taken from their measurements and the positions are filtered
    Q = torch.diag(torch.tensor([args.q_pos] * nq + [args.q_vel] * nq, dtype=torch.float64))
    prec = torch.full((D,), 1.0 / args.sigma ** 2, dtype=dt, device=dev)
    live = sum(c >= 0 for c in cols)
    print(f"extended Kalman filter on the free-hip monopod: {M} robots, {args.steps} control steps, observation slots -> state columns "
          f"{cols}", flush=True)
    err_sum = torch.zeros((), dtype=dt, device=dev)
    noise_sum = torch.zeros((), dtype=dt, device=dev)
    applied = torch.zeros((), dtype=torch.int64, device=dev)
    refusals = torch.zeros((), dtype=torch.int64, device=dev)
    bits = 2 ** torch.arange(D, device=dev, dtype=torch.int32)
    count = lambda mask: ((mask[:, None] & bits[None]) != 0).sum()
    torch.cuda.synchronize()
    t0 = time.time()
    for k in range(args.steps):
        action = 0.2 * (2.0 * torch.rand(M, 2, dtype=dt, device=dev, generator=gen) - 1.0)
        obs_real = real.step(action, want_terminal=False)[0]
        noise = args.sigma * torch.randn(M, D, dtype=dt, device=dev, generator=gen)
        meas = obs_real + noise
        next_q, next_qd, A, _ = est.linearize(action, want_B=False)
        x, P, nis, used, refused, _ = est.ekf_update((next_q, next_qd), P, meas, prec, A=A, Q=Q, gate=args.gate)
        est.set_state(x[:nq], x[nq:])
        q, qd = real.get_state()
        err_sum += (x - torch.cat((q, qd))).pow(2).mean().sqrt()
        noise_sum += noise.pow(2).mean().sqrt()
        applied += count(used)
        refusals += count(refused)
        if (k + 1) % 25 == 0 or k + 1 == args.steps:
            print(f"control step {k + 1}: rms error of the estimate {float(err_sum) / (k + 1):.4f} (measurement noise "
                  f"{float(noise_sum) / (k + 1):.4f}), mean nis {float(nis.mean()):.2f} over {live} slots, largest variance "
                  f"{float(P.diagonal(dim1=1, dim2=2).max()):.3e}", flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    gated = args.steps * M * live - int(applied) - int(refusals)         # (every reading here is finite and every precision positive)
    print(f"rms error {float(err_sum) / args.steps:.4f} against a measurement noise of {float(noise_sum) / args.steps:.4f} over {args.steps} "
          f"control steps of {M} robots; {gated} slots gated, {int(refusals)} refused of {args.steps * M * live}; "
          f"{args.steps * M / wall:.0f} filter steps/s incl. the real handle's step and set_state")
    real_env.close(); est_env.close()


if __name__ == "__main__":
    main()
