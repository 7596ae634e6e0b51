#!/usr/bin/env python3
"""A particle filter on the observation of Monopod-balance-v1, for many robots at once, with the simulator as the process model.

  python examples/pf_tracking.py [--robots 4] [--particles 256] [--steps 100] [--meas-sigma 0.05] [--proc-sigma 0.1]
                                 [--resample-ratio 0.5]

Two handles: a real handle of M robots and a particle handle of S x M environments without auto-reset, lane s M + m being
particle s of robot m, forked once by particles.copy_envs_from(real, arange(N) % M).  Every control step
  1. steps both with the same action: real.step(action), and particles.rollout_policy(1, weights, sigma=proc_sigma), whose bias
     column holds the action of the lane's robot, so that every particle applies clip(action + proc_sigma eps): process noise,
  2. forms the measurement meas = obs_real + meas_sigma noise,
  3. particles.pf_update(obs, meas, prec, ...) (one os2rp_pf_update launch, include/os2r_pf.h) weights every robot's particles,
     forms the estimate and, where the effective sample size fell below --resample-ratio S, the resampling index,
  4. particles.copy_envs_from(particles, index) moves the ancestors' complete state into their offspring (-1: the lane stays).
No tensor is reshuffled in between, and nothing but the printed numbers leaves the device.  The script prints the estimate's
error against the true observation and how many robots resampled; it claims no filtering quality.
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
    ap.add_argument("--particles", type=int, default=256, help="particles per robot")
    ap.add_argument("--steps", type=int, default=100, help="control steps")
    ap.add_argument("--meas-sigma", type=float, default=0.05, help="standard deviation of the measurement noise, per observation entry")
    ap.add_argument("--proc-sigma", type=float, default=0.1, help="standard deviation of the particles' action noise")
    ap.add_argument("--resample-ratio", type=float, default=0.5, help="resample a robot whose effective sample size is below this share of S")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    M, S = args.robots, args.particles
    N = S * M
    real_env = g.make("Monopod-balance-v1", num_envs=M, seed=args.seed)
    part_env = g.make("Monopod-balance-v1", num_envs=N, seed=args.seed + 1, auto_reset=False)
    real_env.reset(); part_env.reset()
    real, particles = real_env.sim, part_env.sim
    dev, dt, D = real.device, real.dtype, real.D
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    lane_robot = torch.arange(N, device=dev) % M
    particles.copy_envs_from(real, lane_robot.to(torch.int32))
    prec = torch.full((D,), 1.0 / args.meas_sigma ** 2, dtype=dt, device=dev)
    weights = torch.zeros(N, 2, D + 1, dtype=dt, device=dev)         # the per-environment policy: zero gains, the action as its bias
    logw = None
    print(f"particle filter on Monopod-balance-v1: {M} robots x {S} particles, {args.steps} control steps", flush=True)
    err_sum = torch.zeros((), dtype=dt, device=dev)
    noise_sum = torch.zeros((), dtype=dt, device=dev)
    resamplings = torch.zeros((), dtype=torch.int64, device=dev)
    lost = torch.zeros((), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t0 = time.time()
    for k in range(args.steps):
        action = 0.3 * torch.sin(torch.full((M, 2), 0.05 * k, dtype=dt, device=dev) + torch.arange(M, device=dev, dtype=dt)[:, None])
        obs_real = real.step(action, want_terminal=False)[0]
        weights[:, :, D] = action[lane_robot]
        outs = particles.rollout_policy(1, weights, sigma=args.proc_sigma, want_outputs=True)[2]
        obs = outs[0][0]                                               # [N, D]: the observation after the one step
        noise = args.meas_sigma * torch.randn(M, D, dtype=dt, device=dev, generator=gen)
        meas = obs_real + noise
        u = torch.rand(M, dtype=dt, device=dev, generator=gen)
        logw, index, est, _, ess, count, resampled = particles.pf_update(obs, meas, prec, particles=S, logw=logw, u=u,
                                                                         resample_ratio=args.resample_ratio)
        particles.copy_envs_from(particles, index)
        err_sum += (est - obs_real).pow(2).mean().sqrt()
        noise_sum += noise.pow(2).mean().sqrt()
        resamplings += resampled.sum()
        lost += (count == 0).sum()
        if (k + 1) % 25 == 0 or k + 1 == args.steps:
            print(f"control step {k + 1}: rms error of the estimate {float(err_sum) / (k + 1):.4f} (of the measurement "
                  f"{float(noise_sum) / (k + 1):.4f}), mean ess {float(ess.mean()):.1f} of {S}, robots resampled so far "
                  f"{int(resamplings)}, lost {int(lost)}", flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    print(f"rms error {float(err_sum) / args.steps:.4f} against a measurement noise of {float(noise_sum) / args.steps:.4f} over {args.steps} "
          f"control steps of {M} robots; {int(resamplings)} resamplings, {int(lost)} times a robot was lost; "
          f"{args.steps * (N + M) / wall / 1e6:.3f} M env-steps/s incl. updates and copies")
    real_env.close(); part_env.close()


if __name__ == "__main__":
    main()
