#!/usr/bin/env python3
"""Basic augmented random search (ARS, Mania et al. 2018) of a linear policy for Monopod-balance-v1, entirely on the GPU.

  python examples/ars_balancing.py [--envs 8192] [--iters 20] [--horizon 500] [--step-size 0.02] [--noise 0.03]

Every iteration perturbs the policy theta [2, D+1] (row j: weights of action j on the D observations, then its bias) along
P = envs / 2 random directions delta_p, runs theta + nu*delta_p on environment p and theta - nu*delta_p on environment P + p --
per-env weights of ONE os2r_rollout_policy call, after a reset, the returns summed over each environment's first episode --
and moves theta along sum_p (R+_p - R-_p) delta_p / (P * std(R)).  No observation, action or reward leaves the device.
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
    ap.add_argument("--envs", type=int, default=8192, help="environments = 2 x perturbation directions")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=500, help="env-steps per rollout (the return stops at the first episode end)")
    ap.add_argument("--step-size", type=float, default=0.02)
    ap.add_argument("--noise", type=float, default=0.03, help="nu: scale of the perturbations")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    args = ap.parse_args()
    P = args.envs // 2
    if P < 1:
        raise SystemExit("--envs must be at least 2")
    env = g.make("Monopod-balance-v1", num_envs=2 * P, seed=args.seed, dtype=args.dtype)
    env.reset()
    sim = env.sim
    dev, dt, D = sim.device, sim.dtype, sim.D
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    theta = torch.zeros(2, D + 1, dtype=dt, device=dev)
    print(f"ARS on Monopod-balance-v1: {P} directions x 2 = {2 * P} environments, horizon {args.horizon}, obs dim {D}", flush=True)
    t0 = time.time()
    for it in range(args.iters):
        delta = torch.randn(P, 2, D + 1, dtype=dt, device=dev, generator=gen)
        w = torch.cat([theta + args.noise * delta, theta - args.noise * delta])     # [2P, 2, D+1]: one policy per environment
        sim.reset()
        ret, length, _ = sim.rollout_policy(args.horizon, w, first_episode=True)
        r_plus, r_minus = ret[:P], ret[P:]
        sigma = ret.std().clamp_min(1e-8)
        theta = theta + args.step_size / (P * sigma) * torch.einsum("p,pjd->jd", r_plus - r_minus, delta)
        print(f"iteration {it}: mean return {float(ret.mean()):8.2f}  best {float(ret.max()):6.1f}  "
              f"mean episode length {float(length.to(torch.float64).mean()):6.1f}", flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    steps = args.iters * 2 * P * args.horizon
    print(f"{steps / 1e6:.1f} M env-steps in {wall:.2f} s ({steps / wall / 1e6:.1f} M env-steps/s incl. resets and updates)")
    env.close()


if __name__ == "__main__":
    main()
