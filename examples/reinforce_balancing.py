#!/usr/bin/env python3
"""REINFORCE (Williams 1992) with a batch baseline for a linear-Gaussian policy on Monopod-balance-v1, entirely on the GPU.

  python examples/reinforce_balancing.py [--envs 8192] [--iters 20] [--horizon 500] [--step-size 0.05] [--sigma 0.2]
                                         [--gradient torch|device] [--weight return|reward-to-go] [--gamma 1.0]

The policy is a = clip(theta . [o; 1] + sigma * eps), eps ~ N(0, 1) per action and env-step.  Every iteration resets the batch and
runs ONE os2r_rollout_policy_noisy call: all environments share theta, the noise is drawn inside the rollout kernel, and the
call returns the observations, the applied actions and the noise per step and the return of each environment's first episode.
The score of step k is grad_theta log pi = eps / sigma * [o; 1] on the action components where the clip did not bind (where it
did, the applied action does not depend on theta to first order and the step contributes nothing); the update is
theta += step * mean_e[ (R_e - mean R) / std R * sum_k score_ek ] / mean episode length.  Nothing leaves the device.

--gradient torch (the default) forms the update with five torch statements; --gradient device with one policy_gradient call
(include/os2r_pg.h) on the arrays the rollout returned, as they are: reset -> rollout_policy -> policy_gradient -> theta +=.
--weight reward-to-go (device only) weights every step with its discounted reward-to-go (--gamma) minus the batch's mean
reward-to-go of that step, in place of the lane's normalised return.
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
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=500, help="env-steps per rollout (the return stops at the first episode end)")
    ap.add_argument("--step-size", type=float, default=0.05)
    ap.add_argument("--sigma", type=float, default=0.2, help="standard deviation of the exploration noise on both actions")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--gradient", default="torch", choices=["torch", "device"], help="the update: five torch statements, or one policy_gradient call")
    ap.add_argument("--weight", default="return", choices=["return", "reward-to-go"], help="what weights a step's score (reward-to-go: device only)")
    ap.add_argument("--gamma", type=float, default=1.0, help="the discount of the reward-to-go")
    args = ap.parse_args()
    if args.weight == "reward-to-go" and args.gradient != "device":
        ap.error("--weight reward-to-go needs --gradient device")
    N, H = args.envs, args.horizon
    env = g.make("Monopod-balance-v1", num_envs=N, seed=args.seed, dtype=args.dtype)
    env.reset()
    sim = env.sim
    dev, dt, D = sim.device, sim.dtype, sim.D
    theta = torch.zeros(2, D + 1, dtype=dt, device=dev)
    sigma = torch.full((2,), args.sigma, dtype=dt, device=dev)
    print(f"REINFORCE on Monopod-balance-v1: {N} environments, horizon {H}, obs dim {D}, sigma {args.sigma}", flush=True)
    t0 = time.time()
    for it in range(args.iters):
        obs0 = sim.reset()
        if args.gradient == "device":
            ret, length, (O, R, Dn, _, _), (A, E) = sim.rollout_policy(H, theta, sigma=sigma, salt=it, first_episode=True,
                                                                       want_outputs=True, want_actions=True, want_noise=True)
            if args.weight == "return":
                weight = dict(adv=(ret - ret.mean()) / ret.std().clamp_min(1e-8))                  # batch baseline
            else:
                # the baseline of step k is the batch's mean discounted reward from k on, from the per-step means (an episode that
                # has ended counts as 0 from there on)
                counted = (torch.arange(H, device=dev).unsqueeze(1) < length.unsqueeze(0)).to(dt)
                ahead = torch.arange(H, device=dev).unsqueeze(0) - torch.arange(H, device=dev).unsqueeze(1)      # [k, i]: i - k
                discount = torch.triu(torch.full((H, H), args.gamma, dtype=dt, device=dev) ** ahead.clamp_min(0))
                base = (discount @ (R * counted).mean(1)).unsqueeze(1)                               # [H, 1]
                weight = dict(rewards=R, done=Dn, gamma=args.gamma, baseline=base)
            grad, steps, clipped, valid, _, _, _ = sim.policy_gradient(O, E, sigma, obs0=obs0, actions=A, length=length, **weight)
            mean_len = float(steps[0]) / max(int(valid[0]), 1)
            theta = theta + args.step_size * grad[0] / float(max(int(steps[0]), 1))
            print(f"iteration {it}: mean return {float(ret.mean()):8.2f}  best {float(ret.max()):6.1f}  "
                  f"mean episode length {mean_len:6.1f}  clipped {100 * float(clipped.sum()) / float(max(2 * int(steps[0]), 1)):4.1f} %", flush=True)
            continue
        # (the salt separates the iterations' noise: every rollout starts at another step counter anyway, the salt makes it explicit)
        ret, length, (O, _, Dn, _, _), (A, E) = sim.rollout_policy(H, theta, sigma=sigma, salt=it, first_episode=True,
                                                                   want_outputs=True, want_actions=True, want_noise=True)
        prev = torch.cat([obs0.unsqueeze(0), O[:-1]])                                   # [H, N, D]: the observation each action saw
        ended = (Dn != 0).to(torch.int32)
        alive = ((torch.cumsum(ended, 0) - ended) == 0).to(dt)                          # [H, N]: step k belongs to the first episode
        adv = (ret - ret.mean()) / ret.std().clamp_min(1e-8)                            # batch baseline
        coef = (A.abs() < 1.0).to(dt) * E / sigma * (alive * adv.unsqueeze(0)).unsqueeze(-1)   # [H, N, 2]
        grad = torch.cat([torch.einsum("knj,knd->jd", coef, prev), coef.sum((0, 1)).unsqueeze(1)], 1)
        mean_len = float(length.to(torch.float64).mean())
        theta = theta + args.step_size * grad / (N * mean_len)
        print(f"iteration {it}: mean return {float(ret.mean()):8.2f}  best {float(ret.max()):6.1f}  "
              f"mean episode length {mean_len:6.1f}  clipped {100 * float((A.abs() >= 1.0).to(dt).mean()):4.1f} %", flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    steps = args.iters * N * H
    print(f"{steps / 1e6:.1f} M env-steps in {wall:.2f} s ({steps / wall / 1e6:.1f} M env-steps/s incl. resets and updates)")
    print(f"gradient {args.gradient}, weight {args.weight}: torch's peak allocated memory {torch.cuda.max_memory_allocated(dev) / 1e6:.0f} MB")
    env.close()


if __name__ == "__main__":
    main()
