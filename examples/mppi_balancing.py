#!/usr/bin/env python3
"""Model-predictive path integral control (MPPI, Williams et al. 2017) of Monopod-balance-v1 with the simulator as the model.

  python examples/mppi_balancing.py [--steps 200] [--lanes 256] [--horizon 20] [--sigma 0.4] [--temperature 0.5]

Two handles: a one-environment "real" robot and a planner of --lanes environments without auto-reset.  Every control step
  1. copies the real robot's complete state and parameters into every planner lane (one os2r_copy_envs launch:
     HipSim.copy_envs_from(real, 0)),
  2. rolls the lanes --horizon env-steps under the nominal action sequence plus Gaussian noise (one os2r_rollout call),
  3. weights the lanes by softmin of their cost (minus the reward summed until the lane's first done flag) and moves the
     nominal sequence to the weighted mean of the lanes' sequences,
  4. applies the first nominal action to the real robot and shifts the sequence.
Nothing but the printed numbers leaves the device.  The script prints what a run achieved; it claims no control quality.
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
    ap.add_argument("--steps", type=int, default=200, help="control steps of the real robot")
    ap.add_argument("--lanes", type=int, default=256, help="planner environments (sampled action sequences)")
    ap.add_argument("--horizon", type=int, default=20, help="env-steps per planner rollout")
    ap.add_argument("--sigma", type=float, default=0.4, help="standard deviation of the action noise")
    ap.add_argument("--temperature", type=float, default=0.5, help="softmin temperature on the summed reward")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    L, H = args.lanes, args.horizon
    real_env = g.make("Monopod-balance-v1", num_envs=1, seed=args.seed)
    plan_env = g.make("Monopod-balance-v1", num_envs=L, seed=args.seed + 1, auto_reset=False)
    real_env.reset(); plan_env.reset()
    real, planner = real_env.sim, plan_env.sim
    dev, dt = real.device, real.dtype
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    nominal = torch.zeros(H, 2, dtype=dt, device=dev)
    total = torch.zeros((), dtype=dt, device=dev)
    episodes = torch.zeros((), dtype=torch.int64, device=dev)
    print(f"MPPI on Monopod-balance-v1: {L} lanes x horizon {H}, {args.steps} control steps", flush=True)
    torch.cuda.synchronize()
    t0 = time.time()
    for k in range(args.steps):
        planner.copy_envs_from(real, 0)
        acts = (nominal[:, None, :] + args.sigma * torch.randn(H, L, 2, dtype=dt, device=dev, generator=gen)).clamp_(-1.0, 1.0)
        _, rew, done, _, _ = planner.rollout(H, acts)
        ended = (done != 0).to(dt).cumsum(0)
        alive = torch.cat([torch.ones(1, L, dtype=dt, device=dev), (ended[:-1] == 0).to(dt)])   # until the lane's first done flag
        ret = (rew * alive).sum(0)
        w = torch.softmax((ret - ret.max()) / args.temperature, 0)
        nominal = torch.einsum("l,hlj->hj", w, acts)
        _, r, d, _ = real.step(nominal[0:1], want_terminal=False)
        total += r[0]
        over = d[0] != 0
        episodes += over
        nominal = torch.where(over, torch.zeros_like(nominal), torch.cat([nominal[1:], torch.zeros(1, 2, dtype=dt, device=dev)]))
        if (k + 1) % 50 == 0 or k + 1 == args.steps:
            print(f"control step {k + 1}: return so far {float(total):9.2f}, episodes ended {int(episodes)}", flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    steps = args.steps * (L * H + 1)
    print(f"return {float(total):.2f} over {args.steps} control steps ({int(episodes)} episodes ended); "
          f"{steps / 1e6:.2f} M env-steps in {wall:.2f} s ({steps / wall / 1e6:.2f} M env-steps/s incl. copies and updates)")
    real_env.close(); plan_env.close()


if __name__ == "__main__":
    main()
