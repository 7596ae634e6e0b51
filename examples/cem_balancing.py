#!/usr/bin/env python3
"""Cross-entropy-method planning (CEM; the shooting planner of PETS and PlaNet) of Monopod-balance-v1 with the simulator as the
model.

  python examples/cem_balancing.py [--steps 100] [--robots 1] [--lanes 256] [--elites 32] [--horizon 20] [--iters 3] [--sigma 0.4]
                                   [--gain 1.0] [--sigma-gain 1.0] [--sigma-min 0.05]

Two handles: a real handle of --robots M environments and a planner of --lanes x M without auto-reset, lane s M + m being sample
s of robot m.  Every control step
  1. --iters times:
       planner.copy_envs_from(real, arange(N) % M) forks every robot into its lanes (one launch; every iteration plans from the
       real robots' present state, so the fork is repeated: a rollout leaves the lanes a horizon further),
       planner.rollout_schedule(horizon, table, sigma=lane_sigma, salt=..., first_episode=True, want_actions=True) is the sampled
       rollout: every lane applies clip(nominal + sigma eps), sigma its robot's current width, the salt new in every iteration,
       planner.cem_update(...) (one os2rx_cem_update call, include/os2r_cem.h) picks the best --elites lanes of every robot and
       moves the nominal to their mean and the width to their pooled standard deviation, both written where the next rollout
       reads them; shift=0 on all iterations but the last, shift=1 on the last,
  2. the width is reset to --sigma for the next control step,
  3. real.step(applied).
No tensor is reshuffled in between.  Nothing but the printed numbers leaves the device.  The script prints what a run achieved;
it claims no control quality.
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
    ap.add_argument("--steps", type=int, default=100, help="control steps of the real robots")
    ap.add_argument("--robots", type=int, default=1, help="real robots planned for at once")
    ap.add_argument("--lanes", type=int, default=256, help="sampled action sequences per robot")
    ap.add_argument("--elites", type=int, default=32, help="lanes of every robot the distribution is refitted from")
    ap.add_argument("--horizon", type=int, default=20, help="env-steps per planner rollout")
    ap.add_argument("--iters", type=int, default=3, help="rollout and update per control step")
    ap.add_argument("--sigma", type=float, default=0.4, help="the sampling width every control step starts with")
    ap.add_argument("--gain", type=float, default=1.0, help="how far the nominal moves towards the elite mean, in (0, 1]")
    ap.add_argument("--sigma-gain", type=float, default=1.0, help="how far the width moves towards the elites', in (0, 1]")
    ap.add_argument("--sigma-min", type=float, default=0.05, help="the floor of the width")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    M, S, E, H, I = args.robots, args.lanes, args.elites, args.horizon, args.iters
    N = S * M
    sigma_max = max(args.sigma, args.sigma_min)
    real_env = g.make("Monopod-balance-v1", num_envs=M, seed=args.seed)
    plan_env = g.make("Monopod-balance-v1", num_envs=N, seed=args.seed + 1, auto_reset=False)
    real_env.reset(); plan_env.reset()
    real, planner = real_env.sim, plan_env.sim
    dev, dt = real.device, real.dtype
    index = (torch.arange(N, device=dev) % M).to(torch.int32)
    nominal = torch.zeros(H, M, 2, dtype=dt, device=dev)
    # the width as cem_update returns it: transposed views of [2, M] and [2, N] buffers, which go on without a copy
    sigma0 = torch.full((2, M), args.sigma, dtype=dt, device=dev).t()
    lane0 = torch.full((2, N), args.sigma, dtype=dt, device=dev).t()
    total = torch.zeros(M, dtype=dt, device=dev)
    episodes = torch.zeros(M, dtype=torch.int64, device=dev)
    widths = torch.zeros(I, dtype=dt, device=dev)
    print(f"CEM on Monopod-balance-v1: {M} robots x {S} lanes ({E} elites) x horizon {H} x {I} iterations, {args.steps} control steps, "
          f"sigma in [{args.sigma_min}, {sigma_max}]", flush=True)
    # the table rollout_schedule reads and cem_update writes the bias column of: all zeros is the zero nominal
    table = torch.zeros(H, 2, planner.D + 1, N, dtype=dt, device=dev).permute(3, 0, 1, 2)
    torch.cuda.synchronize()
    t0 = time.time()
    for k in range(args.steps):
        sigma, lane_sigma = sigma0, lane0
        for i in range(I):
            planner.copy_envs_from(real, index)
            ret, _, _, (acts, _) = planner.rollout_schedule(H, table, sigma=lane_sigma, salt=k * I + i, first_episode=True, want_actions=True)
            applied, nominal, table, sigma, lane_sigma, _, _, _, _ = planner.cem_update(
                ret, acts, nominal, sigma, samples=S, elites=E, gain=args.gain, sigma_gain=args.sigma_gain, sigma_min=args.sigma_min,
                sigma_max=sigma_max, shift=1 if i == I - 1 else 0, tail="zero", table=table, want_variance=False)
            widths[i] = sigma.mean()
        _, r, d, _ = real.step(applied, want_terminal=False)
        total += r
        episodes += d != 0
        print(f"control step {k + 1}: mean return so far {float(total.mean()):9.2f}, mean sigma per iteration "
              + " ".join(f"{v:.4f}" for v in widths.tolist()), flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    steps = args.steps * (I * N * H + M)
    print("return per robot: " + " ".join(f"{v:.2f}" for v in total.tolist()))
    print(f"mean return {float(total.mean()):.2f} (min {float(total.min()):.2f}, max {float(total.max()):.2f}) over {args.steps} control steps of "
          f"{M} robots ({int(episodes.sum())} episodes ended); {steps / 1e6:.2f} M env-steps in {wall:.2f} s "
          f"({steps / wall / 1e6:.2f} M env-steps/s incl. copies and updates)")
    real_env.close(); plan_env.close()


if __name__ == "__main__":
    main()
