#!/usr/bin/env python3
"""Model-predictive path integral control (MPPI, Williams et al. 2017) of Monopod-balance-v1 with the simulator as the model.

  python examples/mppi_balancing.py [--steps 200] [--lanes 256] [--horizon 20] [--sigma 0.4] [--temperature 0.5]
                                    [--update torch|device] [--robots 1]

Two handles: a one-environment "real" robot and a planner of --lanes environments without auto-reset.  Every control step
  1. copies the real robot's complete state and parameters into every planner lane (one os2r_copy_envs launch:
     HipSim.copy_envs_from(real, 0)),
  2. rolls the lanes --horizon env-steps under the nominal action sequence plus Gaussian noise (one os2r_rollout call),
  3. weights the lanes by softmin of their cost (minus the reward summed until the lane's first done flag) and moves the
     nominal sequence to the weighted mean of the lanes' sequences,
  4. applies the first nominal action to the real robot and shifts the sequence.
Nothing but the printed numbers leaves the device.  The script prints what a run achieved; it claims no control quality.

--update device plans for --robots real robots at once with three launches and a step per control step, no tensor reshuffled in
between: a real handle of M environments and a planner of --lanes x M, lane s M + m being sample s of robot m;
  1. planner.copy_envs_from(real, arange(N) % M) forks every robot into its lanes,
  2. planner.rollout_schedule(horizon, table, sigma=..., first_episode=True, want_actions=True) is the sampled rollout: the table's
     weight columns are zero and its bias column holds the nominal, so every lane applies clip(nominal + sigma eps) with eps from
     the counter RNG, and the call returns the reward summed until the lane's first done flag and the applied actions,
  3. planner.mppi_update(...) (one os2rm_mppi_update launch, include/os2r_mppi.h) weights every robot's lanes, forms the new
     nominal, shifts it, writes it into the table's bias column and returns the action to apply,
  4. real.step(applied).
A robot whose episode just ended keeps its shifted nominal; its next samples start from the reset state and are weighted there.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gym_os2r_amd as g


def device_update(args):
    """--update device: M robots, every control step copy_envs_from -> rollout_schedule -> mppi_update -> step."""
    M, S, H = args.robots, args.lanes, args.horizon
    N = S * M
    real_env = g.make("Monopod-balance-v1", num_envs=M, seed=args.seed)
    plan_env = g.make("Monopod-balance-v1", num_envs=N, seed=args.seed + 1, auto_reset=False)
    real_env.reset(); plan_env.reset()
    real, planner = real_env.sim, plan_env.sim
    dev, dt = real.device, real.dtype
    index = (torch.arange(N, device=dev) % M).to(torch.int32)
    nominal = torch.zeros(H, M, 2, dtype=dt, device=dev)
    total = torch.zeros(M, dtype=dt, device=dev)
    episodes = torch.zeros(M, dtype=torch.int64, device=dev)
    print(f"MPPI on Monopod-balance-v1: {M} robots x {S} lanes x horizon {H}, {args.steps} control steps, update on the device", flush=True)
    # the table rollout_schedule reads and mppi_update writes the bias column of: all zeros is the zero nominal
    table = torch.zeros(H, 2, planner.D + 1, N, dtype=dt, device=dev).permute(3, 0, 1, 2)
    torch.cuda.synchronize()
    t0 = time.time()
    for k in range(args.steps):
        planner.copy_envs_from(real, index)
        ret, _, _, (acts, _) = planner.rollout_schedule(H, table, sigma=args.sigma, first_episode=True, want_actions=True)
        applied, nominal, table, _, _, _ = planner.mppi_update(ret, acts, nominal, samples=S, temperature=args.temperature, shift=1,
                                                               tail="zero", table=table)
        _, r, d, _ = real.step(applied, want_terminal=False)
        total += r
        episodes += d != 0
        if (k + 1) % 50 == 0 or k + 1 == args.steps:
            print(f"control step {k + 1}: mean return so far {float(total.mean()):9.2f}, episodes ended {int(episodes.sum())}", flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    steps = args.steps * (N * H + M)
    print(f"mean return {float(total.mean()):.2f} (min {float(total.min()):.2f}, max {float(total.max()):.2f}) over {args.steps} control steps of "
          f"{M} robots ({int(episodes.sum())} episodes ended); {steps / 1e6:.2f} M env-steps in {wall:.2f} s "
          f"({steps / wall / 1e6:.2f} M env-steps/s incl. copies and updates)")
    real_env.close(); plan_env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="control steps of the real robot")
    ap.add_argument("--lanes", type=int, default=256, help="planner environments (sampled action sequences)")
    ap.add_argument("--horizon", type=int, default=20, help="env-steps per planner rollout")
    ap.add_argument("--sigma", type=float, default=0.4, help="standard deviation of the action noise")
    ap.add_argument("--temperature", type=float, default=0.5, help="softmin temperature on the summed reward")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--update", choices=["torch", "device"], default="torch",
                    help="torch: the update in torch statements, one robot; device: one os2rm_mppi_update launch, --robots robots")
    ap.add_argument("--robots", type=int, default=1, help="real robots planned for at once (--update device; --lanes is per robot)")
    args = ap.parse_args()
    if args.update == "device":
        return device_update(args)
    if args.robots != 1:
        ap.error("--robots needs --update device (the torch update plans for one robot)")
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
