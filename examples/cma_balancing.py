#!/usr/bin/env python3
"""CMA-ES (Cholesky-CMA-ES, Suttorp, Hansen and Igel 2009) of a linear policy for Monopod-balance-v1, entirely on the GPU, for
many populations at once.

  python examples/cma_balancing.py [--populations 4] [--samples 64] [--iters 20] [--horizon 500] [--sigma0 0.1] [--normalize]

Every iteration runs reset -> cma_sample -> rollout_policy(first_episode=True) -> cma_update (libos2r_cma.so,
include/os2r_cma.h) with no tensor reshuffled in between.  cma_sample factors the covariance of each of the M populations and
writes mean_m + sigma_m A_m z for each of its S samples, one policy per environment: environment s M + m runs sample s of
population m.  The normals z are drawn from the stepper's counter RNG by the launch that samples, and drawn again, not read, by
the launch that updates mean, step size, covariance and the two evolution paths from the one return per lane.  The populations
start alike and differ in the population word of their normals only; the best and the median population are printed.  No
observation, action, reward or policy leaves the device.

--normalize lets the policies act on whitened observations, (x - mean) / std with the running mean and deviation of everything
their population has seen so far (libos2r_norm.so, include/os2r_norm.h).  The policy is linear, so the rollout is the same launch:
reset -> cma_sample -> norm_fold (the samples on whitened observations to weights on raw ones, every lane at once) ->
rollout_policy -> cma_update -> obs_stats (the batch merged into the running statistics).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gym_os2r_amd as g
from gym_os2r_amd import cma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--populations", type=int, default=4, help="M: populations searched at once")
    ap.add_argument("--samples", type=int, default=64, help="S: samples (environments) per population")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=500, help="env-steps per rollout (the return stops at the first episode end)")
    ap.add_argument("--sigma0", type=float, default=0.1, help="the initial step size")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--normalize", action="store_true", help="running observation whitening")
    args = ap.parse_args()
    M, S = args.populations, args.samples
    if M < 1 or S < 2:
        raise SystemExit("--populations must be at least 1 and --samples at least 2")
    N = S * M
    env = g.make("Monopod-balance-v1", num_envs=N, seed=args.seed, dtype=args.dtype)
    env.reset()
    sim = env.sim
    dev, dt, D, i32 = sim.device, sim.dtype, sim.D, torch.int32
    E = 2 * (D + 1)
    new = lambda *shape, dtype=dt: torch.empty(*shape, dtype=dtype, device=dev)
    # two state sets, swapped every iteration; everything else is made once
    state = sim.cma_init(torch.zeros(M, 2, D + 1, dtype=dt, device=dev), args.sigma0)
    state_new = tuple(torch.empty_like(t) for t in state)
    factor, failed, weights = new(M, E, E), new(M, dtype=i32), new(N, 2, D + 1)
    count, status, rank = new(M, dtype=i32), new(M, dtype=i32), new(N, dtype=i32)
    rankw_host, _ = cma.constants(E, S)
    rankw = torch.tensor(rankw_host, dtype=torch.float64).to(dt).to(dev)
    if args.normalize:
        stats, stats_new = ((torch.zeros(M, dtype=torch.int64, device=dev), torch.zeros(M, D, dtype=dt, device=dev),
                             torch.zeros(M, D, dtype=dt, device=dev)) for _ in range(2))
        folded = torch.empty_like(weights)
        lane_sum, lane_count = new(2 * D, N), new(2, N, dtype=i32)
    print(f"CMA-ES on Monopod-balance-v1: {M} populations x {S} samples = {N} environments, {len(rankw_host)} parents, sigma0 {args.sigma0}, "
          f"horizon {args.horizon}, obs dim {D}{', whitened observations' if args.normalize else ''}", flush=True)
    t0 = time.time()
    for it in range(args.iters):
        obs0 = sim.reset()
        sim.cma_sample_into(state, factor, failed, weights, samples=S, generation=it)
        if args.normalize:
            sim.norm_fold_into(weights, stats, folded, lanes=N)
            ret, length, outs = sim.rollout_policy(args.horizon, folded, first_episode=True, want_outputs=True)
        else:
            ret, length, _ = sim.rollout_policy(args.horizon, weights, first_episode=True)
        _, constants = cma.constants(E, S, age=it)
        sim.cma_update_into(ret, state, factor, failed, state_new, count, status, rank, samples=S, generation=it, rankw=rankw, constants=constants)
        state, state_new = state_new, state
        if args.normalize:
            sim.obs_stats_into(outs[0], *stats_new, lane_sum, lane_count, policies=M, obs0=obs0, length=length, state=stats)
            stats, stats_new = stats_new, stats
        per_pop = ret.view(S, M).mean(0)                                           # (for the line below only)
        print(f"iteration {it}: mean return best population {float(per_pop.max()):8.2f}  median {float(per_pop.median()):8.2f}  "
              f"best lane {float(ret.max()):6.1f}  mean episode length {float(length.to(torch.float64).mean()):6.1f}  "
              f"sigma {float(state[1].min()):.4f}..{float(state[1].max()):.4f}  updated {int((status == 0).sum())} of {M}", flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    steps = args.iters * N * args.horizon
    print(f"{steps / 1e6:.1f} M env-steps in {wall:.2f} s ({steps / wall / 1e6:.1f} M env-steps/s incl. resets and updates)")
    env.close()


if __name__ == "__main__":
    main()
