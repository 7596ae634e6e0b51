#!/usr/bin/env python3
"""Basic augmented random search (ARS, Mania et al. 2018) of a linear policy for Monopod-balance-v1, entirely on the GPU.

  python examples/ars_balancing.py [--envs 8192] [--iters 20] [--horizon 500] [--step-size 0.02] [--noise 0.03]
                                   [--update torch|device] [--populations 1] [--top 0] [--normalize]

Every iteration perturbs the policy theta [2, D+1] (row j: weights of action j on the D observations, then its bias) along
P = envs / 2 random directions delta_p, runs theta + nu*delta_p on environment p and theta - nu*delta_p on environment P + p --
per-env weights of ONE os2r_rollout_policy call, after a reset, the returns summed over each environment's first episode --
and moves theta along sum_p (R+_p - R-_p) delta_p / (P * std(R)).  No observation, action or reward leaves the device.

--update device runs reset -> es_perturb -> rollout_policy -> es_update (libos2r_es.so, include/os2r_es.h) with no tensor
reshuffled in between: the directions are drawn from the stepper's counter RNG by the launch that perturbs, and drawn again,
not read, by the launch that updates.  --populations M searches M policies at once on envs / (2 M) directions each -- they
start alike and differ in the population word of their directions only --, --top b keeps the b best directions of each
(ARS V1-t); the best and the median population are printed.

--update device --normalize is ARS V2-t: the policy acts on whitened observations, (x - mean) / std with the running mean and
deviation of everything its population has seen so far (libos2r_norm.so, include/os2r_norm.h).  The policy is linear, so the
rollout is the same launch: reset -> es_perturb -> norm_fold (theta +- nu delta on whitened observations to weights on raw
ones, every lane at once) -> rollout_policy -> es_update -> obs_stats (the batch merged into the running statistics).
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
    ap.add_argument("--update", default="torch", choices=["torch", "device"], help="device: es_perturb / es_update of libos2r_es.so")
    ap.add_argument("--populations", type=int, default=1, help="policies searched at once (--update device)")
    ap.add_argument("--top", type=int, default=0, help="directions kept per population, 0: all (--update device)")
    ap.add_argument("--normalize", action="store_true", help="ARS V2: running observation whitening (--update device)")
    args = ap.parse_args()
    if args.update == "device":
        return device(args)
    if args.populations != 1 or args.top != 0 or args.normalize:
        raise SystemExit("--populations, --top and --normalize need --update device")
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


def device(args):
    """The same search with both ends of the iteration on the device, for M populations at once."""
    M = args.populations
    S = args.envs // (2 * M) if M >= 1 else 0
    if S < 1:
        raise SystemExit("--envs must be at least 2 x --populations")
    N = 2 * S * M
    env = g.make("Monopod-balance-v1", num_envs=N, seed=args.seed, dtype=args.dtype)
    env.reset()
    sim = env.sim
    dev, dt, D, i32 = sim.device, sim.dtype, sim.D, torch.int32
    theta, theta_new = (torch.zeros(M, 2, D + 1, dtype=dt, device=dev) for _ in range(2))
    weights = torch.empty(N, 2, D + 1, dtype=dt, device=dev)
    sigma_r = torch.empty(M, dtype=dt, device=dev)
    count, used, kept = (torch.empty(n, dtype=i32, device=dev) for n in (M, M, S * M))
    score = torch.empty(S * M, dtype=dt, device=dev) if 0 < args.top < S else None
    if args.normalize:                                                             # two running states, swapped every iteration
        state, state_new = ((torch.zeros(M, dtype=torch.int64, device=dev), torch.zeros(M, D, dtype=dt, device=dev),
                             torch.zeros(M, D, dtype=dt, device=dev)) for _ in range(2))
        folded = torch.empty_like(weights)
        lane_sum, lane_count = torch.empty(2 * D, N, dtype=dt, device=dev), torch.empty(2, N, dtype=i32, device=dev)
    print(f"ARS{' V2' if args.normalize else ''} on Monopod-balance-v1: {M} populations x {S} directions x 2 = {N} environments, top {args.top or S}, horizon {args.horizon}, "
          f"obs dim {D}", flush=True)
    t0 = time.time()
    for it in range(args.iters):
        obs0 = sim.reset()
        sim.es_perturb_into(theta, weights, directions=S, nu=args.noise, generation=it)
        if args.normalize:
            sim.norm_fold_into(weights, state, folded, lanes=N)
            ret, length, outs = sim.rollout_policy(args.horizon, folded, first_episode=True, want_outputs=True)
        else:
            ret, length, _ = sim.rollout_policy(args.horizon, weights, first_episode=True)
        sim.es_update_into(ret, theta, theta_new, sigma_r, count, used, kept, directions=S, generation=it, step_size=args.step_size,
                           top=args.top, score=score)
        theta, theta_new = theta_new, theta
        if args.normalize:
            sim.obs_stats_into(outs[0], *state_new, lane_sum, lane_count, policies=M, obs0=obs0, length=length, state=state)
            state, state_new = state_new, state
        per_pop = ret.view(2 * S, M).mean(0)                                       # (for the line below only)
        print(f"iteration {it}: mean return best population {float(per_pop.max()):8.2f}  median {float(per_pop.median()):8.2f}  "
              f"best lane {float(ret.max()):6.1f}  mean episode length {float(length.to(torch.float64).mean()):6.1f}  "
              f"directions used {int(used.min())}..{int(used.max())}", flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    steps = args.iters * N * args.horizon
    print(f"{steps / 1e6:.1f} M env-steps in {wall:.2f} s ({steps / wall / 1e6:.1f} M env-steps/s incl. resets and updates)")
    env.close()


if __name__ == "__main__":
    main()
