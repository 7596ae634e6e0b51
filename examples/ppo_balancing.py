#!/usr/bin/env python3
"""PPO (Schulman et al. 2017) with GAE(lambda) for a linear-Gaussian policy and a linear value function on Monopod-balance-v1,
entirely on the GPU: one batch pays for several updates.

  python examples/ppo_balancing.py [--envs 8192] [--iters 20] [--horizon 500] [--epochs 4] [--clip 0.2] [--kl-stop 0.02]
                                   [--step-size 0.05] [--sigma 0.2] [--gamma 0.99] [--lam 0.95] [--ridge 1e-3] [--normalize]

The policy is a = clip(theta . [o; 1] + sigma * eps) as in examples/actor_critic_balancing.py, the critic V(o) = w . [o; 1].  One
iteration is a chain of calls on the arrays the rollout returned, as they are, with no tensor reshuffled in between:

  reset -> rollout_policy -> gae -> (advantage normalisation, one torch line) -> E x (ppo_gradient; theta += step grad / steps)
        -> value_fit

ppo_gradient (include/os2r_ppo.h) evaluates the gradient of the clipped surrogate at the current theta on the batch that
theta_old sampled: in the first epoch the two are equal, every ratio is 1 and the gradient is the score-function gradient of
policy_gradient bit for bit; from the second on every step carries its importance ratio, and a step whose ratio has left
[1 - clip, 1 + clip] in the direction its advantage pushes adds nothing.  Its stats give the k3 estimate of the KL divergence
between theta_old and theta, (dev - logr) / steps; with --kl-stop the epochs end when it passes the value.  Nothing leaves the
device but the numbers printed.

--normalize: theta acts on whitened observations, (x - mean) / std with the running mean and deviation of every batch so far
(libos2r_norm.so, include/os2r_norm.h).  The rollout and ppo_gradient take norm_fold(theta), weights on raw observations, and
norm_unfold takes every gradient back to theta; obs_stats merges the batch into the statistics behind the last epoch, so the
statistics are the same for theta and theta_old.  The critic stays on raw observations.
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
    ap.add_argument("--horizon", type=int, default=500, help="env-steps per rollout (an environment's first episode counts)")
    ap.add_argument("--epochs", type=int, default=4, help="updates per batch")
    ap.add_argument("--clip", type=float, default=0.2, help="the clip of the importance ratio, in (0, 1)")
    ap.add_argument("--kl-stop", type=float, default=None, help="stop the epochs of a policy when its KL estimate passes this value")
    ap.add_argument("--step-size", type=float, default=0.05)
    ap.add_argument("--sigma", type=float, default=0.2, help="standard deviation of the exploration noise on both actions")
    ap.add_argument("--gamma", type=float, default=0.99, help="the discount")
    ap.add_argument("--lam", type=float, default=0.95, help="the lambda of the advantage estimate")
    ap.add_argument("--ridge", type=float, default=1e-3, help="the ridge of the value fit, towards the previous weights")
    ap.add_argument("--normalize", action="store_true", help="running observation whitening of the policy's input")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    args = ap.parse_args()
    N, H = args.envs, args.horizon
    env = g.make("Monopod-balance-v1", num_envs=N, seed=args.seed, dtype=args.dtype)
    env.reset()
    sim = env.sim
    dev, dt, D = sim.device, sim.dtype, sim.D
    theta = torch.zeros(2, D + 1, 1, dtype=dt, device=dev).permute(2, 0, 1)  # [P, 2, D+1] over the kernel's [2, D+1, P], one policy
    sigma = torch.full((2,), args.sigma, dtype=dt, device=dev)
    w = torch.zeros(1, D + 1, dtype=dt, device=dev)                       # [P, D+1]
    state = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, D, dtype=dt, device=dev), torch.zeros(1, D, dtype=dt, device=dev))
    fold = (lambda t: sim.norm_fold(t, state)) if args.normalize else (lambda t: t)
    print(f"PPO on Monopod-balance-v1: {N} environments, horizon {H}, obs dim {D}, sigma {args.sigma}, gamma {args.gamma}, lambda {args.lam}, "
          f"{args.epochs} epochs, clip {args.clip}, kl-stop {args.kl_stop}, ridge {args.ridge}{', whitened observations' if args.normalize else ''}", flush=True)
    t0 = time.time()
    for it in range(args.iters):
        obs0 = sim.reset()
        ret, length, (O, R, Dn, T, _), (A, E) = sim.rollout_policy(H, fold(theta)[0], sigma=sigma, salt=it, first_episode=True, want_outputs=True,
                                                                   want_terminal=True, want_actions=True, want_noise=True)
        adv, lam_ret, _ = sim.gae(O, R, Dn, w, obs0=obs0, term_obs=T, length=length, gamma=args.gamma, lam=args.lam)
        n = length.sum().clamp_min(1).to(dt)                              # (adv is 0 behind an episode's end: the sums run over the counted steps)
        adv = (adv - adv.sum() / n) / (adv.square().sum() / n - (adv.sum() / n) ** 2).clamp_min(1e-16).sqrt()
        theta_old = theta
        active = torch.ones(1, dtype=torch.bool, device=dev)             # [P]: the policies whose epochs go on
        epochs, gated_share, kl = 0, 0.0, 0.0
        for _ in range(args.epochs):
            grad, stats, steps, clipped, gated, valid, _, _, _ = sim.ppo_gradient(O, E, sigma, fold(theta), fold(theta_old), adv, clip=args.clip,
                                                                                obs0=obs0, actions=A, length=length)
            if args.normalize:
                grad = sim.norm_unfold(grad, state)
            count = steps.clamp_min(1).to(dt)
            kl_p = (stats[:, 1] - stats[:, 2]) / count                    # the k3 estimate, per policy
            gated_share, kl = float(gated.sum()) / float(count.sum()), float(kl_p.mean())
            if args.kl_stop is not None:
                active = active & (kl_p <= args.kl_stop)
            if not bool(active.any()):
                break
            theta = theta + args.step_size * active.to(dt).view(-1, 1, 1) * grad / count.view(-1, 1, 1)
            epochs += 1
        if args.normalize:
            state = sim.obs_stats(O, obs0=obs0, length=length, state=state)[0]
        w, failed, _, _ = sim.value_fit(O, lam_ret, obs0=obs0, length=length, prev=w, ridge=args.ridge)
        print(f"iteration {it}: mean return {float(ret.mean()):8.2f}  epochs {epochs}  gated {100 * gated_share:5.1f} %  KL {kl:.5f}"
              + ("  (the value fit failed: w kept)" if int(failed[0]) else ""), flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    total = args.iters * N * H
    print(f"{total / 1e6:.1f} M env-steps in {wall:.2f} s ({total / wall / 1e6:.1f} M env-steps/s incl. resets and updates)")
    env.close()


if __name__ == "__main__":
    main()
