#!/usr/bin/env python3
"""Natural policy gradient with a trust region (Kakade 2002; the step of TRPO, Schulman et al. 2015, in closed form) for a
linear-Gaussian policy and a linear value function on Monopod-balance-v1, entirely on the GPU.

  python examples/npg_balancing.py [--envs 8192] [--iters 20] [--horizon 500] [--kl 0.01] [--damping 1e-3] [--sigma 0.2]
                                   [--gamma 0.99] [--lam 0.95] [--ridge 1e-3]

The policy is a = clip(theta . [o; 1] + sigma * eps) as in examples/reinforce_balancing.py, the critic V(o) = w . [o; 1].  One
iteration is five calls on the arrays the rollout returned, as they are, with no tensor reshuffled in between:

  reset -> rollout_policy -> gae -> policy_gradient -> natural_step -> theta += step -> value_fit

natural_step (include/os2r_npg.h) turns the plain gradient into a step whose mean KL divergence from the policy that sampled
the batch is --kl nats: the Fisher matrix of each action component from the observations of the steps on which its clip did not
bind, a Cholesky solve, and the scaling sqrt(2 kl / (g . d)).  There is no step size to tune against the scale of the advantages
or the width of the exploration; beta, the factor on the natural-gradient direction, is printed with the flags of a failed
solve.  Nothing leaves the device but the numbers printed.
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
    ap.add_argument("--kl", type=float, default=0.01, help="the mean KL divergence of one update, in nats")
    ap.add_argument("--damping", type=float, default=1e-3, help="added to the diagonal of the Fisher matrices")
    ap.add_argument("--sigma", type=float, default=0.2, help="standard deviation of the exploration noise on both actions")
    ap.add_argument("--gamma", type=float, default=0.99, help="the discount")
    ap.add_argument("--lam", type=float, default=0.95, help="the lambda of the advantage estimate")
    ap.add_argument("--ridge", type=float, default=1e-3, help="the ridge of the value fit, towards the previous weights")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    args = ap.parse_args()
    N, H = args.envs, args.horizon
    env = g.make("Monopod-balance-v1", num_envs=N, seed=args.seed, dtype=args.dtype)
    env.reset()
    sim = env.sim
    dev, dt, D = sim.device, sim.dtype, sim.D
    theta = torch.zeros(1, 2, D + 1, dtype=dt, device=dev)                # [P, 2, D+1], one policy
    sigma = torch.full((2,), args.sigma, dtype=dt, device=dev)
    w = torch.zeros(1, D + 1, dtype=dt, device=dev)                       # [P, D+1]
    print(f"natural policy gradient on Monopod-balance-v1: {N} environments, horizon {H}, obs dim {D}, sigma {args.sigma}, kl {args.kl}, "
          f"damping {args.damping}, gamma {args.gamma}, lambda {args.lam}", flush=True)
    t0 = time.time()
    for it in range(args.iters):
        obs0 = sim.reset()
        ret, length, (O, R, Dn, T, _), (A, E) = sim.rollout_policy(H, theta[0], sigma=sigma, salt=it, first_episode=True, want_outputs=True,
                                                                   want_terminal=True, want_actions=True, want_noise=True)
        adv, lam_ret, _ = sim.gae(O, R, Dn, w, obs0=obs0, term_obs=T, length=length, gamma=args.gamma, lam=args.lam)
        grad, steps, clipped, valid, _, _, _ = sim.policy_gradient(O, E, sigma, obs0=obs0, actions=A, length=length, rewards=adv, done=Dn,
                                                                   gamma=0.0)
        step, _, beta, quad, failed, _, opened, _, _ = sim.natural_step(O, sigma, grad, obs0=obs0, actions=A, length=length,
                                                                        damping=args.damping, kl=args.kl)
        theta = theta + step
        w, fit_failed, _, _ = sim.value_fit(O, lam_ret, obs0=obs0, length=length, prev=w, ridge=args.ridge)
        mean_len = float(steps[0]) / max(int(valid[0]), 1)
        print(f"iteration {it}: mean return {float(ret.mean()):8.2f}  mean episode length {mean_len:6.1f}  beta {float(beta[0]):9.3e}  "
              f"failed {failed[0].tolist()}  open steps {opened[0].tolist()} of {int(steps[0])}"
              + ("  (the value fit failed: w kept)" if int(fit_failed[0]) else ""), flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    total = args.iters * N * H
    print(f"{total / 1e6:.1f} M env-steps in {wall:.2f} s ({total / wall / 1e6:.1f} M env-steps/s incl. resets and updates)")
    env.close()


if __name__ == "__main__":
    main()
