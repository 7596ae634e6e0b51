#!/usr/bin/env python3
"""System identification of the monopod on the GPU: which damping, friction and gravity make the simulator reproduce a log?

  python examples/sysid_monopod.py [--mode fixed_hip] [--actions random|pd] [--segments 64] [--steps 10] [--iters 8] [--noise 0] [--hold 5]

A "real" handle of one environment holds hidden parameters (the damping and the Coulomb friction of hip and knee, and gravity)
and logs one trajectory of segments x steps env-steps, under random actions, each held for --hold steps, or (--actions pd) under
a PD law that drives hip and knee along slow sinusoids about the reset pose, its torques clamped to [-1, 1]; the identification
replays the logged actions open loop either way.  The log is cut into
M = segments pieces of K = steps: their start states, their actions [K, M, 2] and their measured observations [K, M, D]
(+ N(0, noise) with --noise).  At the start of every piece the real handle's own state is set again, so that its contact solver
starts the piece cold, as the lanes of the identification do.

The identification runs on a second handle of N = (2 P + 1) M environments (libos2r_sysid.so, include/os2r_sysid.h): lane
s M + m replays piece m with the nominal parameters (s = 0), with parameter p raised (s = 1 + p) or lowered (s = 1 + P + p).
Every iteration is sysid_perturb -> set_params x 5 -> set_state -> rollout(K, actions) -> sysid_update, with no tensor
reshuffled in between: the start states and the actions are tiled over the 2 P + 1 lane groups once, before the loop, and the
blocks of the packed parameter array are what set_params takes.  sysid_update forms the Gauss-Newton system from the lanes'
observations, accepts or rejects the point, adapts the damping lam and writes the next point, all on the device; the loop is
stream-ordered but for the five set_params calls and set_state, which synchronise the host as they always do.  A rejected point
costs its 2 P perturbed lanes: the loop needs no host decision in exchange.  What is printed per iteration reads a few numbers
back and is no part of the loop.
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gym_os2r_amd as g
from gym_os2r_amd import abi, rewards, sysid
from gym_os2r_amd.sim import HipSim
from gym_os2r_amd.tasks import monopod_no_norm

# the identified parameters: (field, dof name or None), the hidden truth, the step, the bounds
PARAMS = ((abi.PARAM_DAMPING, "hip_joint", 0.02, 1e-3, 0.0, 0.1), (abi.PARAM_DAMPING, "knee_joint", 0.005, 1e-3, 0.0, 0.1),
          (abi.PARAM_FRICTION, "hip_joint", 0.004, 1e-4, 0.0, 0.05), (abi.PARAM_FRICTION, "knee_joint", 0.002, 1e-4, 0.0, 0.05),
          (abi.PARAM_GRAVITY, None, -9.6, 1e-2, -11.0, -9.0))


def handle(mode, num_envs, seed, contact):
    task = monopod_no_norm.MonopodTask(agent_rate=1000, task_mode=mode, reward_class=rewards.BalancingV1, reset_positions=["stand"])
    task.create_spaces()
    model = g.get_model(g.config.SettingsConfig().get_config(f"task_modes/{mode}/model"))
    spec = task.kernel_spec(model, reset_mode=abi.RESET_FIXED, randomize_params=False, max_episode_steps=0)
    return HipSim(abi.config_struct(model, spec, num_envs=num_envs, dtype=abi.F64, seed=seed, contact=contact, auto_reset=False)), model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="fixed_hip", help="task mode of the raw-observation monopod task")
    ap.add_argument("--contact", action="store_true", help="ground contact on (free_hip)")
    ap.add_argument("--segments", type=int, default=64, help="M: pieces the log is cut into")
    ap.add_argument("--steps", type=int, default=10, help="K: env-steps per piece")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--hold", type=int, default=5, help="env-steps a random action is held in the log")
    ap.add_argument("--actions", default="random", choices=["random", "pd"], help="what drives the real robot while it is logged")
    ap.add_argument("--kp", type=float, default=2.0, help="--actions pd: action per radian of joint error")
    ap.add_argument("--kd", type=float, default=0.05, help="--actions pd: action per radian / s of joint velocity")
    ap.add_argument("--noise", type=float, default=0.0, help="standard deviation of the measurement noise")
    ap.add_argument("--lam0", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    M, K = args.segments, args.steps
    real, model = handle(args.mode, 1, args.seed, args.contact)
    nq, dev, dt = real.nq, real.device, real.dtype
    names = model["dof_names"]
    sel = [(f, 0 if dof is None else names.index(dof)) for f, dof, *_ in PARAMS]
    truth = torch.tensor([[p[2] for p in PARAMS]], dtype=dt, device=dev)
    h, lo, hi = [p[3] for p in PARAMS], [p[4] for p in PARAMS], [p[5] for p in PARAMS]
    P = len(sel)
    S = 2 * P + 1

    # the log: one trajectory of M K steps on the real handle, which holds the truth
    real.reset()
    nominal = sysid.pack({f: real.get_params(f) for f in sysid.FIELDS}, nq)              # [4 nq + 1, 1]: what the simulator believes
    hidden = nominal.clone()
    for (f, i), v in zip(sel, truth[0]):
        hidden[sysid.row(nq, f, i)] = v
    for f in sysid.FIELDS:
        real.set_params(f, sysid.field_view(hidden, nq, f))
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    drawn = torch.rand((M * K + args.hold - 1) // args.hold, 2, dtype=dt, device=dev, generator=gen) * 2 - 1
    log_actions = drawn.repeat_interleave(args.hold, 0)[:M * K].reshape(M, K, 1, 2)
    q0, qd0, meas = [], [], []
    joints = [names.index("hip_joint"), names.index("knee_joint")]           # the two actuated dofs, in the order of an action
    rest = real.get_state()[0][joints, 0]
    amplitude = torch.tensor([0.4, 0.6], dtype=dt, device=dev)
    for m in range(M):
        q, qd = real.get_state()
        real.set_state(q, qd)                                  # (its own state: the contact solver starts the piece cold)
        q0.append(q)
        qd0.append(qd)
        if args.actions == "random":
            meas.append(real.rollout(K, log_actions[m])[0])
            continue
        piece = []
        for k in range(K):                                     # the PD law needs the state of every step: a step at a time
            q, qd = real.get_state()
            phase = 2 * math.pi * (m * K + k) / 200.0
            target = rest + amplitude * torch.tensor([math.sin(phase), math.sin(1.7 * phase)], dtype=dt, device=dev)
            log_actions[m, k, 0] = (args.kp * (target - q[joints, 0]) - args.kd * qd[joints, 0]).clamp(-1.0, 1.0)
            piece.append(real.step(log_actions[m, k])[0])
        meas.append(torch.stack(piece))
    real.close()
    meas = torch.cat(meas, 1).contiguous()                     # [K, M, D]
    if args.noise > 0:
        meas = meas + args.noise * torch.randn(meas.shape, dtype=dt, device=dev, generator=gen)
    actions = log_actions[:, :, 0].transpose(0, 1)             # [K, M, 2]

    # the identification: N lanes, everything tiled once
    sim, _ = handle(args.mode, S * M, args.seed, args.contact)
    D = sim.D
    q0, qd0 = torch.cat(q0, 1).repeat(1, S).contiguous(), torch.cat(qd0, 1).repeat(1, S).contiguous()
    actions = actions.repeat(1, S, 1).contiguous()
    base = nominal.expand(-1, M).contiguous()
    prec = torch.full((D,), 1.0 if args.noise <= 0 else 1.0 / args.noise ** 2, dtype=dt, device=dev)
    theta = torch.tensor([[nominal[sysid.row(nq, f, i), 0].item() for f, i in sel]], dtype=dt, device=dev)
    state = sim.sysid_init(theta, args.lam0)
    state_new = tuple(torch.empty_like(t) for t in state)                                # two state sets, swapped every iteration
    theta_next = torch.empty_like(theta)
    E = P * (P + 1) // 2 + P + 1
    sums, counts = torch.empty(E * (M + 1), dtype=dt, device=dev), torch.empty(M + 1, dtype=torch.int32, device=dev)
    cost, valid = torch.empty(1, dtype=dt, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    accepted = torch.empty(1, dtype=torch.uint8, device=dev)
    params = torch.empty(sysid.rows(nq), S * M, dtype=dt, device=dev)
    constants = sysid.constants()
    obs, rew, done = (torch.empty(K, S * M, D, dtype=dt, device=dev), torch.empty(K, S * M, dtype=dt, device=dev),
                      torch.empty(K, S * M, dtype=torch.uint8, device=dev))
    steps = dict(h=h, lo=lo, hi=hi)
    print(f"identifying {P} parameters of the {args.mode} monopod from {M} pieces of {K} steps logged under {args.actions} actions: {S * M} lanes, "
          f"obs dim {D}, noise {args.noise}", flush=True)
    print(f"start {[f'{v:.5g}' for v in theta[0].tolist()]}  truth {[f'{v:.5g}' for v in truth[0].tolist()]}", flush=True)
    torch.cuda.synchronize()
    t0 = time.time()
    for it in range(args.iters):
        sim.sysid_perturb_into(theta, base, params, sel=sel, **steps)
        for f in sysid.FIELDS:
            sim.set_params(f, sysid.field_view(params, nq, f))
        sim.set_state(q0, qd0)
        sim.rollout_into(K, actions, obs, rew, done)
        sim.sysid_update_into(obs, meas, prec, theta, state, state_new, theta_next, sums, counts, constants=constants, done=done, cost=cost,
                              valid=valid, accepted=accepted, **steps)
        state, state_new = state_new, state
        theta, theta_next = theta_next, theta
        err = ((state[0] - truth).abs() / truth.abs()).max()
        print(f"iteration {it}: cost {float(cost[0]):.6e}  best {float(state[1][0]):.6e}  lam {float(state[4][0]):.3e}  "
              f"{'accepted' if int(accepted[0]) else 'rejected'}  valid {int(valid[0])} of {M}  status {int(state[5][0])}  "
              f"largest relative parameter error {float(err):.3e}", flush=True)
    torch.cuda.synchronize()
    wall = time.time() - t0
    print(f"identified {[f'{v:.6g}' for v in state[0][0].tolist()]}")
    print(f"relative errors {[f'{v:.2e}' for v in ((state[0] - truth).abs() / truth.abs())[0].tolist()]}")
    print(f"{args.iters} iterations in {wall:.3f} s: {wall / args.iters * 1e3:.2f} ms per iteration, printing included "
          f"({args.iters * S * M * K / wall / 1e6:.2f} M env-steps/s)")
    sim.close()


if __name__ == "__main__":
    main()
