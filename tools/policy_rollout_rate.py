#!/usr/bin/env python3
"""Closed-loop rate of os2r_rollout_policy (include/os2r.h) against the open-loop rollout and a Python closed loop, at C4.

  python tools/policy_rollout_rate.py [--envs 65536] [--dtype f64] [--preroll 1000] [--steps 200] [--reps 3] [--out FILE.json]
  python tools/policy_rollout_rate.py --only policy10      # just the K = 10 shared-weight policy rollouts (for rocprofv3)

C4 is bench.py's default workload: 65 536 free_hip environments, ground contact, per-env domain randomisation, rolled into
the stationary regime (--preroll device-action env-steps) before anything is timed.  Every line starts from the same
checkpoint of that regime and times --steps env-steps of the whole batch with HIP events on the current stream (median of
--reps windows, after one untimed warm-up call).  Lines:
  rollout        os2r_rollout, device-drawn actions, obs / reward / done written, K env-steps per launch
  policy         os2r_rollout_policy, shared [2, D+1] or per-env [N, 2, D+1] weights, per-step outputs off (returns and
                 lengths only) or on (obs / reward / done), K env-steps per call
  replayed       os2r_rollout with the actions the policy took in that window (recomputed in torch from its observations,
                 bit for bit): the open-loop launch on the same trajectory -- the cost of an env-step depends on the regime the
                 actions drive the robots into (contacts, solver rounds), so this is the line the policy is compared with
  policy noisy   os2r_rollout_policy_noisy, shared weights and shared sigma = 0.3 (Gaussian exploration noise drawn in the kernel),
                 per-step outputs off, or all on (obs / reward / done / applied actions / noise); its `replayed` line is
                 os2r_rollout with the actions it reported -- noise drives the robots into another regime than the
                 deterministic policy does, so the noisy lines are compared with that one, not with `policy`
  python loop    step_into per env-step, the policy a torch.nn.Linear(D, 2) (the shared weights) + clamp on the returned
                 observation
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_sim(args):
    import gym_os2r_amd as g
    from gym_os2r_amd import abi, rewards
    from gym_os2r_amd.sim import HipSim
    from gym_os2r_amd.tasks.monopod import MonopodTask
    task = MonopodTask(1000, task_mode="free_hip", reward_class=rewards.BalancingV1, reset_positions=["stand"])
    task.create_spaces()
    model = g.get_model(g.config.SettingsConfig().get_config("task_modes/free_hip/model"))
    spec = task.kernel_spec(model, reset_mode=abi.RESET_RANDOM, randomize_params=True, max_episode_steps=100_000)
    cfg = abi.config_struct(model, spec, num_envs=args.envs, seed=args.seed, contact=True,
                            dtype=abi.F64 if args.dtype == "f64" else abi.F32)
    return HipSim(cfg)


def timed(torch, sim, ck, fn, calls, reps):
    """Median GPU milliseconds of fn(0) ... fn(calls - 1), each window started from checkpoint `ck` after one warm-up call."""
    out = []
    for _ in range(reps):
        sim.restore(ck)
        fn(0)
        sim.restore(ck)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(i)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    out.sort()
    return out[len(out) // 2]


def policy_actions(torch, obs, W):
    """The kernel's clip policy in torch, in the documented order (include/os2r.h): bit for bit its actions."""
    D = obs.shape[1]
    Wn = W.unsqueeze(0).expand(obs.shape[0], 2, D + 1) if W.dim() == 2 else W
    z = Wn[:, :, D].clone()
    for d in range(D):
        z = z + Wn[:, :, d] * obs[:, d:d + 1]
    return torch.clamp(z, -1.0, 1.0)


def recorded_actions(torch, sim, ck, obs0, W, K, calls):
    """[calls, K, N, 2]: the actions os2r_rollout_policy takes over `calls` calls of K env-steps from checkpoint `ck`."""
    sim.restore(ck)
    acts, prev = [], obs0
    for _ in range(calls):
        _, _, (O, _, _, _, _) = sim.rollout_policy(K, W, want_outputs=True)
        acts.append(torch.stack([policy_actions(torch, prev if k == 0 else O[k - 1], W) for k in range(K)]))
        prev = O[K - 1]
    return torch.stack(acts)


def recorded_noisy_actions(torch, sim, ck, W, sigma, K, calls):
    """[calls, K, N, 2]: the actions os2r_rollout_policy_noisy reports over `calls` calls of K env-steps from checkpoint `ck`."""
    sim.restore(ck)
    return torch.stack([sim.rollout_policy(K, W, sigma=sigma, want_actions=True)[3][0] for _ in range(calls)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--preroll", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=200, help="env-steps per timed window (a multiple of 50)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=["policy10"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    sim = make_sim(args)
    N, D, dt = sim.N, sim.D, sim.dtype
    sim.bench_steps(max(args.preroll, 1))
    ck = sim.checkpoint()
    obs0 = sim.reset(torch.zeros(N, dtype=torch.uint8, device=sim.device))   # (mask all zero: the current observation, nothing reset)
    g = torch.Generator(device=sim.device).manual_seed(1)
    w_shared = 0.3 * torch.randn(2, D + 1, dtype=dt, device=sim.device, generator=g)
    w_env = 0.3 * torch.randn(N, 2, D + 1, dtype=dt, device=sim.device, generator=g)
    sigma = torch.full((2,), 0.3, dtype=dt, device=sim.device)

    if args.only == "policy10":
        for _ in range(1 + args.steps // 10):
            sim.rollout_policy(10, w_shared)
        torch.cuda.synchronize()
        print(f"policy rollouts done: {N} envs, K = 10, {1 + args.steps // 10} calls")
        return

    rows = []

    def row(name, K, ms, steps):
        rate = N * steps / (ms * 1e-3) / 1e6
        rows.append({"line": name, "K": K, "M_env_steps_per_s": rate, "us_per_env_step": ms * 1e3 / steps})
        print(f"{name:<46} K={K:<3} {rate:8.1f} M env-steps/s   {ms * 1e3 / steps:7.1f} us per env-step", flush=True)

    for K in (10, 50):
        calls = args.steps // K
        obs, rew = torch.empty(K, N, D, dtype=dt, device=sim.device), torch.empty(K, N, dtype=dt, device=sim.device)
        done = torch.empty(K, N, dtype=torch.uint8, device=sim.device)
        row("rollout (device actions)", K, timed(torch, sim, ck, lambda i: sim.rollout_into(K, None, obs, rew, done), calls, args.reps),
            calls * K)
        for wname, w in (("shared", w_shared), ("per-env", w_env)):
            acts = recorded_actions(torch, sim, ck, obs0, w, K, calls)
            row(f"rollout, replayed {wname} policy", K,
                timed(torch, sim, ck, lambda i: sim.rollout_into(K, acts[i], obs, rew, done), calls, args.reps), calls * K)
            del acts
            row(f"rollout_policy {wname}, outputs off", K,
                timed(torch, sim, ck, lambda i: sim.rollout_policy(K, w), calls, args.reps), calls * K)
            row(f"rollout_policy {wname}, outputs on", K,
                timed(torch, sim, ck, lambda i: sim.rollout_policy(K, w, want_outputs=True), calls, args.reps), calls * K)
        acts = recorded_noisy_actions(torch, sim, ck, w_shared, sigma, K, calls)
        row("rollout, replayed noisy shared policy", K,
            timed(torch, sim, ck, lambda i: sim.rollout_into(K, acts[i], obs, rew, done), calls, args.reps), calls * K)
        del acts
        row("rollout_policy noisy shared, outputs off", K,
            timed(torch, sim, ck, lambda i: sim.rollout_policy(K, w_shared, sigma=sigma), calls, args.reps), calls * K)
        row("rollout_policy noisy shared, all outputs on", K,
            timed(torch, sim, ck, lambda i: sim.rollout_policy(K, w_shared, sigma=sigma, want_outputs=True, want_actions=True,
                                                               want_noise=True), calls, args.reps), calls * K)
        del obs, rew, done

    lin = torch.nn.Linear(D, 2).to(sim.device, dt)
    with torch.no_grad():
        lin.weight.copy_(w_shared[:, :D])
        lin.bias.copy_(w_shared[:, D])
    obs, rew = torch.empty(N, D, dtype=dt, device=sim.device), torch.empty(N, dtype=dt, device=sim.device)
    done = torch.empty(N, dtype=torch.uint8, device=sim.device)
    state = {}

    def py_loop(i):
        if i == 0:
            state["obs"] = obs0
        with torch.no_grad():
            for _ in range(50):
                a = lin(state["obs"]).clamp_(-1.0, 1.0)
                sim.step_into(a, obs, rew, done)
                state["obs"] = obs
    row("python loop (step_into + Linear, shared W)", 1, timed(torch, sim, ck, py_loop, args.steps // 50, args.reps), args.steps)

    res = {"workload": f"C4: {N} envs free_hip, ground contact, per-env domain randomisation, {args.dtype}",
           "preroll": args.preroll, "steps_per_window": args.steps, "reps": args.reps, "when": time.strftime("%Y-%m-%d"),
           "device": torch.cuda.get_device_name(sim.device), "rows": rows}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    sim.close()


if __name__ == "__main__":
    main()
