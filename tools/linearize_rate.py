#!/usr/bin/env python3
"""Time per call of os2r_linearize (include/os2r.h) against the composed path it replaces, at C4 in f64.

  python tools/linearize_rate.py [--envs 64 4096 65536] [--reps 5] [--out profiles/linearize_rate.txt]

C4 is bench.py's default workload: free_hip environments (five joints, P = 2 (2 nq + 2) + 1 = 25 evaluation points), ground
contact, per-env domain randomisation.  A handle of N environments is rolled a few hundred env-steps so that robots lie on
the ground and the solver state is populated.  Cases, each timed with HIP events on the current stream around a window of
calls, the cases alternating within one process --reps times after one untimed round (median, min and max per case):
  fused        sim.linearize_into(actions, eps, next, A, B): one launch, N x 25 lanes, caller-owned outputs
  composed     the path of tests/test_gpu_linearize.py with everything kept on the device: fork.copy_envs_from(sim, index) into a
               handle of 25 N environments, get_state / get_solver_state, the perturbations in torch, set_state,
               set_solver_state, step, get_state, the quotients in torch -- the fork handle and the index are made once,
               outside the window; the events bracket the host's share (two synchronisations per call) too
  step         fork.step(actions) alone, 25 N lanes with epilogue: the scale of the physics both paths run
A window holds as many calls as fit about 0.3 s of the step case (at least 3).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_sim(n, seed, auto_reset):
    import gym_os2r_amd as g
    from gym_os2r_amd import abi, rewards
    from gym_os2r_amd.sim import HipSim
    from gym_os2r_amd.tasks.monopod import MonopodTask
    task = MonopodTask(1000, task_mode="free_hip", reward_class=rewards.BalancingV1, reset_positions=["stand"])
    task.create_spaces()
    model = g.get_model(g.config.SettingsConfig().get_config("task_modes/free_hip/model"))
    spec = task.kernel_spec(model, reset_mode=abi.RESET_RANDOM, randomize_params=True, max_episode_steps=100_000)
    return HipSim(abi.config_struct(model, spec, num_envs=n, seed=seed, contact=True, dtype=abi.F64, auto_reset=auto_reset))


def window(torch, fn, calls):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls      # us per call


def measure(torch, n, reps, emit):
    sim = make_sim(n, 1, True)
    sim.bench_steps(300)
    nq = sim.nq
    n2, P = 2 * nq, 2 * (2 * nq + 2) + 1
    fork = make_sim(P * n, 2, False)
    dev, dt = sim.device, sim.dtype
    eps = float(torch.finfo(dt).eps) ** (1.0 / 3.0)
    h = torch.tensor(eps, dtype=dt, device=dev)
    actions = torch.rand(n, 2, dtype=dt, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * 2 - 1
    index = torch.arange(n, dtype=torch.int32, device=dev).repeat(P)
    nxt, A, B = (torch.empty(*s, dtype=dt, device=dev) for s in ((n2, n), (n2, n2, n), (n2, 2, n)))

    def fused():
        sim.linearize_into(actions, eps, nxt, A, B)

    def composed():
        fork.copy_envs_from(sim, index)
        q, qd = fork.get_state()
        lam, flags = fork.get_solver_state()
        act = actions.repeat(P, 1)
        x = torch.cat([q, qd])                                           # [2nq, P n]
        blocks = x.view(n2, P, n)
        for c in range(n2):
            blocks[c, 2 * c] += h
            blocks[c, 2 * c + 1] -= h
        ab = act.view(P, n, 2)
        for j in range(2):
            c = n2 + j
            ab[2 * c, :, j] = (ab[2 * c, :, j] + h).clamp(max=1.0)
            ab[2 * c + 1, :, j] = (ab[2 * c + 1, :, j] - h).clamp(min=-1.0)
        fork.set_state(x[:nq], x[nq:])
        fork.set_solver_state(lam, flags)
        fork.step(act, want_terminal=False)
        f = torch.cat(fork.get_state()).view(n2, P, n)
        xin = torch.cat([blocks, ab.permute(2, 0, 1)])                   # [2nq + 2, P, n]
        hi, lo = slice(0, 2 * (n2 + 2), 2), slice(1, 2 * (n2 + 2), 2)
        cols = torch.arange(n2 + 2, device=dev)
        den = xin[cols, 2 * cols] - xin[cols, 2 * cols + 1]              # [2nq + 2, n]
        return f[:, -1], (f[:, hi] - f[:, lo]) / den[None]

    act_fork = actions.repeat(P, 1)

    def step():
        fork.step(act_fork, want_terminal=False)

    # the two paths agree before anything is timed (the tests assert it bit for bit at their sizes)
    fused()
    c_next, c_J = composed()
    torch.cuda.synchronize()
    same = torch.equal(c_next, nxt) and torch.equal(c_J[:, :n2], A) and torch.equal(c_J[:, n2:], B)
    calls = max(3, min(200, int(0.3e6 / max(window(torch, step, 3), 1.0))))
    cases = [("fused os2r_linearize", fused), ("composed fork/perturb/step/quotients", composed), (f"step of {P} N lanes alone", step)]
    times = {name: [] for name, _ in cases}
    for rep in range(reps + 1):                      # round 0 is the warm-up of every case
        for name, fn in cases:
            us = window(torch, fn, calls)
            if rep:
                times[name].append(us)
    emit(f"{n} envs ({P * n} lanes), f64, {calls} calls per window, {reps} alternating windows; fused == composed bit for bit: {same}")
    med, spread = {}, {}
    for name, _ in cases:
        t = sorted(times[name])
        med[name], spread[name] = t[len(t) // 2], t[-1] - t[0]
        emit(f"  {name:<40} {med[name]:12.1f} us per call  (min {t[0]:.1f}, max {t[-1]:.1f})")
    f_, c_, s_ = (med[name] for name, _ in cases)
    emit(f"  composed / fused {c_ / f_:8.2f} x     fused / step alone {f_ / s_:6.2f} x")
    sim.close(); fork.close()
    return f_ <= c_ + max(spread.values()), same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[64, 4096, 65536])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("linearize_rate: no GPU visible; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"os2r_linearize, time per call over HIP events; {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    ok = True
    for n in args.envs:
        holds, same = measure(torch, n, args.reps, emit)
        ok = ok and holds and same
    emit("condition (fused no slower than the composed path beyond the spread of the repeats, at every size): " + ("holds" if ok else "DOES NOT HOLD"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
