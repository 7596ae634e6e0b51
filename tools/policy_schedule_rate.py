#!/usr/bin/env python3
"""Rate of os2r_rollout_policy_scheduled (include/os2r.h) against os2r_rollout_policy of this build and of the parent commit's
build, at C4 in f64.

  python tools/policy_schedule_rate.py --parent-lib /path/to/parent/libos2r.so [--envs 65536] [--preroll 1000] [--steps 100]
                                       [--reps 7] [--out profiles/policy_schedule_rate.txt]

C4 is bench.py's default workload: 65 536 free_hip environments, ground contact, per-env domain randomisation, rolled into the
stationary regime (--preroll device-action env-steps) before anything is timed.  Every case starts from the same checkpoint of
that regime and times --steps env-steps of the whole batch in calls of K = 10 and K = 50 env-steps with HIP events on the current
stream, after one untimed warm-up call.  The cases ALTERNATE inside one process: repeat r runs every case once before repeat
r + 1 starts, in turns forwards and backwards, so a drift of the clock or of the machine hits all of them alike.  Every slot of
every table holds the same weight set as (a): all cases drive the robots along the same trajectory, and what differs is how the
weights are fetched.  The checkpoint's episode steps are set to e mod 97: on the episode clock the lanes of a wave sit at
different slots.
  (a0) rollout_policy, shared weights, the PARENT commit's library (--parent-lib; a second copy of the C-ABI in this process)
  (a)  rollout_policy, shared weights, this build
  (b)  rollout_schedule, window clock, shared table, T = K
  (c)  rollout_schedule, episode clock with wrap, shared table, T = K: the lanes of a wave sit at different slots
  (d)  rollout_schedule, episode clock with wrap, per-env tables, T = K
  (e)  the composed loop: per env-step the slot's weights in torch (Linear + clamp on the returned observation), then step_into
Two conditions, both against the spread of the parent's own repeats (max - min of (a0)): the median of (a) lies within that spread
of the median of (a0) -- the one-set path does not pay for the schedule --, and the median of (b) is no slower than the median of
(a) by more than that spread.  (c) to (e) are reported only.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_sim(args, parent_lib=None):
    import gym_os2r_amd as g
    from gym_os2r_amd import abi, rewards
    from gym_os2r_amd.sim import HipSim
    from gym_os2r_amd.tasks.monopod import MonopodTask
    task = MonopodTask(1000, task_mode="free_hip", reward_class=rewards.BalancingV1, reset_positions=["stand"])
    task.create_spaces()
    model = g.get_model(g.config.SettingsConfig().get_config("task_modes/free_hip/model"))
    spec = task.kernel_spec(model, reset_mode=abi.RESET_RANDOM, randomize_params=True, max_episode_steps=100_000)
    cfg = abi.config_struct(model, spec, num_envs=args.envs, seed=args.seed, contact=True, dtype=abi.F64)
    sim = HipSim(cfg)
    if parent_lib is not None:
        # the same handle class over the other library: its handle is made by that library's os2r_create
        sim.close()
        sim._lib = parent_lib
        rc = parent_lib.os2r_create(C.byref(cfg), C.byref(sim._h))
        if rc != abi.OK:
            raise RuntimeError(f"os2r_create of the parent library failed ({rc})")
    return sim


def load_parent(path):
    """The parent build's C-ABI next to this build's: the call signatures are those of the symbols both have."""
    from gym_os2r_amd import _lib
    ours, lib = _lib.load(), C.CDLL(path)
    for name in _lib.SYMBOLS:
        if hasattr(lib, name):
            getattr(lib, name).argtypes = getattr(ours, name).argtypes
            getattr(lib, name).restype = getattr(ours, name).restype
    return lib


def window_ms(torch, sim, ck, fn, calls):
    """GPU milliseconds of fn(0) ... fn(calls - 1) from checkpoint `ck`, after one warm-up call."""
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
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libos2r.so built from the parent commit")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--preroll", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=100, help="env-steps per timed window (a multiple of 50)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    sim = make_sim(args)
    old = make_sim(args, load_parent(args.parent_lib)) if args.parent_lib else None
    N, D, dt, dev = sim.N, sim.D, sim.dtype, sim.device
    sim.bench_steps(max(args.preroll, 1))
    ck = sim.checkpoint()
    ck["steps"] = (torch.arange(N, device=sim.device) % 97).to(torch.int32)
    obs0 = sim.reset(torch.zeros(N, dtype=torch.uint8, device=dev))      # (mask all zero: the current observation, nothing reset)
    g = torch.Generator(device=dev).manual_seed(1)
    w = 0.3 * torch.randn(2, D + 1, dtype=dt, device=dev, generator=g)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"C4: {N} envs free_hip, ground contact, per-env domain randomisation, f64; preroll {args.preroll}, {args.steps} env-steps per "
        f"window, {args.reps} alternating repeats; {torch.cuda.get_device_name(dev)}, {time.strftime('%Y-%m-%d')}")
    verdicts = []
    for K in (10, 50):
        calls = args.steps // K
        table = w.unsqueeze(0).repeat(K, 1, 1).contiguous()                # [K, 2, D+1]
        table_env = table.unsqueeze(0).repeat(N, 1, 1, 1)                  # [N, K, 2, D+1]
        slots0 = ck["steps"][:64].to(torch.int64) % K
        lin = torch.nn.Linear(D, 2).to(dev, dt)
        obs, rew = torch.empty(N, D, dtype=dt, device=dev), torch.empty(N, dtype=dt, device=dev)
        done = torch.empty(N, dtype=torch.uint8, device=dev)
        state = {}

        def composed(i):
            if i == 0:
                state["obs"] = obs0
            with torch.no_grad():
                for k in range(K):
                    lin.weight.copy_(table[k, :, :D])
                    lin.bias.copy_(table[k, :, D])
                    a = lin(state["obs"]).clamp_(-1.0, 1.0)
                    sim.step_into(a, obs, rew, done)
                    state["obs"] = obs

        cases = []
        if old is not None:
            cases.append(("(a0) rollout_policy shared, parent build", old, lambda i: old.rollout_policy(K, w)))
        cases += [("(a)  rollout_policy shared, this build", sim, lambda i: sim.rollout_policy(K, w)),
                  ("(b)  rollout_schedule window clock, shared", sim, lambda i: sim.rollout_schedule(K, table)),
                  ("(c)  rollout_schedule episode clock, shared", sim, lambda i: sim.rollout_schedule(K, table, clock="episode", wrap=True)),
                  ("(d)  rollout_schedule episode clock, per-env", sim,
                   lambda i: sim.rollout_schedule(K, table_env, clock="episode", wrap=True)),
                  ("(e)  composed loop: torch policy -> step", sim, composed)]
        ms = {name: [] for name, _, _ in cases}
        for r in range(args.reps):
            for name, handle, fn in (cases if r % 2 == 0 else cases[::-1]):      # (no case always runs behind the same one)
                ms[name].append(window_ms(torch, handle, ck, fn, calls))
        say(f"K = {K}: T = {K}, {len(set(slots0.tolist()))} different slots among the 64 lanes of the first wave on the episode clock")
        stat = {}
        for name, _, _ in cases:
            v = sorted(ms[name])
            med, lo, hi = v[len(v) // 2], v[0], v[-1]
            stat[name[:4].strip()] = (med, lo, hi)
            rate = N * calls * K / (med * 1e-3) / 1e6
            say(f"  {name:<46} {rate:8.2f} M env-steps/s   window median {med:9.3f} ms  min {lo:9.3f}  max {hi:9.3f}")
        if "(a0)" in stat:
            spread = stat["(a0)"][2] - stat["(a0)"][1]
            ok_a = abs(stat["(a)"][0] - stat["(a0)"][0]) <= spread
            ok_b = stat["(b)"][0] - stat["(a)"][0] <= spread
            say(f"  parent's spread of repeats {spread:.3f} ms; (a) - (a0) = {stat['(a)'][0] - stat['(a0)'][0]:+.3f} ms: "
                f"{'within' if ok_a else 'OUTSIDE'}; (b) - (a) = {stat['(b)'][0] - stat['(a)'][0]:+.3f} ms: "
                f"{'within' if ok_b else 'OUTSIDE'}")
            verdicts += [ok_a, ok_b]
        del table_env
    if verdicts:
        say("both conditions hold at both K" if all(verdicts) else "a condition does NOT hold (see the lines marked OUTSIDE)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sim.close()
    if old is not None:
        old.close()


if __name__ == "__main__":
    main()
