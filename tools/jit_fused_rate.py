#!/usr/bin/env python3
"""What a custom robot's own fused code objects (gym_os2r_amd/jit.py, csrc/os2r_jit_fused_unit.hip) buy over the launch loop,
and what their first use costs.

  python tools/jit_fused_rate.py [--envs 65536,4096] [--preroll 1000] [--steps 100] [--reps 5] [--rounds 2]
                                 [--first-use | --no-first-use] [--no-rates] [--out profiles/jit_fused_rate.txt [--append]]

The robot is tests/helpers.perturbed_model("free_hip", seed 79): no compiled-in table matches, so every handle runs on code
objects built for it.  The workload is bench.py's C4 on that robot, in f64: free_hip, BalancingV1, ground contact, per-env
domain randomisation, rolled into the stationary regime (--preroll device-action env-steps) before anything is timed.  Every
case starts from the checkpoint of that regime and times --steps env-steps in calls of K = 50 with HIP events on the current
stream, after one untimed warm-up call; --reps windows per case, the median is reported with min and max.

A handle keeps the kernels that were registered when it was created, and registrations are per process.  So each side of a
comparison is a child process of its own, started fresh (never a replaced program):
  fused    default environment: the step, rollout, policy and linearize objects
  loop     OS2R_JIT_FUSED=0: the step object only -- rollout() is K launches, a policy rollout three launches per env-step,
           linearize() the library's generic run-time-model kernels
  generic  OS2R_JIT=0: no code object at all (reported for linearize)
The children run in the order fused, loop, generic and then backwards (--rounds), so that no side always runs behind the same
one; the windows of all rounds are pooled.  Cases: rollout(K) with device-drawn actions, rollout_policy(K, W) with shared weights,
rollout_schedule(K, table) on the window clock with T = K, and linearize (all outputs; the rate counts environments linearised).

--first-use times jit.build_all for a robot the cache has never seen (seed from the clock) into an empty directory, with and
without OS2R_JIT_FUSED=0: the wall time a user waits before the first step.  It needs hipcc and no GPU, and depends on the
host's cores (the four objects compile side by side); the line names their number.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
K = 50
CASES = ("rollout", "rollout_policy", "rollout_schedule", "linearize")


def robot(seed=79):
    import numpy as np
    from helpers import perturbed_model
    return perturbed_model("free_hip", np.random.default_rng(seed))


def make_cfg(envs, model):
    from helpers import make_config
    from gym_os2r_amd import abi
    return make_config("free_hip", "BalancingV1", True, reset_mode=abi.RESET_RANDOM, randomize_params=True, max_episode_steps=100_000,
                       model_overrides=model, num_envs=envs, seed=0, contact=True, dtype=abi.F64)[0]


def window_ms(torch, sim, ck, fn, calls):
    """GPU milliseconds of `calls` calls of fn from checkpoint `ck`, after one warm-up call."""
    sim.restore(ck)
    fn()
    sim.restore(ck)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def worker(args):
    """One side of the comparison in this process: {envs: {case: [ms per window]}} as one JSON line."""
    import torch
    from gym_os2r_amd.sim import HipSim
    out = {"specialised": None, "name": torch.cuda.get_device_name(0)}
    for envs in args.envs:
        sim = HipSim(make_cfg(envs, robot()))
        out["specialised"] = bool(sim.specialised)
        sim.bench_steps(max(args.preroll, 1))
        ck = sim.checkpoint()
        g = torch.Generator(device=sim.device).manual_seed(1)
        w = 0.3 * torch.randn(2, sim.D + 1, dtype=sim.dtype, device=sim.device, generator=g)
        table = w.unsqueeze(0).repeat(K, 1, 1).contiguous()
        act = torch.rand(sim.N, 2, dtype=sim.dtype, device=sim.device, generator=g) * 2 - 1
        n2 = 2 * sim.nq
        nxt, ja, jb = sim._new(n2, sim.N), sim._new(n2, n2, sim.N), sim._new(n2, 2, sim.N)
        calls = max(args.steps // K, 1)
        obs, rew = sim._new(K, sim.N, sim.D), sim._new(K, sim.N)
        done = sim._new(K, sim.N, dtype=torch.uint8)
        fns = {"rollout": (lambda: sim.rollout_into(K, None, obs, rew, done), calls), "rollout_policy": (lambda: sim.rollout_policy(K, w), calls),
               "rollout_schedule": (lambda: sim.rollout_schedule(K, table), calls),
               "linearize": (lambda: sim.linearize_into(act, None, nxt, ja, jb), 5)}
        ms = {c: [] for c in CASES}
        for r in range(args.reps):
            for c in (CASES if r % 2 == 0 else CASES[::-1]):
                ms[c].append(window_ms(torch, sim, ck, *fns[c]))
        out[str(envs)] = ms
        sim.close()
    print("RESULT " + json.dumps(out), flush=True)


def first_use(fused):
    """Wall seconds of jit.build_all for a robot no cache holds, into an empty directory."""
    from gym_os2r_amd import jit
    cfg = make_cfg(64, robot(seed=time.time_ns() % (2 ** 32)))
    with tempfile.TemporaryDirectory(prefix="os2r_first_use_") as d:
        os.environ["OS2R_KERNEL_CACHE"] = d
        os.environ["OS2R_JIT_FUSED"] = "1" if fused else "0"
        t = time.perf_counter()
        paths = jit.build_all(cfg.model, int(cfg.dtype), True, jit.task_layout(cfg.task))
        return time.perf_counter() - t, sorted(paths)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="65536,4096", type=lambda s: [int(v) for v in s.split(",")])
    ap.add_argument("--preroll", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=100, help="env-steps per timed window (a multiple of 50)")
    ap.add_argument("--reps", type=int, default=5, help="windows per case and child process")
    ap.add_argument("--rounds", type=int, default=2, help="passes over the child processes, in turns forwards and backwards")
    ap.add_argument("--first-use", dest="first_use", action="store_true", default=None)
    ap.add_argument("--no-first-use", dest="first_use", action="store_false")
    ap.add_argument("--no-rates", action="store_true", help="only the first-use build times (needs no GPU)")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to --out (the rates and the build times may come from two runs)")
    args = ap.parse_args()
    os.environ.setdefault("OS2R_KERNEL_CACHE", os.path.join(ROOT, ".kernel_cache"))
    if args.worker:
        return worker(args)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    sides = {"fused": {"OS2R_JIT": "1", "OS2R_JIT_FUSED": "1"}, "loop": {"OS2R_JIT": "1", "OS2R_JIT_FUSED": "0"},
             "generic": {"OS2R_JIT": "0"}}
    if not args.no_rates:
        pooled, name = {}, "?"
        for rnd in range(args.rounds):
            for side in (list(sides) if rnd % 2 == 0 else list(sides)[::-1]):
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", side, "--envs", ",".join(map(str, args.envs)),
                       "--preroll", str(args.preroll), "--steps", str(args.steps), "--reps", str(args.reps)]
                r = subprocess.run(cmd, env={**os.environ, **sides[side]}, stdout=subprocess.PIPE, text=True, timeout=600)
                res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not res:
                    raise SystemExit(f"the {side} child failed ({r.returncode}):\n{r.stdout[-2000:]}")
                res = json.loads(res[-1][7:])
                assert res["specialised"] == (side != "generic"), (side, res["specialised"])
                name = res["name"]
                for envs in args.envs:
                    for c, v in res[str(envs)].items():
                        pooled.setdefault((side, envs, c), []).extend(v)
        say(f"custom free_hip robot (perturbed, seed 79), BalancingV1, ground contact, per-env domain randomisation, f64; preroll "
            f"{args.preroll}, {args.steps} env-steps per window in calls of K = {K}, {args.reps} windows x {args.rounds} child processes "
            f"per side; {name}, {time.strftime('%Y-%m-%d')}")
        for envs in args.envs:
            say(f"{envs} envs:")
            med = {}
            for c in CASES:
                for side in sides:
                    v = sorted(pooled[side, envs, c])
                    m = med[side, c] = v[len(v) // 2]
                    work = envs * (5 if c == "linearize" else max(args.steps // K, 1) * K)
                    unit = "M linearisations/s" if c == "linearize" else "M env-steps/s"
                    say(f"  {c:<17} {side:<8} {work / (m * 1e-3) / 1e6:9.2f} {unit:<19} window median {m:9.3f} ms  min {v[0]:9.3f}  max {v[-1]:9.3f}")
            for c in CASES[:3]:
                say(f"  {c}: fused / loop = {med['loop', c] / med['fused', c]:.3f}x")
            say(f"  linearize: code object / generic kernels (OS2R_JIT=0) = {med['generic', 'linearize'] / med['fused', 'linearize']:.3f}x"
                f"; / OS2R_JIT_FUSED=0 = {med['loop', 'linearize'] / med['fused', 'linearize']:.3f}x")
    else:
        say("rates: not measured in this run (--no-rates)")
    if args.first_use or (args.first_use is None and args.no_rates):
        for fused in (True, False):
            secs, kinds = first_use(fused)
            say(f"first use, empty cache, {'default' if fused else 'OS2R_JIT_FUSED=0'}: jit.build_all {secs:6.1f} s wall for {', '.join(kinds)} "
                f"({len(os.sched_getaffinity(0))} cores)")
    else:
        say("first-use build times: not measured in this run (--first-use)")
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
