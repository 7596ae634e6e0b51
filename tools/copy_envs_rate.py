#!/usr/bin/env python3
"""Time per call of os2r_copy_envs (include/os2r.h) against the composed path it replaces, at C4 in f64.

  python tools/copy_envs_rate.py [--envs 65536 256] [--calls 200] [--reps 5] [--out profiles/copy_envs_rate.txt]

C4 is bench.py's default workload: free_hip environments (five joints), ground contact, per-env domain randomisation.  Two
handles of --envs environments each, rolled a few hundred env-steps so that every array holds live values.  Cases, each
timed with HIP events on the current stream around --calls calls, the cases alternating within one process --reps times
(median per case, after one untimed round):
  identity     dst.copy_envs_from(src): every environment takes its namesake, loads and stores coalesced -- one launch
  fork         dst.copy_envs_from(src, index of zeros): environment 0 into every lane, one load address per wave -- one launch
  in-place     src.copy_envs_from(src, random permutation): gather into the handle's staging rows and copy back -- two launches
  composed     what existed before: src.checkpoint(), index_select with the same permutation, dst.restore() -- about 28
               launches and nine host synchronisations; the events bracket the host's share too, which is the point
Bytes per call are counted from the array sizes (every selected row read once and written once, the index read once; the
in-place case moves everything twice) and set against the 8 TB/s HBM peak the project uses; a fork reads one column, so its
figure is the written bytes.  The composed path's bytes are not counted: it is bound by launches and waits, not by memory.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def make_sim(n, seed):
    import gym_os2r_amd as g
    from gym_os2r_amd import abi, rewards
    from gym_os2r_amd.sim import HipSim
    from gym_os2r_amd.tasks.monopod import MonopodTask
    task = MonopodTask(1000, task_mode="free_hip", reward_class=rewards.BalancingV1, reset_positions=["stand"])
    task.create_spaces()
    model = g.get_model(g.config.SettingsConfig().get_config("task_modes/free_hip/model"))
    spec = task.kernel_spec(model, reset_mode=abi.RESET_RANDOM, randomize_params=True, max_episode_steps=100_000)
    return HipSim(abi.config_struct(model, spec, num_envs=n, seed=seed, contact=True, dtype=abi.F64))


def env_bytes(sim):
    """bytes of one environment over every array os2r_copy_envs moves (state and parameters)"""
    esz = 8 if str(sim.dtype).endswith("64") else 4
    rows = 10 * sim.nq + 5            # q, qd, 4 history rows, 4 nq impulses; 4 nq parameters + gravity
    return rows * esz + 3 * 4 + 1     # + solver flags, elapsed steps, episode index; pose id


def window(torch, fn, calls):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls      # us per call


def measure(torch, n, calls, reps, emit):
    src, dst = make_sim(n, 1), make_sim(n, 2)
    src.bench_steps(300); dst.bench_steps(10)
    zeros = torch.zeros(n, dtype=torch.int32, device=src.device)
    perm = torch.randperm(n, device=src.device).to(torch.int32)
    perm_l = perm.long()

    def composed():
        ck = src.checkpoint()
        new = {k: (v.index_select(-1, perm_l) if hasattr(v, "index_select") else v) for k, v in ck.items() if k != "params"}
        new["params"] = {f: v.index_select(-1, perm_l) for f, v in ck["params"].items()}
        new["step_count"] = dst.step_count
        dst.restore(new)

    b = env_bytes(src) * n
    cases = [("identity (cross-handle)", lambda: dst.copy_envs_from(src), calls, 2 * b),
             ("fork of env 0 (cross-handle)", lambda: dst.copy_envs_from(src, zeros), calls, b + 4 * n),
             ("in-place random permutation", lambda: src.copy_envs_from(src, perm), calls, 4 * b + 8 * n),
             ("composed checkpoint/index_select/restore", composed, max(calls // 10, 5), None)]
    times = {name: [] for name, _, _, _ in cases}
    for rep in range(reps + 1):                      # round 0 is the warm-up of every case (and the staging allocation)
        for name, fn, c, _ in cases:
            us = window(torch, fn, c)
            if rep:
                times[name].append(us)
    emit(f"{n} envs, f64, {env_bytes(src)} B per environment, {calls} calls per window, median of {reps} alternating windows")
    med = {}
    for name, _, _, nbytes in cases:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        bw = "" if nbytes is None else f"   {nbytes / 1e6:9.3f} MB moved  {nbytes / med[name] / 1e3:8.1f} GB/s  {100 * nbytes / (med[name] * 1e-6) / HBM_PEAK:5.1f} % of 8 TB/s"
        emit(f"  {name:<42} {med[name]:10.1f} us per call  (min {t[0]:.1f}, max {t[-1]:.1f}){bw}")
    comp = med["composed checkpoint/index_select/restore"]
    for name in ("identity (cross-handle)", "fork of env 0 (cross-handle)", "in-place random permutation"):
        emit(f"  composed / {name:<31} {comp / med[name]:8.1f} x")
    src.close(); dst.close()
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[65536, 256])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("copy_envs_rate: no GPU visible; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"os2r_copy_envs, time per call over HIP events; {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    ok = True
    for n in args.envs:
        med = measure(torch, n, args.calls, args.reps, emit)
        comp = med["composed checkpoint/index_select/restore"]
        ok = ok and med["identity (cross-handle)"] <= comp and med["fork of env 0 (cross-handle)"] <= comp
    emit("condition (identity and fork no slower than the composed path): " + ("holds" if ok else "DOES NOT HOLD"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
