#!/usr/bin/env python3
"""Time per plan of os2r_lqr_gains (include/os2r.h) against the torch loop of the examples it replaces, on identical inputs.

  python tools/lqr_gains_rate.py [--cases stationary trajectory] [--dtype f64] [--reps 5] [--out profiles/lqr_gains_rate.txt]
                                 [--stationary 1 500 65536] [--trajectory 50 1 16384]        (knots sweeps trajectories)

Both cases use the free_hip robot (nq 5, n = 10, D = 10 raw observation slots: Monopod-nonorm-balance-v1's layout) and synthetic
Jacobians A = I + 0.3 N(0,1) / sqrt(n), B = 0.5 N(0,1), an SPD Q with a zero first row and column, R = [[.1, .02], [.02, .2]]:
  stationary   K = 1, sweeps = 500, M = 65 536: examples/lqr_balancing.py, one problem per environment
  trajectory   K = 50, sweeps = 1, M = 16 384: examples/tvlqr_tracking.py's recursion, batched over trajectories
Paths, each timed with HIP events on the current stream, alternating within one process --reps times after one untimed round
(median, min and max per path):
  device   sim.lqr_gains_into(...): one launch that also writes the weight table; caller-owned outputs, nothing allocated
  torch    the examples' loop, kept on the device: per knot K_k = linalg.solve(R + B'PB, B'PA), P <- Q + A'P(A - B K_k),
           P <- (P + P') / 2, then weights_of_gain; its inputs are [M, n, n] copies made once, outside the window
The device path's window holds as many calls as fit about 0.3 s (at least 3); the torch loop is one plan per window.  Before
anything is timed the two gain tables are compared (they differ by rounding: another order of the same sums).
Bytes and operations are counted from the shapes: a knot reads (n^2 + 2n) values per trajectory (960 B in fp64) and does
n^2 (n + 2) + 2 n (n + 2) + n^2 (n + 1) / 2 multiply-adds (1 990 at n = 10), each a multiplication and an addition.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def make_sim(dtype):
    import gym_os2r_amd as g
    from gym_os2r_amd import abi, rewards
    from gym_os2r_amd.sim import HipSim
    from gym_os2r_amd.tasks.monopod_no_norm import MonopodTask
    task = MonopodTask(1000, task_mode="free_hip", reward_class=rewards.BalancingV1, reset_positions=["stand"])
    task.create_spaces()
    model = g.get_model(g.config.SettingsConfig().get_config("task_modes/free_hip/model"))
    spec = task.kernel_spec(model, reset_mode=abi.RESET_FIXED, randomize_params=False, max_episode_steps=0)
    # (the call takes the dtype, nq and the observation layout from its handle: 64 environments do)
    return HipSim(abi.config_struct(model, spec, num_envs=64, seed=1, contact=True, dtype=abi.F64 if dtype == "f64" else abi.F32))


def window(torch, fn, calls):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls      # ms per call


def measure(torch, sim, name, K, sweeps, M, reps, emit):
    from lqr_balancing import state_column_of_slot, weights_of_gain
    dev, dt, n, D = sim.device, sim.dtype, 2 * sim.nq, sim.D
    L = K * M
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, dtype=dt, device=dev, generator=gen)
    A = torch.eye(n, dtype=dt, device=dev)[:, :, None] + 0.3 * rnd(n, n, L) / n ** 0.5          # the kernel's layout
    B = 0.5 * rnd(n, 2, L)
    g = torch.randn(n - 1, n - 1, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    Q = torch.zeros(n, n, dtype=torch.float64)
    Q[1:, 1:] = g @ g.T / (n - 1) + 0.1 * torch.eye(n - 1, dtype=torch.float64)
    Q = 0.5 * (Q + Q.T)
    R = torch.tensor([[0.1, 0.02], [0.02, 0.2]], dtype=torch.float64)
    actions, obs = torch.rand(L, 2, dtype=dt, device=dev, generator=gen) * 2 - 1, rnd(L, D)
    cols = state_column_of_slot(sim.cfg.task, sim.nq)
    gains, flags, table = (torch.empty(K, 2, n, M, dtype=dt, device=dev), torch.empty(K, M, dtype=torch.uint8, device=dev),
                           torch.empty(K, 2, D + 1, M, dtype=dt, device=dev))

    def device():
        sim.lqr_gains_into(A, B, Q, R, knots=K, sweeps=sweeps, gains_out=gains, flags_out=flags, actions=actions, obs=obs,
                           weights_out=table)

    # the torch path's inputs, as the examples hold them: [K, M, n, n] contiguous, Q and R on the device
    At = A.view(n, n, K, M).permute(2, 3, 0, 1).contiguous()
    Bt = B.view(n, 2, K, M).permute(2, 3, 0, 1).contiguous()
    Qd, Rd = Q.to(dev, dt), R.to(dev, dt)
    a_k, o_k = actions.view(K, M, 2), obs.view(K, M, D)

    def loop():
        P = Qd.expand(M, n, n)
        Ks = [None] * K
        for _ in range(sweeps):
            for k in range(K - 1, -1, -1):
                Ak, Bk = At[k], Bt[k]
                Bkt = Bk.transpose(1, 2)
                Kk = torch.linalg.solve(Rd + Bkt @ P @ Bk, Bkt @ P @ Ak)
                P = Qd + Ak.transpose(1, 2) @ P @ (Ak - Bk @ Kk)
                P = 0.5 * (P + P.transpose(1, 2))
                Ks[k] = Kk
        return Ks, [weights_of_gain(Ks[k], a_k[k], o_k[k], cols) for k in range(K)]

    device()
    Ks, _ = loop()
    torch.cuda.synchronize()
    ref = torch.stack(Ks)                                                  # [K, M, 2, n]
    got = gains.permute(0, 3, 1, 2)
    rel = float((got - ref).abs().max() / ref.abs().max())
    emit(f"{name}: K = {K}, sweeps = {sweeps}, M = {M}, {str(dt).split('.')[-1]}; {int(flags.sum())} knots refused; "
         f"largest |K_device - K_torch| / max |K_torch| = {rel:.2e}")
    calls = max(3, min(200, int(300.0 / max(window(torch, device, 1), 1e-3))))
    cases = [("device: one os2r_lqr_gains launch", device, calls), ("torch: the examples' loop", loop, 1)]
    times = {c[0]: [] for c in cases}
    for rep in range(reps + 1):                      # round 0 is the warm-up of both paths
        for label, fn, c in cases:
            ms = window(torch, fn, c)
            if rep:
                times[label].append(ms)
    med = {}
    for label, _, c in cases:
        t = sorted(times[label])
        med[label] = t[len(t) // 2]
        emit(f"  {label:<36} {med[label]:12.3f} ms per plan  (min {t[0]:.3f}, max {t[-1]:.3f}; {c} per window, {reps} windows)")
    d_, t_ = (med[c[0]] for c in cases)
    ratios = sorted(b / a for a in times[cases[0][0]] for b in times[cases[1][0]])
    emit(f"  torch / device {t_ / d_:10.1f} x  (over all pairs of windows: {ratios[0]:.1f} .. {ratios[-1]:.1f})")
    esz = A.element_size()
    knots = K * sweeps * M
    bytes_ = (n * n + 2 * n) * esz * (K * M if K == 1 else knots) + (2 * n + 2 * (D + 1)) * esz * K * M + K * M
    fma = n * n * (n + 2) + 2 * n * (n + 2) + n * n * (n + 1) // 2        # P [A|B]; the rows of G and B'PB; the upper triangle of A'(PA)
    emit(f"  device: {knots / d_ * 1e-6:.2f} G knot-trajectories / s; {bytes_ / d_ * 1e-6:.1f} GB/s of compulsory traffic; "
         f"{2 * fma * knots / d_ * 1e-9:.2f} TFLOP/s counting {fma} multiply-adds per knot")
    return d_ <= t_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["stationary", "trajectory"], choices=["stationary", "trajectory"])
    ap.add_argument("--stationary", type=int, nargs=3, default=[1, 500, 65536], metavar=("K", "SWEEPS", "M"))
    ap.add_argument("--trajectory", type=int, nargs=3, default=[50, 1, 16384], metavar=("K", "SWEEPS", "M"))
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lqr_gains_rate: no GPU visible; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"os2r_lqr_gains against the torch loop, time per plan over HIP events; {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    sim = make_sim(args.dtype)
    faster = True
    for name in args.cases:
        K, sweeps, M = getattr(args, name)
        faster = measure(torch, sim, name, K, sweeps, M, args.reps, emit) and faster
    emit("the launch is faster than the loop in every case measured: " + ("yes" if faster else "NO"))
    sim.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
