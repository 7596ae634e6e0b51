#!/usr/bin/env python3
"""Time per call of HipSim.natural_step_into (libos2r_npg.so, include/os2r_npg.h) against the batched torch statement of the same
step and against the sibling HipSim.value_fit_into on the same arrays, in one run.

  python tools/npg_rate.py [--shapes 1,8192,500 1,65536,50 64,256,50 4096,16,50 65536,1,50] [--dtype f64 f32] [--reps 5]
                           [--out profiles/npg_rate.txt]

A shape is P policies, S samples per policy, K steps; N = S P lanes, D = 10 observation slots (the free_hip robot's).  The inputs
are random on the device -- observations uniform in [-1, 1], actions N(0, 0.7) clipped to [-1, 1] (a clip binds on about 15 % of
the steps), lengths between K / 2 and K, a gradient and a gradient of the widths ~ N(0, 1) --; a small handle of the free_hip
robot is made for its methods alone.  Every path is warmed up with three calls, a ten-call probe sizes its windows to about
0.3 s (at least 3 calls), and the paths alternate window by window, --reps windows each after one untimed round: median, min and
max per path, HIP events on the current stream.
  torch        a masked einsum for the two moment matrices of every policy, linalg.cholesky and cholesky_solve for the two
               directions, the widths' scalar entries and the scaling
  value fit    value_fit_into on the same observations and lengths with every output, its tensors made once: one set of 77
               sums a lane where the natural step has 132
  device       natural_step_into with every output, its tensors made once
Reported with the device time: the compulsory bytes -- of the counted steps the observations and the action pairs read,
lane_mom written and read again, lane_count, mom, the gradient and the outputs -- over the time, against 8 TB/s.  No ratio is
fixed in advance: the file says what was measured.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ilqr_steer_rate import compare  # noqa: E402

D, DAMPING, KL, RIDGE, PEAK = 10, 1e-3, 0.01, 1e-3, 8e12


def measure(torch, sim, P, S, K, reps, emit):
    from gym_os2r_amd import critic, npg
    dev, dt = sim.device, sim.dtype
    esz = 8 if dt == torch.float64 else 4
    N, E, Ef = S * P, npg.moments(D), critic.moments(D)
    i32 = torch.int32
    gen = torch.Generator(device=dev).manual_seed(0)
    uni = lambda *s: torch.rand(*s, dtype=dt, device=dev, generator=gen) * 2 - 1
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    obs, obs0 = uni(K, N, D), uni(N, D)
    act = (torch.randn(K, N, 2, dtype=dt, device=dev, generator=gen) * 0.7).clamp(-1, 1)
    sigma = torch.tensor([0.2, 0.3], dtype=dt, device=dev)
    length = torch.randint(max(1, K // 2), K + 1, (N,), device=dev, generator=gen).to(i32)
    grad = torch.randn(2, D + 1, P, dtype=dt, device=dev, generator=gen)
    lsig = torch.randn(2, P, dtype=dt, device=dev, generator=gen)
    target = torch.rand(K, N, dtype=dt, device=dev, generator=gen)
    step, direction, ls_step, beta, quad = new(2, D + 1, P), new(2, D + 1, P), new(2, P), new(P), new(P)
    failed, steps, opened, valid = new(3, P, dtype=i32), new(P, dtype=i32), new(2, P, dtype=i32), new(P, dtype=i32)
    lane_mom, mom, count = new(E, N), new(E, P), new(4, N, dtype=i32)
    w, fit_lane, fit_mom, fit_count = new(D + 1, P), new(Ef, N), new(Ef, P), new(2, N, dtype=i32)
    fit_failed, fit_steps, fit_valid = (new(P, dtype=i32) for _ in range(3))
    counted = torch.arange(K, device=dev).unsqueeze(1) < length.unsqueeze(0)                     # [K, N]: made once
    kept = {}

    def device_step():
        sim.natural_step_into(obs, sigma, grad, step, lane_mom, mom, count, policies=P, obs0=obs0, actions=act, length=length, lsig_grad=lsig,
                              damping=DAMPING, kl=KL, dir=direction, lsig_step=ls_step, beta=beta, quad=quad, failed=failed, steps=steps,
                              open=opened, valid=valid)

    def device_fit():
        sim.value_fit_into(obs, target, w, fit_lane, fit_mom, fit_count, obs0=obs0, policies=P, length=length, ridge=RIDGE, failed=fit_failed,
                           steps=fit_steps, valid=fit_valid)

    def torch_step():
        rows = torch.cat([obs0.unsqueeze(0), obs[:-1]])
        phi = torch.cat([rows, torch.ones(K, N, 1, dtype=dt, device=dev)], 2).view(K, S, P, D + 1)
        mask = ((act.abs() < 1) & counted.unsqueeze(-1)).to(dt).view(K, S, P, 2)
        c = counted.view(K, S, P).sum((0, 1)).to(dt)                                            # [P]
        F = torch.einsum("kspj,kspa,kspb->jpab", mask, phi, phi) / (sigma * sigma).view(2, 1, 1, 1) / c.view(1, P, 1, 1)
        A = F + DAMPING * torch.eye(D + 1, dtype=dt, device=dev)
        g = (grad / c).permute(0, 2, 1).unsqueeze(-1)                                           # [2, P, D+1, 1]
        d = torch.cholesky_solve(g, torch.linalg.cholesky(A)).squeeze(-1)                       # [2, P, D+1]
        g_ls = lsig / c
        d_ls = g_ls / (2 * mask.sum((0, 1)).t() / c + DAMPING)
        q = (g.squeeze(-1) * d).sum((0, 2)) + (g_ls * d_ls).sum(0)
        kept["step"] = (torch.sqrt(2 * KL / q).view(1, P, 1) * d).permute(0, 2, 1)

    device_step()
    torch_step()
    device_fit()
    torch.cuda.synchronize()
    tol = 1e-8 if dt == torch.float64 else 2e-2           # (both paths sum millions of terms in the dtype, in different orders)
    far = float((step - kept["step"]).abs().max()) / float(kept["step"].abs().max())
    assert far < tol, f"the device call and the torch statement disagree: {far}"
    assert int(valid.sum()) == N and int(steps.sum()) == int(length.sum()) and int(failed.sum()) == 0 and int(fit_failed.sum()) == 0
    emit(f"P = {P} policies, S = {S} samples, K = {K} steps, N = {N} lanes, D = {D}, {str(dt).split('.')[-1]}")
    walked = int(length.sum())
    nbytes = ((walked * (D + 2) + N * D + 2) * esz + N * 4 + 2 * (E * N * esz + 4 * N * 4) + 2 * E * P * esz + 4 * P * 4
              + (2 * (D + 1) + 2) * P * esz + (2 * 2 * (D + 1) + 2 + 2) * P * esz + 3 * P * 4)
    labels = ("torch: einsum, cholesky, cholesky_solve", "device, sibling: value_fit_into", "device: natural_step_into")
    res = compare(torch, list(zip(labels, (torch_step, device_fit, device_step))), reps, emit)
    med = res[labels[2]][0]
    emit(f"  device: {nbytes / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes / (med * 1e-3) / 1e9:.1f} GB/s, "
         f"{100 * nbytes / (med * 1e-3) / PEAK:.2f} % of 8 TB/s")
    emit(f"  torch / device: {res[labels[0]][0] / med:.2f}   device / value_fit_into: {med / res[labels[1]][0]:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1,8192,500", "1,65536,50", "64,256,50", "4096,16,50", "65536,1,50"], help="P,S,K")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("npg_rate: no GPU visible; nothing is measured without one")
    from gym_os2r_amd import abi
    from gym_os2r_amd.sim import HipSim
    from helpers import make_config
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                   # (kept as it grows: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"HipSim.natural_step_into against the torch statement and against HipSim.value_fit_into; HIP events; "
         f"{torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    for dtype in args.dtype:
        sim = HipSim(make_config("free_hip", "BalancingV2", False, num_envs=4, contact=True, seed=1,
                                 dtype=abi.F64 if dtype == "f64" else abi.F32)[0])
        assert sim.D == D
        for shape in args.shapes:
            P, S, K = (int(v) for v in shape.split(","))
            measure(torch, sim, P, S, K, args.reps, emit)
            torch.cuda.empty_cache()
        sim.close()


if __name__ == "__main__":
    main()
