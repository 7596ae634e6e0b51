#!/usr/bin/env python3
"""Time per call of os2re_ekf_update (libos2r_ekf.so, include/os2r_ekf.h) through HipSim.ekf_update_into against the batched torch
statement of the same filter step, in one run.

  python tools/ekf_update_rate.py [--robots 64 4096 65536] [--dtype f64 f32] [--reps 5] [--out profiles/ekf_update_rate.txt]

nq = 5 (n = 10 states) and D = 10 observation slots, slot d showing state column d; M robots.  The inputs are random, well
conditioned covariances, Jacobians near the identity and readings near the predicted state, on the device; no simulator is
needed: ekf_update_into is called on a HipSim that was given a layout and no handle.  Every path is warmed up with three calls, a
ten-call probe sizes its windows to about 0.3 s (at least 3 calls), and the paths alternate window by window, --reps windows each
after one untimed round: median, min and max per path, HIP events on the current stream.
  device   HipSim.ekf_update_into with its checks: one launch
  torch    bmm for P- = A P A' + Q, then the joint update: S = H P- H' + R by indexing, linalg.solve for the gain, bmm for x and P,
           and the normalised innovation squared: about a dozen statements on [M, n, n] tensors, a launch or more each
Both are timed with the covariance prediction (A given) and without it.
Reported with each device time: the compulsory bytes (x_pred, p_in's upper triangle, a, meas read; x_out, p_out, nis, used, refused
written) over the time, against 8 TB/s.  The same arrays are read in every call of a window and the largest shape moves 150 MB,
so they can be served from the 256 MiB last-level cache, not from HBM: the figure says how far the call is from the memory
system's ceiling, not what HBM delivered.  No ratio is fixed in advance: the file says what was measured.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ilqr_steer_rate import compare  # noqa: E402

PEAK = 8e12
NQ, D = 5, 10


def measure(torch, dtype, M, reps, emit):
    from gym_os2r_amd import abi, control
    from gym_os2r_amd.sim import HipSim
    dev = torch.device("cuda:0")
    dt = torch.float64 if dtype == "f64" else torch.float32
    esz = 8 if dtype == "f64" else 4
    n = 2 * NQ
    cols = list(range(D))
    sim = HipSim.__new__(HipSim)                       # the controller methods need a layout, not a simulator
    sim.N, sim.nq, sim.D, sim.dtype, sim.device = M, NQ, D, dt, dev
    sim._h = sim._lib = None
    sim._control_layout = control.layout(abi.F64 if dtype == "f64" else abi.F32, NQ, 0, cols)
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, dtype=dt, device=dev, generator=gen)
    G = rnd(M, n, n)
    P_t = 0.05 * torch.eye(n, dtype=dt, device=dev) + 0.05 / n * G @ G.transpose(1, 2)
    P_t = (0.5 * (P_t + P_t.transpose(1, 2))).contiguous()                       # [M, n, n], torch's layout
    A_t = (torch.eye(n, dtype=dt, device=dev) + 0.05 * rnd(M, n, n)).contiguous()
    x_t = rnd(M, n)
    prec = 50.0 + 150.0 * torch.rand(D, dtype=dt, device=dev, generator=gen)
    meas = (x_t[:, cols] + 0.2 * rnd(M, D)).contiguous()
    Q64 = 0.01 * torch.eye(n, dtype=torch.float64)
    Q_t = Q64.to(dev, dt)
    R_t = torch.diag(1.0 / prec)
    # the kernel's layouts, the robot index fastest
    x_k, P_k, A_k = x_t.t().contiguous(), P_t.permute(1, 2, 0).contiguous(), A_t.permute(1, 2, 0).contiguous()
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    out = dict(x=new(n, M), P=new(n, n, M), nis=new(M), used=new(M, dtype=torch.int32), refused=new(M, dtype=torch.int32))

    def device(predict):
        def fn():
            sim.ekf_update_into(x_k, P_k, meas, prec, out["x"], out["P"], A=A_k if predict else None, Q=Q64 if predict else None,
                                nis=out["nis"], used=out["used"], refused=out["refused"])
        return fn
    kept = {}

    def torch_update(predict):
        def fn():
            Pm = torch.baddbmm(Q_t, torch.bmm(A_t, P_t), A_t.transpose(1, 2)) if predict else P_t
            HP = Pm[:, cols, :]                                                 # H P-: [M, D, n]
            S = HP[:, :, cols] + R_t
            nu = meas - x_t[:, cols]
            K = torch.linalg.solve(S, HP).transpose(1, 2)                        # P- H' S^-1: [M, n, D]
            kept["x"] = x_t + torch.bmm(K, nu[:, :, None])[:, :, 0]
            kept["P"] = Pm - torch.bmm(K, HP)
            kept["nis"] = (nu * torch.linalg.solve(S, nu[:, :, None])[:, :, 0]).sum(1)
        return fn
    tol = 1e-10 if dtype == "f64" else 2e-4
    for predict in (True, False):
        device(predict)(), torch_update(predict)()
        torch.cuda.synchronize()
        assert float((out["x"].t() - kept["x"]).abs().max()) < tol and float((out["P"].permute(2, 0, 1) - kept["P"]).abs().max()) < tol, \
            "the device update and the torch statements disagree"
        assert float(((out["nis"] - kept["nis"]) / kept["nis"]).abs().max()) < tol * 100 and bool((out["used"] == 2 ** D - 1).all())
        assert not bool(out["refused"].any())
    emit(f"M = {M} robots, nq = {NQ}, D = {D}, {str(dt).split('.')[-1]}")
    labels = ("torch, with A: bmm, indexing, linalg.solve ...", "torch, without A", "device, with A: ekf_update_into", "device, without A: ekf_update_into")
    res = compare(torch, list(zip(labels, (torch_update(True), torch_update(False), device(True), device(False)))), reps, emit)
    tri = n * (n + 1) // 2
    for label, predict in zip(labels[2:], (True, False)):
        nbytes = (n + tri + (n * n if predict else 0) + D + n + n * n + 1) * M * esz + 2 * M * 4
        med = res[label][0]
        emit(f"  {label.split(':')[0]}: {nbytes / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes / (med * 1e-3) / 1e9:.1f} GB/s, "
             f"{100 * nbytes / (med * 1e-3) / PEAK:.2f} % of 8 TB/s")
    for ours, theirs in ((labels[2], labels[0]), (labels[3], labels[1])):
        emit(f"  {theirs.split(':')[0]} / {ours.split(':')[0]}: {res[theirs][0] / res[ours][0]:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, nargs="+", default=[64, 4096, 65536], help="M")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ekf_update_rate: no GPU visible; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                   # (kept as it grows: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"os2re_ekf_update through HipSim.ekf_update_into against the batched torch statement of the same filter step; HIP events; "
         f"{torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    for dtype in args.dtype:
        for M in args.robots:
            measure(torch, dtype, M, args.reps, emit)


if __name__ == "__main__":
    main()
