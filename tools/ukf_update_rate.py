#!/usr/bin/env python3
"""Time per call of os2ru_ukf_points and os2ru_ukf_update (libos2r_ukf.so, include/os2r_ukf.h) through HipSim.ukf_points_into and
HipSim.ukf_update_into against the batched torch statements of the same two halves of an unscented filter step, in one run.

  python tools/ukf_update_rate.py [--robots 64 4096 65536] [--dtype f64 f32] [--reps 5] [--out profiles/ukf_update_rate.txt]

nq = 5 (n = 10 states, S = 21 sigma points) and D = 10 observation slots, slot d showing state column d; M robots.  The inputs
are random, well conditioned covariances and, as the propagated points, the sigma points themselves moved by a small random
linear map, on the device; no simulator is needed: the methods are called on a HipSim that was given a layout and no handle.
Every path is warmed up with three calls, a ten-call probe sizes its windows to about 0.3 s (at least 3 calls), and the paths
alternate window by window, --reps windows each after one untimed round: median, min and max per path, HIP events on the
current stream.
  points, device   HipSim.ukf_points_into with its checks: one launch
  points, torch    linalg.cholesky, then cat of x, x + gamma L' and x - gamma L' into the [n, S M] layout set_state takes
  update, device   HipSim.ukf_update_into with its checks, without and with points_out (the next step's points): one launch
  update, torch    the points gathered to [M, S, n], einsum for mean and covariance, then the joint update: S = H P- H' + R by
                   indexing, linalg.solve for the gain, bmm for x and P, and the normalised innovation squared
Reported with each device time: the compulsory bytes over the time, against 8 TB/s.  The same arrays are read in every call of a
window and may be served from the 256 MiB last-level cache, not from HBM: the figure says how far the call is from the memory
system's ceiling, not what HBM delivered.  No ratio is fixed in advance: the file says what was measured, a shape that loses
included.
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
    from gym_os2r_amd import abi, control, ukf
    from gym_os2r_amd.sim import HipSim
    dev = torch.device("cuda:0")
    dt = torch.float64 if dtype == "f64" else torch.float32
    esz = 8 if dtype == "f64" else 4
    n = 2 * NQ
    S = ukf.npoints(NQ)
    cols = list(range(D))
    sim = HipSim.__new__(HipSim)                       # the controller methods need a layout, not a simulator
    sim.N, sim.nq, sim.D, sim.dtype, sim.device = S * M, NQ, D, dt, dev
    sim._h = sim._lib = None
    sim._control_layout = control.layout(abi.F64 if dtype == "f64" else abi.F32, NQ, 0, cols)
    gamma, wm0, wc0, wi = ukf.weights(n)
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, dtype=dt, device=dev, generator=gen)
    G = rnd(M, n, n)
    P_t = 0.05 * torch.eye(n, dtype=dt, device=dev) + 0.05 / n * G @ G.transpose(1, 2)
    P_t = (0.5 * (P_t + P_t.transpose(1, 2))).contiguous()                       # [M, n, n], torch's layout
    x_t = rnd(M, n)
    prec = 50.0 + 150.0 * torch.rand(D, dtype=dt, device=dev, generator=gen)
    Q64 = 0.01 * torch.eye(n, dtype=torch.float64)
    Q_t = Q64.to(dev, dt)
    R_t = torch.diag(1.0 / prec)
    # the kernel's layouts, the robot index fastest
    x_k, P_k = x_t.t().contiguous(), P_t.permute(1, 2, 0).contiguous()
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    i32 = torch.int32
    out = dict(points=new(n, S * M), failed=new(M, dtype=i32), x=new(n, M), P=new(n, n, M), nis=new(M), used=new(M, dtype=i32),
               refused=new(M, dtype=i32), lost=new(M, dtype=i32), next=new(n, S * M), next_failed=new(M, dtype=i32))
    kept = {}

    def points_device():
        sim.ukf_points_into(x_k, P_k, out["points"], failed=out["failed"])

    def points_torch():
        L = torch.linalg.cholesky(P_t)                                          # [M, n, n]
        step = gamma * L.transpose(1, 2)                                        # row j: gamma L[:, j]
        chi = torch.cat((x_t[:, None, :], x_t[:, None, :] + step, x_t[:, None, :] - step), 1)    # [M, S, n]
        kept["points"] = chi.permute(2, 1, 0).reshape(n, S * M)                 # the layout set_state takes: a copy
    points_device(), points_torch()
    torch.cuda.synchronize()
    tol = 1e-10 if dtype == "f64" else 2e-4
    assert float((out["points"] - kept["points"]).abs().max()) < tol and not bool(out["failed"].any()), "the device points and torch's disagree"
    # the propagated points: the points themselves under a small linear map per robot
    F = torch.eye(n, dtype=dt, device=dev) + 0.05 * rnd(M, n, n)
    cube = out["points"].reshape(n, S, M)
    moved = torch.einsum("mij,jsm->ism", F, cube).reshape(n, S * M).contiguous()
    q_k, qd_k = moved[:NQ], moved[NQ:]
    done = torch.zeros(S * M, dtype=torch.uint8, device=dev)
    meas = (torch.einsum("mij,mj->mi", F, x_t)[:, cols] + 0.2 * rnd(M, D)).contiguous()

    def update_device(with_points):
        def fn():
            sim.ukf_update_into((q_k, qd_k), P_k, meas, prec, out["x"], out["P"], Q=Q64, done=done, nis=out["nis"], used=out["used"],
                                refused=out["refused"], lost=out["lost"], points_out=out["next"] if with_points else None,
                                failed=out["next_failed"] if with_points else None)
        return fn

    def update_torch():
        chi = torch.cat((q_k, qd_k)).reshape(n, S, M).permute(2, 1, 0)           # [M, S, n]
        xbar = wm0 * chi[:, 0] + wi * chi[:, 1:].sum(1)
        d = chi - xbar[:, None, :]
        Pm = Q_t + wc0 * torch.einsum("mi,mj->mij", d[:, 0], d[:, 0]) + wi * torch.einsum("msi,msj->mij", d[:, 1:], d[:, 1:])
        HP = Pm[:, cols, :]                                                 # H P-: [M, D, n]
        Sm = HP[:, :, cols] + R_t
        nu = meas - xbar[:, cols]
        K = torch.linalg.solve(Sm, HP).transpose(1, 2)                       # P- H' S^-1: [M, n, D]
        kept["x"] = xbar + torch.bmm(K, nu[:, :, None])[:, :, 0]
        kept["P"] = Pm - torch.bmm(K, HP)
        kept["nis"] = (nu * torch.linalg.solve(Sm, nu[:, :, None])[:, :, 0]).sum(1)
    update_device(True)(), update_torch()
    torch.cuda.synchronize()
    assert float((out["x"].t() - kept["x"]).abs().max()) < tol and float((out["P"].permute(2, 0, 1) - kept["P"]).abs().max()) < tol, \
        "the device update and the torch statements disagree"
    assert float(((out["nis"] - kept["nis"]) / kept["nis"]).abs().max()) < tol * 100 and bool((out["used"] == 2 ** D - 1).all())
    assert not bool(out["refused"].any()) and not bool(out["lost"].any()) and not bool(out["next_failed"].any())
    emit(f"M = {M} robots, nq = {NQ}, S = {S}, D = {D}, {str(dt).split('.')[-1]}")
    labels = ("points, torch: linalg.cholesky, cat, permute", "update, torch: einsum, indexing, linalg.solve ...", "points, device: ukf_points_into",
              "update, device, no points_out: ukf_update_into", "update, device, with points_out: ukf_update_into")
    res = compare(torch, list(zip(labels, (points_torch, update_torch, points_device, update_device(False), update_device(True)))), reps, emit)
    tri = n * (n + 1) // 2
    state = n * S * M
    # compulsory: points reads x and the upper triangle of p, writes the points and failed; the update reads the state, the done flags
    # and meas (p_in is read too, although only a lost robot needs it: counted), writes x, p, nis and three int32 per robot
    nbytes = {labels[2]: (n + tri + n * S) * M * esz + M * 4,
              labels[3]: state * esz + S * M + (tri + D + n + n * n + 1) * M * esz + 3 * M * 4,
              labels[4]: state * esz + S * M + (tri + D + n + n * n + 1) * M * esz + 4 * M * 4 + state * esz}
    for label in labels[2:]:
        med = res[label][0]
        emit(f"  {label.split(':')[0]}: {nbytes[label] / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes[label] / (med * 1e-3) / 1e9:.1f} GB/s, "
             f"{100 * nbytes[label] / (med * 1e-3) / PEAK:.2f} % of 8 TB/s")
    for ours, theirs in ((labels[2], labels[0]), (labels[3], labels[1]), (labels[4], labels[1])):
        emit(f"  {theirs.split(':')[0]} / {ours.split(':')[0]}: {res[theirs][0] / res[ours][0]:.2f}")
    both = res[labels[0]][0] + res[labels[1]][0]
    emit(f"  a filter step: torch points + update {both:.4f} ms; device points + update {res[labels[2]][0] + res[labels[3]][0]:.4f} ms; "
         f"device update with points_out {res[labels[4]][0]:.4f} ms: {both / res[labels[4]][0]:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, nargs="+", default=[64, 4096, 65536], help="M")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ukf_update_rate: no GPU visible; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                   # (kept as it grows: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"os2ru_ukf_points and os2ru_ukf_update through HipSim.ukf_points_into / ukf_update_into against the batched torch statements of "
         f"the same filter step; HIP events; {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    for dtype in args.dtype:
        for M in args.robots:
            measure(torch, dtype, M, args.reps, emit)


if __name__ == "__main__":
    main()
