#!/usr/bin/env python3
"""Time per call of os2rb_ilqr_backward_box (include/os2r_box.h) against its sibling os2rt_ilqr_backward_mu on the same arrays, in
one run.

  python tools/ilqr_box_rate.py [--knots 50] [--traj 64 4096 16384] [--dtype f64 f32] [--reps 5] [--out profiles/ilqr_box_rate.txt]

The free_hip robot (nq 5, n = 10, D = 10), K knots, mu_dev = 0.5 everywhere, the box (-1, 1); gains, ff, flags and dv asked of
both, the clamp bytes of the box pass, and -- `table` -- the weight table for the four step sizes 1, 1/2, 1/4, 1/8 or none.
Synthetic A, B of tools/ilqr_backward_rate.py's kind; the gradients lx, lu and p_final are scaled by one factor, found by bisection
on the device before anything is timed, until about a third of the knots have a clamped component (`a third`), or are zero, so
that every step is 0 and none is clamped (`none`: every wave skips the edge candidates).  Every path is warmed up with three
calls, a ten-call probe sizes its windows to about 0.3 s, and the two paths alternate window by window, --reps windows each after
one untimed round: median, min and max per path, HIP events on the current stream (tools/ilqr_steer_rate.py's method and code).
The yardstick is the sibling.  The box pass is called slower only beyond the sibling's own window range plus the share of the
added compulsory bytes in what the sibling moves: the K M clamp bytes and, without the table, the 2 K M words of the nominal
actions (with the table the sibling moves them already).
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ilqr_steer_rate import ALPHAS, compare, make_sim, verdict  # noqa: E402


def measure(torch, sim, K, M, reps, emit):
    from gym_os2r_amd import abi, box, control, steer
    from gym_os2r_amd.control import slot_columns
    dev, dt, nq, D = sim.device, sim.dtype, sim.nq, sim.D
    n, nal = 2 * nq, len(ALPHAS)
    N, L = nal * M, K * M
    esz = 8 if dt == torch.float64 else 4
    cols = slot_columns(sim.cfg.task, nq)
    shown = [c for c in cols if c >= 0]
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, dtype=dt, device=dev, generator=gen)
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    lay = control.layout(abi.F64 if dt == torch.float64 else abi.F32, nq, sim.cfg.device, cols)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    qdiag = [0.0 if c not in shown else (1.0 if c < nq else 0.01) for c in range(n)]
    q = (C.c_double * (n * n))(*[qdiag[i] if i == j else 0.0 for i in range(n) for j in range(n)])
    r = (C.c_double * 4)(0.1, 0.0, 0.0, 0.1)
    al = (C.c_double * nal)(*ALPHAS)
    lo, hi = (C.c_double * 2)(-1.0, -1.0), (C.c_double * 2)(1.0, 1.0)

    A = torch.eye(n, dtype=dt, device=dev)[:, :, None] + 0.3 * rnd(n, n, L) / n ** 0.5
    B = 0.5 * rnd(n, 2, L)
    lx0, lu0, pv0 = rnd(n, L), 0.3 * rnd(2, L), rnd(n, M)
    lx, lu, pv = new(n, L), new(2, L), new(n, M)
    act, obs = torch.rand(L, 2, dtype=dt, device=dev, generator=gen) * 1.8 - 0.9, rnd(L, D)
    mu_dev = torch.full((M,), 0.5, dtype=dt, device=dev)
    outs = [dict(gain=new(K, 2, n, M), ff=new(K, 2, M), flag=new(K, M, dtype=torch.uint8), dv=new(K, 2, M), w=new(K, 2, D + 1, N)) for _ in range(2)]
    clamp = new(K, M, dtype=torch.uint8)
    blib, tlib = box.load(), steer.load()

    def args(o, table, boxed):
        w = (p(act), p(obs), al, nal, p(o["w"])) if table else (p(act) if boxed else None, None, None, 0, None)
        head = (C.byref(lay), K, M, p(A), p(B), p(lx), p(lu), q, r)
        tail = (None, p(pv), p(o["gain"]), p(o["ff"]), None, None, p(o["flag"]), p(o["dv"]))
        if boxed:
            return head + (0.0, p(mu_dev), lo, hi) + tail + (p(clamp),) + w + (stream,)
        return head + (p(mu_dev),) + tail + w + (stream,)

    def scale(s):
        for t, t0 in ((lx, lx0), (lu, lu0), (pv, pv0)):
            torch.mul(t0, s, out=t)

    def share(a):
        if blib.os2rb_ilqr_backward_box(*a) != abi.OK:
            raise RuntimeError(blib.os2rb_last_error().decode())
        torch.cuda.synchronize()
        return float((clamp != 0).double().mean())

    for table in (True, False):
        a_theirs, a_ours = args(outs[0], table, False), args(outs[1], table, True)

        def sibling():
            if tlib.os2rt_ilqr_backward_mu(*a_theirs) != abi.OK:
                raise RuntimeError(tlib.os2rt_last_error().decode())

        def boxed():
            if blib.os2rb_ilqr_backward_box(*a_ours) != abi.OK:
                raise RuntimeError(blib.os2rb_last_error().decode())
        for want in ("a third", "none"):
            if want == "none":
                scale(0.0)
                got = share(a_ours)
            else:
                low, high = 1e-4, 1e4
                for _ in range(24):
                    mid = (low * high) ** 0.5
                    scale(mid)
                    got = share(a_ours)
                    if 0.30 <= got <= 0.37:
                        break
                    low, high = (mid, high) if got < 0.30 else (low, mid)
            refused = int(outs[1]["flag"].sum())
            emit(f"K = {K}, M = {M}, {str(dt).split('.')[-1]}, {'table for ' + str(nal) + ' step sizes' if table else 'no table'}, clamped: {want} "
                 f"({100 * got:.1f} % of the knots, {refused} refused)")
            labels = ("os2rt_ilqr_backward_mu: mu_dev = 0.5 everywhere", "os2rb_ilqr_backward_box: the same arrays, box (-1, 1)")
            res = compare(torch, list(zip(labels, (sibling, boxed))), reps, emit)
            moved = (L * (n * n + 2 * n + n + 2) + n * M + M + K * M * (2 * n + 2 + 2)) * esz + K * M
            added = K * M
            if table:
                moved += (L * (2 + D) + K * 2 * (D + 1) * N) * esz
            else:
                added += 2 * L * esz
            verdict(res, labels[0], labels[1], added, moved, emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--knots", type=int, default=50)
    ap.add_argument("--traj", type=int, nargs="+", default=[64, 4096, 16384])
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ilqr_box_rate: no GPU visible; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                   # (kept as it grows: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"os2rb_ilqr_backward_box against os2rt_ilqr_backward_mu on the same arrays; HIP events; {torch.cuda.get_device_name(0)}, "
         f"{time.strftime('%Y-%m-%d')}")
    for dtype in args.dtype:
        sim = make_sim(dtype)
        for M in args.traj:
            measure(torch, sim, args.knots, M, args.reps, emit)
        sim.close()


if __name__ == "__main__":
    main()
