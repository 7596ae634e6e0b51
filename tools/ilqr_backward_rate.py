#!/usr/bin/env python3
"""Time per backward pass of os2rc_ilqr_backward (include/os2r_control.h) against os2r_lqr_gains at the same size and against the
batched torch loop of the textbook recursion, on identical inputs.

  python tools/ilqr_backward_rate.py [--size 50 16384] [--dtype f64] [--reps 5] [--out profiles/ilqr_backward_rate.txt]    (knots trajectories)

The free_hip robot (nq 5, n = 10, D = 10 raw observation slots: Monopod-nonorm-balance-v1's layout) and the synthetic inputs of
tools/lqr_gains_rate.py -- A = I + 0.3 N(0,1) / sqrt(n), B = 0.5 N(0,1), an SPD Q with a zero first row and column,
R = [[.1, .02], [.02, .2]] -- plus gradients lx = N(0,1), lu = 0.3 N(0,1), p_final = N(0,1).
Paths, each timed with HIP events on the current stream, alternating within one process --reps times after one untimed round
(median, min and max per path):
  ilqr      sim.ilqr_backward_into(...), mu = 0: one launch writing gains, ff, flags, dv and the weight table of ONE step size
            (what lqr_gains writes, plus the affine outputs); caller-owned outputs, nothing allocated
  ilqr x4   the same with mu = 0.5 and the table of four step sizes (examples/ilqr_balancing.py's call: four times the table)
  lqr       sim.lqr_gains_into(...), sweeps = 1: gains, flags and the weight table -- the merged kernel
  torch     per knot k = -(Quu + mu I)^-1 Qu, Kf = -(Quu + mu I)^-1 Qux, Vx, Vxx symmetrised (mu = 0.5), batched over the
            trajectories; its inputs are [K, M, n, n] copies made once, outside the window; it writes no table
The device paths' windows hold as many calls as fit about 0.3 s (at least 3); the torch loop is one pass per window.  Before
anything is timed the kernel's gains, ff and value gradient are compared with the loop's (they differ by rounding).
Operations are counted from the shapes: os2r_lqr_gains' knot does n^2 (n + 2) + 2 n (n + 2) + n^2 (n + 1) / 2 multiply-adds
(1 990 at n = 10); this kernel adds n (n + 2) for Qx and Qu, 4 n for p' and a dozen for k and dv (2 162), and with mu != 0
another 3 n (n + 1) / 2 + 3 n (2 357): a tenth to a fifth more.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lqr_gains_rate import make_sim, window  # noqa: E402


def measure(torch, sim, K, M, reps, emit):
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
    lx, lu, pf = rnd(n, L), 0.3 * rnd(2, L), rnd(n, M)
    new = lambda *s: torch.empty(*s, dtype=dt, device=dev)
    gains, ff, dv, pout, flags = new(K, 2, n, M), new(K, 2, M), new(K, 2, M), new(n, M), torch.empty(K, M, dtype=torch.uint8, device=dev)
    table1, table4 = new(K, 2, D + 1, M), new(K, 2, D + 1, 4 * M)
    mu = 0.5

    def ilqr():
        sim.ilqr_backward_into(A, B, Q, R, knots=K, lx=lx, lu=lu, mu=0.0, p_final=pf, gains_out=gains, ff_out=ff, flags_out=flags, dv_out=dv,
                               actions=actions, obs=obs, alphas=(1.0,), weights_out=table1)

    def ilqr4():
        sim.ilqr_backward_into(A, B, Q, R, knots=K, lx=lx, lu=lu, mu=mu, p_final=pf, gains_out=gains, ff_out=ff, p_out=pout, flags_out=flags,
                               dv_out=dv, actions=actions, obs=obs, alphas=(1.0, 0.5, 0.25, 0.125), weights_out=table4)

    def lqr():
        sim.lqr_gains_into(A, B, Q, R, knots=K, sweeps=1, gains_out=gains, flags_out=flags, actions=actions, obs=obs, weights_out=table1)

    At = A.view(n, n, K, M).permute(2, 3, 0, 1).contiguous()
    Bt = B.view(n, 2, K, M).permute(2, 3, 0, 1).contiguous()
    lxt, lut = lx.view(n, K, M).permute(1, 2, 0).contiguous(), lu.view(2, K, M).permute(1, 2, 0).contiguous()
    Qd, Rd, I2 = Q.to(dev, dt), R.to(dev, dt), torch.eye(2, dtype=dt, device=dev)

    def loop():
        P, p = Qd.expand(M, n, n), pf.T
        Ks, ks = [None] * K, [None] * K
        for k in range(K - 1, -1, -1):
            Ak, Bk = At[k], Bt[k]
            Akt, Bkt = Ak.transpose(1, 2), Bk.transpose(1, 2)
            Qx, Qu = lxt[k] + (Akt @ p[:, :, None])[:, :, 0], lut[k] + (Bkt @ p[:, :, None])[:, :, 0]
            Quu, Qux = Rd + Bkt @ P @ Bk, Bkt @ P @ Ak
            sol = torch.linalg.solve(Quu + mu * I2, torch.cat([Qu[:, :, None], Qux], 2))
            kf, Kf = -sol[:, :, 0], -sol[:, :, 1:]
            Kft, Quxt = Kf.transpose(1, 2), Qux.transpose(1, 2)
            p = Qx + (Kft @ (Quu @ kf[:, :, None] + Qu[:, :, None]))[:, :, 0] + (Quxt @ kf[:, :, None])[:, :, 0]
            P = Qd + Akt @ P @ Ak + Kft @ Quu @ Kf + Kft @ Qux + Quxt @ Kf
            P = 0.5 * (P + P.transpose(1, 2))
            Ks[k], ks[k] = Kf, kf
        return Ks, ks, p

    ilqr4()
    Ks, ks, p = loop()
    torch.cuda.synchronize()
    refK, refk = -torch.stack(Ks), torch.stack(ks)                         # [K, M, 2, n], [K, M, 2]
    rel = lambda got, ref: float((got - ref).abs().max() / ref.abs().max())
    emit(f"K = {K}, M = {M}, {str(dt).split('.')[-1]}; {int(flags.sum())} knots refused at mu = {mu}; largest differences from the torch loop, "
         f"relative to the largest entry: gains {rel(gains.permute(0, 3, 1, 2), refK):.2e}, ff {rel(ff.permute(0, 2, 1), refk):.2e}, "
         f"p {rel(pout.T, p):.2e}")
    cases = [("ilqr: one launch, mu = 0, one step size", ilqr), ("ilqr x4: mu = 0.5, four step sizes", ilqr4),
             ("lqr: one os2r_lqr_gains launch", lqr)]
    cases = [(label, fn, max(3, min(200, int(300.0 / max(window(torch, fn, 1), 1e-3))))) for label, fn in cases]
    cases.append(("torch: the textbook loop, mu = 0.5", loop, 1))
    times = {c[0]: [] for c in cases}
    for rep in range(reps + 1):                      # round 0 is the warm-up of every path
        for label, fn, c in cases:
            ms = window(torch, fn, c)
            if rep:
                times[label].append(ms)
    med = {}
    for label, _, c in cases:
        t = sorted(times[label])
        med[label] = t[len(t) // 2]
        emit(f"  {label:<42} {med[label]:10.3f} ms per pass  (min {t[0]:.3f}, max {t[-1]:.3f}; {c} per window, {reps} windows)")
    i1, i4, l_, t_ = (c[0] for c in cases)

    def ratio(what, num, den):
        r = sorted(a / b for a in times[num] for b in times[den])
        emit(f"  {what:<42} {med[num] / med[den]:10.2f} x  (over all pairs of windows: {r[0]:.2f} .. {r[-1]:.2f})")
        return med[num] / med[den]
    r1 = ratio("ilqr / lqr", i1, l_)
    r4 = ratio("ilqr x4 / lqr", i4, l_)
    rt = ratio("torch / ilqr x4", t_, i4)
    fma = n * n * (n + 2) + 2 * n * (n + 2) + n * n * (n + 1) // 2
    fma1 = fma + n * (n + 2) + 4 * n + 12
    fma4 = fma1 + 3 * n * (n + 1) // 2 + 3 * n
    esz = A.element_size()
    read = (n * n + 2 * n + n + 2) * esz * L + (2 + D) * esz * L
    for label, f, nal in ((i1, fma1, 1), (i4, fma4, 4)):
        wrote = (2 * n + 2 + 2 + 2 * (D + 1) * nal) * esz * L + L
        emit(f"  {label.split(':')[0]}: {L / med[label] * 1e-6:.2f} G knot-trajectories / s; {(read + wrote) / med[label] * 1e-6:.1f} GB/s of compulsory "
             f"traffic; {2 * f * L / med[label] * 1e-9:.2f} TFLOP/s counting {f} multiply-adds per knot ({f / fma:.2f} x os2r_lqr_gains' {fma})")
    emit("the launch is faster than the torch loop: " + ("yes" if rt >= 1.0 else "NO"))
    emit("the launch takes at most twice os2r_lqr_gains: " + ("yes" if max(r1, r4) <= 2.0 else "NO"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[50, 16384], metavar=("K", "M"))
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ilqr_backward_rate: no GPU visible; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"os2rc_ilqr_backward against os2r_lqr_gains and the torch loop, time per backward pass over HIP events; "
         f"{torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    for dtype in args.dtype:
        sim = make_sim(dtype)
        measure(torch, sim, args.size[0], args.size[1], args.reps, emit)
        sim.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
