#!/usr/bin/env python3
"""Time per call of os2rx_cem_update (libos2r_cem.so, include/os2r_cem.h) against the batched torch statement of the same update,
in one run.

  python tools/cem_update_rate.py [--shapes 1,256,20 64,256,20 256,256,20 4096,16,50] [--dtype f64 f32] [--reps 5]
                                  [--out profiles/cem_update_rate.txt]

A shape is M robots, S samples per robot, K knots; N = S M lanes, E = max(1, S / 8) elites, D = 10 observation slots (the
free_hip robot's), both gains 1, sigma clamped to [0.05, 1], shift 1 with a zero tail as in the example.  The inputs are random
returns and actions on the device; no simulator handle is needed.  Every path is warmed up with three calls, a ten-call probe
sizes its windows to about 0.3 s (at least 3 calls), and the paths alternate window by window, --reps windows each after one
untimed round: median, min and max per path, HIP events on the current stream.
  device         os2rx_cem_update through ctypes with its arguments built once: nominal_out, var_out, sigma_out and applied
  device+table   the same call with the table [K][2][D+1][N] and lane_sigma [2][N] as well (2 K N + 2 N more words written)
  torch          topk over each robot's samples, gather of the elites' actions from [K][S][M][2], mean, var, sqrt of the mean
                 variance, clamp, the slice and the cat of the shift, with the robot as a batch dimension
  torch+table    the same plus the bias entries of the table and the lane sigma, one indexed assignment each
Reported with each time: the compulsory bytes (returns, actions of the K knots, the nominals, var_out written and read, the
sigmas, applied and, with the table, the bias entries and the lane sigma) over the time, against 8 TB/s.  The same arrays are
read in every call of a window and the largest shape moves about 110 MB, so they are served from the 256 MiB last-level cache,
not from HBM: the figure says how far the call is from the memory system's ceiling, not what HBM delivered.  No ratio is fixed
in advance: the file says what was measured.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ilqr_steer_rate import compare  # noqa: E402

D, SIGMA_MIN, SIGMA_MAX, PEAK = 10, 0.05, 1.0, 8e12


def measure(torch, dtype, M, S, K, reps, emit):
    from gym_os2r_amd import abi, cem, control
    dev = torch.device("cuda:0")
    dt = torch.float64 if dtype == "f64" else torch.float32
    esz = 8 if dtype == "f64" else 4
    N, E = S * M, max(1, S // 8)
    gen = torch.Generator(device=dev).manual_seed(0)
    ret = torch.rand(N, dtype=dt, device=dev, generator=gen) * 10.0
    act = torch.rand(K, N, 2, dtype=dt, device=dev, generator=gen) * 2.0 - 1.0
    new = lambda *s: torch.zeros(*s, dtype=dt, device=dev)
    nom_in, sig_in = new(K, M, 2), torch.full((2, M), 0.4, dtype=dt, device=dev)
    outs = [dict(nominal=new(K, M, 2), var=new(K, M, 2), sigma=new(2, M), applied=new(M, 2), table=new(K, 2, D + 1, N), lane=new(2, N))
            for _ in range(2)]
    t_table, t_lane = new(K, 2, D + 1, N), new(2, N)
    lib = cem.load()
    lay = control.layout(abi.F64 if dtype == "f64" else abi.F32, 5, 0, [-1] * D)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def args(o, table):
        return (C.byref(lay), K, M, S, E, p(ret), p(act), p(nom_in), p(sig_in), 1.0, 1.0, SIGMA_MIN, SIGMA_MAX, 1, cem.TAIL_ZERO,
                p(o["nominal"]), p(o["var"]), p(o["sigma"]), p(o["applied"]), p(o["table"]) if table else None,
                p(o["lane"]) if table else None, None, None, None, stream)
    a_plain, a_table = args(outs[0], False), args(outs[1], True)

    def device(a):
        def fn():
            if lib.os2rx_cem_update(*a) != abi.OK:
                raise RuntimeError(lib.os2rx_last_error().decode())
        return fn
    lane_robot = torch.arange(N, device=dev) % M
    zero_tail = new(1, M, 2)
    kept = {}

    def torch_update(table):
        def fn():
            top = torch.topk(ret.view(S, M), E, dim=0).indices                                             # [E, M]
            elite = torch.gather(act.view(K, S, M, 2), 1, top[None, :, :, None].expand(K, E, M, 2))        # [K, E, M, 2]
            mean = elite.mean(1).clamp(-1.0, 1.0)
            var = elite.var(1, unbiased=False)
            kept["sigma"] = var.mean(0).sqrt().clamp(SIGMA_MIN, SIGMA_MAX).t()                             # [2, M]
            kept["applied"] = mean[0]
            kept["nominal"] = torch.cat([mean[1:], zero_tail])
            if table:
                t_table[:, :, D, :] = kept["nominal"].permute(0, 2, 1)[:, :, lane_robot]
                t_lane[:] = kept["sigma"][:, lane_robot]
        return fn
    device(a_plain)(), device(a_table)(), torch_update(True)()
    torch.cuda.synchronize()
    tol = 1e-12 if dtype == "f64" else 1e-5
    for name in ("nominal", "var", "sigma", "applied"):
        assert torch.equal(outs[0][name], outs[1][name]), name
    for name in ("nominal", "sigma", "applied"):
        assert float((outs[1][name] - kept[name]).abs().max()) < tol, f"the device update and the torch statements disagree: {name}"
    assert float((outs[1]["table"] - t_table).abs().max()) < tol and float((outs[1]["lane"] - t_lane).abs().max()) < tol
    emit(f"M = {M} robots, S = {S} samples, E = {E} elites, K = {K} knots, N = {N} lanes, {str(dt).split('.')[-1]}")
    labels = ("torch: topk, gather, mean, var, sqrt, clamp, cat", "torch+table: ... and the bias entries and the lane sigma",
              "device: os2rx_cem_update", "device+table: os2rx_cem_update")
    res = compare(torch, list(zip(labels, (torch_update(False), torch_update(True), device(a_plain), device(a_table)))), reps, emit)
    plain = (N + K * N * 2 + 4 * K * M * 2 + 2 * 2 * M + M * 2) * esz
    for label, nbytes in ((labels[2], plain), (labels[3], plain + (K * 2 * N + 2 * N) * esz)):
        med = res[label][0]
        emit(f"  {label.split(':')[0]}: {nbytes / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes / (med * 1e-3) / 1e9:.1f} GB/s, "
             f"{100 * nbytes / (med * 1e-3) / PEAK:.2f} % of 8 TB/s")
    for ours, theirs in ((labels[2], labels[0]), (labels[3], labels[1])):
        emit(f"  {theirs.split(':')[0]} / {ours.split(':')[0]}: {res[theirs][0] / res[ours][0]:.2f}")
    emit(f"  the table and the lane sigma cost the device call {res[labels[3]][0] - res[labels[2]][0]:+.4f} ms, the torch statements "
         f"{res[labels[1]][0] - res[labels[0]][0]:+.4f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1,256,20", "64,256,20", "256,256,20", "4096,16,50"], help="M,S,K")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cem_update_rate: no GPU visible; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                   # (kept as it grows: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"os2rx_cem_update against the batched torch statement of the same update; HIP events; "
         f"{torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    for dtype in args.dtype:
        for shape in args.shapes:
            M, S, K = (int(v) for v in shape.split(","))
            measure(torch, dtype, M, S, K, args.reps, emit)


if __name__ == "__main__":
    main()
