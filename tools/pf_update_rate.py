#!/usr/bin/env python3
"""Time per call of os2rp_pf_update (libos2r_pf.so, include/os2r_pf.h) against the torch statements of the same particle-filter
update with the robot as a batch dimension, in one run.

  python tools/pf_update_rate.py [--shapes 1,1024,10 64,256,10 4096,64,10 16384,16,10] [--dtype f64 f32] [--reps 5]
                                 [--out profiles/pf_update_rate.txt]

A shape is M robots, S particles per robot, D observation entries; N = S M lanes.  The inputs are random observations about a
random measurement, random log-weights and offsets on the device; no simulator handle is needed.  Every path is warmed up with
three calls, a ten-call probe sizes its windows to about 0.3 s (at least 3 calls), and the paths alternate window by window,
--reps windows each after one untimed round: median, min and max per path, HIP events on the current stream.
  device         os2rp_pf_update through ctypes with its arguments built once: logw_out, index, est, ess, count and resampled
  torch          the difference, its square, the precision-weighted sum, logsumexp, exp, the weighted mean, the effective sample
                 size, cumsum, searchsorted, where and arange: about fifteen statements, a launch or more each
Both are timed twice: with resample_ratio = 2, where every robot resamples, and with resample_ratio = 0 on valid particles,
where none does.
Reported with each device time: the compulsory bytes (obs, meas, logw_in and u read; logw_out, index, est, ess, count and
resampled written) over the time, against 8 TB/s.  The same arrays are read in every call of a window and the largest shape
moves about 27 MB, so they are served from the 256 MiB last-level cache, not from HBM: the figure says how far the call is from
the memory system's ceiling, not what HBM delivered.  No ratio is fixed in advance: the file says what was measured.
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

PEAK = 8e12


def measure(torch, dtype, M, S, D, reps, emit):
    from gym_os2r_amd import abi, control, pf
    dev = torch.device("cuda:0")
    dt = torch.float64 if dtype == "f64" else torch.float32
    esz = 8 if dtype == "f64" else 4
    N = S * M
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, dtype=dt, device=dev, generator=gen)
    meas = rnd(M, D)
    obs = (meas[None] + 0.5 * rnd(S, M, D)).reshape(N, D).contiguous()
    prec = torch.rand(D, dtype=dt, device=dev, generator=gen) + 0.5
    logw = -torch.rand(S, M, dtype=dt, device=dev, generator=gen)
    u = torch.rand(M, dtype=dt, device=dev, generator=gen)
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    i32 = torch.int32
    out = dict(logw=new(S, M), index=new(N, dtype=i32), est=new(M, D), ess=new(M), count=new(M, dtype=i32), res=new(M, dtype=i32))
    lib = pf.load()
    lay = control.layout(abi.F64 if dtype == "f64" else abi.F32, 5, 0, [-1] * D)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def device(ratio):
        a = (C.byref(lay), M, S, p(obs), p(meas), p(prec), p(logw), p(u), ratio, p(out["logw"]), p(out["index"]), p(out["est"]), None,
             p(out["ess"]), p(out["count"]), p(out["res"]), stream)

        def fn():
            if lib.os2rp_pf_update(*a) != abi.OK:
                raise RuntimeError(lib.os2rp_last_error().decode())
        return fn
    robots = torch.arange(M, device=dev)
    slots = torch.arange(S, device=dev, dtype=dt)[:, None]
    minus_inf = torch.full((), float("-inf"), dtype=dt, device=dev)
    kept = {}

    def torch_update(ratio):
        def fn():
            o = obs.view(S, M, D)
            d = o - meas
            l = logw - 0.5 * (d * d * prec).sum(-1)
            valid = torch.isfinite(l)
            lm = torch.where(valid, l, minus_inf)
            w = torch.exp(lm - torch.logsumexp(lm, 0))
            kept["est"] = torch.einsum("sm,smd->md", w, o)
            kept["ess"] = 1.0 / (w * w).sum(0)
            kept["count"] = valid.sum(0)
            res = (kept["ess"] < ratio * S) | (kept["count"] < S)
            kept["res"] = res
            c = torch.cumsum(w, 0)
            t = (slots + u) / S
            a = torch.searchsorted(c.t().contiguous(), t.t().contiguous(), right=True).clamp_(max=S - 1)
            kept["index"] = torch.where(res[None], a.t() * M + robots, -1).to(torch.int32).reshape(-1)
            kept["logw"] = torch.where(res[None], 0.0, lm - lm.max(0).values)
        return fn
    tol = 1e-10 if dtype == "f64" else 1e-4
    for ratio in (2.0, 0.0):
        device(ratio)(), torch_update(ratio)()
        torch.cuda.synchronize()
        assert float((out["est"] - kept["est"]).abs().max()) < tol * 10 and torch.equal(out["res"] != 0, kept["res"]), \
            "the device update and the torch statements disagree"
        assert float((out["logw"] - kept["logw"]).abs().max()) < tol * 100 and torch.equal(out["count"].long(), kept["count"])
        same = float((out["index"] == kept["index"]).double().mean())
        assert same > 0.99, f"the indices agree in {same:.4f} of the lanes only"
    emit(f"M = {M} robots, S = {S} particles, D = {D}, N = {N} lanes, {str(dt).split('.')[-1]}")
    labels = ("torch, every robot resamples: logsumexp, cumsum, searchsorted ...", "torch, no robot resamples", "device, every robot resamples: os2rp_pf_update",
              "device, no robot resamples: os2rp_pf_update")
    res = compare(torch, list(zip(labels, (torch_update(2.0), torch_update(0.0), device(2.0), device(0.0)))), reps, emit)
    nbytes = (N * D + M * D + N + M + N + M * D + M) * esz + (N + 2 * M) * 4
    for label in labels[2:]:
        med = res[label][0]
        emit(f"  {label.split(':')[0]}: {nbytes / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes / (med * 1e-3) / 1e9:.1f} GB/s, "
             f"{100 * nbytes / (med * 1e-3) / PEAK:.2f} % of 8 TB/s")
    for ours, theirs in ((labels[2], labels[0]), (labels[3], labels[1])):
        emit(f"  {theirs.split(':')[0]} / {ours.split(':')[0]}: {res[theirs][0] / res[ours][0]:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1,1024,10", "64,256,10", "4096,64,10", "16384,16,10"], help="M,S,D")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pf_update_rate: no GPU visible; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                   # (kept as it grows: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"os2rp_pf_update against the torch statements of the same update with the robot as a batch dimension; HIP events; "
         f"{torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    for dtype in args.dtype:
        for shape in args.shapes:
            M, S, D = (int(v) for v in shape.split(","))
            measure(torch, dtype, M, S, D, args.reps, emit)


if __name__ == "__main__":
    main()
