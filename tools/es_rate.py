#!/usr/bin/env python3
"""Time per call of HipSim.es_perturb_into and HipSim.es_update_into (libos2r_es.so, include/os2r_es.h) against the torch
statements of examples/ars_balancing.py with the population as a batch dimension, in one run.

  python tools/es_rate.py [--shapes 1,4096 1,32768 64,256 4096,8] [--dtype f64 f32] [--reps 5] [--out profiles/es_rate.txt]

A shape is M populations and S directions each; N = 2 S M lanes, D = 10 observation slots (the free_hip robot's), E = 22 entries
of one policy.  theta ~ N(0, 0.3) and the returns ~ N(0, 1) are random on the device; a small handle of the free_hip robot is made
for its methods alone.  Every path is warmed up with three calls, a ten-call probe sizes its windows to about 0.3 s (at least 3
calls), and the paths alternate window by window, --reps windows each after one untimed round: median, min and max per path, HIP
events on the current stream.  Each shape is measured with top = 0 (every direction) and top = S / 4.
  perturb, torch    randn [S, M, E], cat of theta + nu delta and theta - nu delta
  perturb, device   es_perturb_into without delta, its tensors made once
  update, torch     on a delta tensor that was kept from the perturbation: (top: topk of max(r+, r-), gather of the returns and of
                    delta), std, einsum, the step
  update, device    es_update_into with grad, its tensors made once; it reads no delta
Reported with the device times: the compulsory bytes -- the perturbation reads theta and writes the weights; the update reads the
returns and theta and writes theta_new, grad, sigma_r, count, used and kept -- over the time, against 8 TB/s.  No ratio is fixed
in advance: the file says what was measured.
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

D, NU, STEP, FLOOR, GENERATION, PEAK = 10, 0.03, 0.02, 1e-8, 3, 8e12


def measure(torch, sim, M, S, reps, emit):
    dev, dt = sim.device, sim.dtype
    esz = 8 if dt == torch.float64 else 4
    SM, N, E, i32 = S * M, 2 * S * M, 2 * (D + 1), torch.int32
    gen = torch.Generator(device=dev).manual_seed(0)
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    theta = torch.randn(M, 2, D + 1, dtype=dt, device=dev, generator=gen) * 0.3
    returns = torch.randn(N, dtype=dt, device=dev, generator=gen)
    weights, delta = new(N, 2, D + 1), new(SM, 2, D + 1)
    theta_new, grad, sigma_r = new(M, 2, D + 1), new(M, 2, D + 1), new(M)
    count, used, kept, score = new(M, dtype=i32), new(M, dtype=i32), new(SM, dtype=i32), new(SM)
    held = {}
    sim.es_perturb_into(theta, weights, directions=S, nu=NU, generation=GENERATION, delta=delta)
    stored = delta.view(S, M, E)                            # what the torch update reads: the directions, kept from the perturbation
    flat = theta.view(M, E)

    def device_perturb():
        sim.es_perturb_into(theta, weights, directions=S, nu=NU, generation=GENERATION)

    def torch_perturb():
        d = torch.randn(S, M, E, dtype=dt, device=dev, generator=gen)
        held["weights"] = torch.cat([flat + NU * d, flat - NU * d])

    def device_update(top):
        return lambda: sim.es_update_into(returns, theta, theta_new, sigma_r, count, used, kept, directions=S, generation=GENERATION,
                                          step_size=STEP, top=top, sigma_floor=FLOOR, grad=grad, score=score)

    def torch_update(top):
        def run():
            rp, rm = returns[:SM].view(S, M), returns[SM:].view(S, M)
            d, b = stored, S
            if 0 < top < S:
                b = top
                idx = torch.maximum(rp, rm).topk(b, dim=0).indices                      # [b, M]
                rp, rm = rp.gather(0, idx), rm.gather(0, idx)
                d = stored.gather(0, idx.unsqueeze(-1).expand(b, M, E))
            sigma = torch.cat([rp, rm]).std(0, unbiased=False).clamp_min(FLOOR)
            held["theta_new"] = flat + (STEP / (b * sigma)).unsqueeze(-1) * torch.einsum("sm,sme->me", rp - rm, d)
        return run

    emit(f"M = {M} populations, S = {S} directions, N = {N} lanes, D = {D}, {str(dt).split('.')[-1]}")
    tol = 1e-9 if dt == torch.float64 else 1e-3             # (both paths sum S terms in the dtype, in different orders)
    labels = ("perturb, torch: randn, cat", "perturb, device: es_perturb_into")
    res = compare(torch, list(zip(labels, (torch_perturb, device_perturb))), reps, emit)
    med = res[labels[1]][0]
    nbytes = (M * E + N * E) * esz
    emit(f"  perturb, device: {nbytes / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes / (med * 1e-3) / 1e9:.1f} GB/s, "
         f"{100 * nbytes / (med * 1e-3) / PEAK:.2f} % of 8 TB/s;  torch / device: {res[labels[0]][0] / med:.2f}")
    for top in (0, max(1, S // 4)):
        dev_fn, torch_fn = device_update(top), torch_update(top)
        dev_fn()
        torch_fn()
        torch.cuda.synchronize()
        far = float((theta_new.view(M, E) - held["theta_new"]).abs().max()) / float(held["theta_new"].abs().max())
        assert far < tol, f"the device call and the torch statement disagree: {far}"
        assert int(count.sum()) == SM and int(used.sum()) == (top if 0 < top < S else S) * M
        what = "topk, gather, std, einsum" if 0 < top < S else "std, einsum"
        labels = (f"update top = {top}, torch: {what}", f"update top = {top}, device: es_update_into")
        res = compare(torch, list(zip(labels, (torch_fn, dev_fn))), reps, emit)
        med = res[labels[1]][0]
        nbytes = (N + 3 * M * E + M) * esz + 2 * M * 4 + SM * 4
        emit(f"  update top = {top}, device: {nbytes / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes / (med * 1e-3) / 1e9:.1f} GB/s, "
             f"{100 * nbytes / (med * 1e-3) / PEAK:.3f} % of 8 TB/s;  torch / device: {res[labels[0]][0] / med:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1,4096", "1,32768", "64,256", "4096,8"], help="M,S")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("es_rate: no GPU visible; nothing is measured without one")
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

    emit(f"HipSim.es_perturb_into and HipSim.es_update_into against the torch statements of the example; HIP events; "
         f"{torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    for dtype in args.dtype:
        sim = HipSim(make_config("free_hip", "BalancingV2", False, num_envs=4, contact=True, seed=1,
                                 dtype=abi.F64 if dtype == "f64" else abi.F32)[0])
        assert sim.D == D
        for shape in args.shapes:
            M, S = (int(v) for v in shape.split(","))
            measure(torch, sim, M, S, args.reps, emit)
            torch.cuda.empty_cache()
        sim.close()


if __name__ == "__main__":
    main()
