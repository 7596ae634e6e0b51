#!/usr/bin/env python3
"""Time per call of HipSim.obs_stats_into, HipSim.norm_fold_into and HipSim.norm_unfold_into (libos2r_norm.so,
include/os2r_norm.h) against their torch statements and, for the statistics, against HipSim.value_fit_into on the same arrays,
in one run.

  python tools/norm_rate.py [--shapes 1,8192,500 1,65536,50 64,256,50 4096,16,50 65536,1,50] [--dtype f64 f32] [--reps 5]
                            [--out profiles/norm_rate.txt]

A shape is P policies, S samples each and K steps; N = S P lanes, D = 10 observation slots (the free_hip robot's).  The
observations are random on the device with a mean of up to 50 and a deviation between 0.1 and 5 per policy and component, the
lengths uniform in 1..K, the running state that of an earlier batch; a small handle of the free_hip robot is made for its methods
alone.  Every path is warmed up with three calls, a ten-call probe sizes its windows to about 0.3 s (at least 3 calls), and the
paths alternate window by window, --reps windows each after one untimed round: median, min and max per path, HIP events on the
current stream.
  stats, torch      the batched statement of the same merge: the mask of the counted steps, masked sum, mean, squared
                    deviations about it, Chan's formula; on x_k = obs[k] (a null obs0), so that no path copies the batch
  stats, device     obs_stats_into, its tensors made once
  stats, value_fit  value_fit_into on the same observations and lengths: its lane launch moves 77 sums a lane where this one
                    moves 20
  fold, torch       r = 1 / clamp(sqrt(m2 / count), floor); W = theta r; b = theta_D - sum W mean; cat -- one set per lane
  fold, device      norm_fold_into with lanes = N
  unfold, torch     (g - g_D mean) r; cat -- per policy, in the gradient's [2, D+1, P] layout
  unfold, device    norm_unfold_into with policy_fastest
Reported with the device time of the statistics: the compulsory bytes -- the observations and lengths read, the state read and
written -- and the scratch bytes (the lane sums and counts, written by one launch and read by the next), over the time, against
8 TB/s.  A torch path that beats its device path is marked LOSS.  No ratio is fixed in advance: the file says what was measured.
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

D, FLOOR, PEAK = 10, 1e-6, 8e12


def ratio(res, yard, label):
    r = res[yard][0] / res[label][0]
    return f"{yard.split(':')[0]} / {label.split(':')[0]}: {r:.2f}" + ("  LOSS" if r < 1.0 else "")


def measure(torch, sim, P, S, K, reps, emit):
    from gym_os2r_amd import critic
    dev, dt = sim.device, sim.dtype
    esz = 8 if dt == torch.float64 else 4
    N, i32, i64 = S * P, torch.int32, torch.int64
    gen = torch.Generator(device=dev).manual_seed(0)
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    rnd = lambda *s: torch.rand(*s, dtype=dt, device=dev, generator=gen)
    mu, sd = 100 * rnd(P, D) - 50, 0.1 + 4.9 * rnd(P, D)
    obs = torch.randn(K, S, P, D, dtype=dt, device=dev, generator=gen).mul_(sd).add_(mu).view(K, N, D)
    obs0 = (torch.randn(S, P, D, dtype=dt, device=dev, generator=gen) * sd + mu).view(N, D)
    length = torch.randint(1, K + 1, (N,), device=dev, generator=gen).to(i32)
    target = torch.randn(K, N, dtype=dt, device=dev, generator=gen)
    state = (torch.full((P,), 5 * S * K, dtype=i64, device=dev), mu + 0.01 * sd, sd * sd * 5 * S * K)
    count, mean, m2, steps, valid = new(P, dtype=i64), new(P, D), new(P, D), new(P, dtype=i32), new(P, dtype=i32)
    lane_sum, lane_count = new(2 * D, N), new(2, N, dtype=i32)
    E = critic.moments(D)
    w, lane_mom, mom, fit_count = new(D + 1, P), new(E, N), new(E, P), new(critic.LANE_COUNTS, N, dtype=i32)
    held = {}
    ks = torch.arange(K, device=dev).view(K, 1)

    def device_stats():
        sim.obs_stats_into(obs, count, mean, m2, lane_sum, lane_count, policies=P, length=length, state=state, steps=steps, valid=valid)

    def torch_stats():
        m = (ks < length.view(1, N)).view(K, S, P, 1)
        x = obs.view(K, S, P, D)
        nb = m.sum((0, 1)).to(dt)                                                     # [P, 1]
        meanb = (x * m).sum((0, 1)) / nb
        dv = (x - meanb) * m
        m2b = (dv * dv).sum((0, 1))
        na = state[0].to(dt).view(P, 1)
        nt = na + nb
        delta = meanb - state[1]
        held["mean"] = state[1] + delta * (nb / nt)
        held["m2"] = state[2] + m2b + delta * delta * (na * nb / nt)
        held["count"] = state[0] + nb.view(P).to(i64)

    def fit():
        sim.value_fit_into(obs, target, w, lane_mom, mom, fit_count, obs0=obs0, policies=P, length=length, ridge=1e-3)

    name = str(dt).split(".")[-1]
    emit(f"P = {P} policies, S = {S} samples, K = {K} steps, N = {N} lanes, D = {D}, {name}")
    device_stats()
    torch_stats()
    torch.cuda.synchronize()
    std = (held["m2"] / held["count"].view(P, 1).to(dt)).sqrt()
    far_mean = float(((mean - held["mean"]).abs() / std).max())
    far_var = float(((m2 - held["m2"]).abs() / held["m2"]).max())
    tol = 1e-9 if dt == torch.float64 else 2e-3                # (the torch statement sums in another order, and about another pivot)
    assert torch.equal(count, held["count"]) and far_mean < tol and far_var < tol, f"the device call and the torch statement disagree: {far_mean}, {far_var}"
    labels = ("stats, torch: mask, sum, mean, deviations, Chan", "stats, device: obs_stats_into", "stats, value_fit: value_fit_into")
    res = compare(torch, list(zip(labels, (torch_stats, device_stats, fit))), reps, emit)
    med = res[labels[1]][0]
    nbytes = K * N * D * esz + N * 4 + 2 * P * (8 + 2 * D * esz)
    scratch = 2 * (2 * D * N * esz + 2 * N * 4)
    emit(f"  stats, device: {nbytes / 1e6:.3f} MB compulsory (+ {scratch / 1e6:.3f} MB of scratch written and read) in {med:.4f} ms = "
         f"{nbytes / (med * 1e-3) / 1e12:.3f} TB/s, {100 * nbytes / (med * 1e-3) / PEAK:.2f} % of 8 TB/s;  {ratio(res, labels[0], labels[1])};  "
         f"{ratio(res, labels[2], labels[1])}")

    theta, weights = torch.randn(N, 2, D + 1, dtype=dt, device=dev, generator=gen), new(N, 2, D + 1)
    grad, grad_theta = torch.randn(2, D + 1, P, dtype=dt, device=dev, generator=gen), new(2, D + 1, P)
    floor = torch.tensor(FLOOR, dtype=dt, device=dev)

    def device_fold():
        sim.norm_fold_into(theta, state, weights, lanes=N)

    def torch_fold():
        r = 1.0 / torch.maximum((state[2] / state[0].view(P, 1).to(dt)).sqrt(), floor)
        t = theta.view(S, P, 2, D + 1)
        W = t[..., :D] * r.view(1, P, 1, D)
        held["weights"] = torch.cat([W, (t[..., D] - (W * state[1].view(1, P, 1, D)).sum(-1)).unsqueeze(-1)], dim=-1)

    def device_unfold():
        sim.norm_unfold_into(grad, state, grad_theta, policy_fastest=True)

    def torch_unfold():
        r = 1.0 / torch.maximum((state[2] / state[0].view(P, 1).to(dt)).sqrt(), floor)
        held["grad_theta"] = torch.cat([(grad[:, :D] - grad[:, D:] * state[1].t()) * r.t(), grad[:, D:]], dim=1)

    device_fold(), torch_fold(), device_unfold(), torch_unfold()
    torch.cuda.synchronize()
    tol = 1e-11 if dt == torch.float64 else 1e-3
    assert float((weights.view(S, P, 2, D + 1) - held["weights"]).abs().max()) / float(held["weights"].abs().max()) < tol
    assert float((grad_theta - held["grad_theta"]).abs().max()) / float(held["grad_theta"].abs().max()) < tol
    labels = ("fold, torch: sqrt, clamp, mul, sum, cat", "fold, device: norm_fold_into, per lane")
    res = compare(torch, list(zip(labels, (torch_fold, device_fold))), reps, emit)
    emit(f"  {ratio(res, labels[0], labels[1])}")
    labels = ("unfold, torch: sqrt, clamp, mul, cat", "unfold, device: norm_unfold_into")
    res = compare(torch, list(zip(labels, (torch_unfold, device_unfold))), reps, emit)
    emit(f"  {ratio(res, labels[0], labels[1])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1,8192,500", "1,65536,50", "64,256,50", "4096,16,50", "65536,1,50"], help="P,S,K")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("norm_rate: no GPU visible; nothing is measured without one")
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

    emit(f"HipSim.obs_stats_into, norm_fold_into and norm_unfold_into against their torch statements and value_fit_into; HIP events; "
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
