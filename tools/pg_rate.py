#!/usr/bin/env python3
"""Time per call of HipSim.policy_gradient_into (libos2r_pg.so, include/os2r_pg.h) against the torch statements of
examples/reinforce_balancing.py for the same gradient, in one run.

  python tools/pg_rate.py [--shapes 1,8192,500 1,65536,50 64,256,50 4096,16,50 65536,1,50] [--dtype f64 f32] [--reps 5]
                          [--out profiles/pg_rate.txt]

A shape is P policies, S samples per policy, K steps; N = S P lanes, D = 10 observation slots (the free_hip robot's).  The inputs
are random on the device -- observations, noise, actions clipped to [-1, 1], rewards, done bytes with probability 0.01, lengths
between K / 2 and K --; a small handle of the free_hip robot is made for its methods alone.  Every path is warmed up with three
calls, a ten-call probe sizes its windows to about 0.3 s (at least 3 calls), and the paths alternate window by window, --reps
windows each after one untimed round: median, min and max per path, HIP events on the current stream.  Both weightings:
  return         one number per lane (adv)
    torch        the example's five statements -- the cat that shifts the observation record by one, the mask (here from the
                 lengths), the coefficient tensor, the einsum, the sum for the bias --, the policy as a batch dimension
    device       policy_gradient_into with grad, lane_grad, lane_count, steps, clipped and valid, its tensors made once
  reward-to-go   gamma = 0.97 with a baseline [K, P]
    torch        a reverse loop over the steps for G, then the statements above with G - baseline in the coefficient
    device       the same call with rewards, done, gamma and baseline
Reported with each device time: the compulsory bytes -- of the counted steps the observations, noise and actions, with rewards
those, the done bytes and the baseline, else adv; obs0, the lengths, sigma; lane_grad and lane_count written and read again, the
P-sized outputs -- over the time, against 8 TB/s.  The largest shapes move about 500 MB a call, more than the 256 MiB last-level
cache holds: there the figure is close to what HBM delivered; the small ones are served from the cache.  With each path: torch's
peak allocated memory over one call, above what the inputs and outputs hold.  No ratio is fixed in advance: the file says what
was measured.
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

D, GAMMA, PEAK = 10, 0.97, 8e12


def measure(torch, sim, P, S, K, reps, emit):
    dev, dt = sim.device, sim.dtype
    esz = 8 if dt == torch.float64 else 4
    N = S * P
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, dtype=dt, device=dev, generator=gen)
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    obs, obs0, noise, act = rnd(K, N, D), rnd(N, D), rnd(K, N, 2), (rnd(K, N, 2) * 0.7).clamp(-1.0, 1.0)
    sigma = torch.tensor([0.2, 0.3], dtype=dt, device=dev)
    length = torch.randint(max(1, K // 2), K + 1, (N,), device=dev, generator=gen).to(torch.int32)
    adv, reward = rnd(N), torch.rand(K, N, dtype=dt, device=dev, generator=gen)
    done = (torch.rand(K, N, device=dev, generator=gen) < 0.01).to(torch.uint8)
    baseline = torch.rand(K, P, dtype=dt, device=dev, generator=gen)
    outs = [dict(grad=new(2, D + 1, P), lane=new(2, D + 1, N), count=new(4, N, dtype=torch.int32), steps=new(P, dtype=torch.int32),
                 clipped=new(2, P, dtype=torch.int32), valid=new(P, dtype=torch.int32)) for _ in range(2)]
    counted = (torch.arange(K, device=dev).unsqueeze(1) < length.unsqueeze(0)).to(dt)           # [K, N]: made once, as the example's mask is cheap
    lane_policy = torch.arange(N, device=dev) % P
    kept = {}

    def device(o, **weight):
        def fn():
            sim.policy_gradient_into(obs, noise, sigma, o["grad"], o["lane"], o["count"], policies=P, obs0=obs0, actions=act, length=length,
                                     steps=o["steps"], clipped=o["clipped"], valid=o["valid"], **weight)
        return fn

    def statements(psi):
        """the example's statements behind the weight psi ([N], or [K, N]) -> grad [2, D+1, P]"""
        prev = torch.cat([obs0.unsqueeze(0), obs[:-1]])
        coef = (act.abs() < 1.0).to(dt) * noise / sigma * (counted * psi).unsqueeze(-1)
        coef_p = coef.view(K, S, P, 2)
        return torch.cat([torch.einsum("kspj,kspd->jdp", coef_p, prev.view(K, S, P, D)), coef_p.sum((0, 1)).t().unsqueeze(1)], 1)

    def torch_return():
        kept["return"] = statements(adv.unsqueeze(0))

    def torch_rtg():
        G = new(N)
        psi = new(K, N)
        for k in range(K - 1, -1, -1):
            G = torch.where(counted[k] > 0, torch.where(done[k] != 0, reward[k], reward[k] + GAMMA * G), G)
            psi[k] = G - baseline[k][lane_policy]
        kept["rtg"] = statements(psi)
    cases = (("return", torch_return, device(outs[0], adv=adv)),
             ("reward-to-go", torch_rtg, device(outs[1], rewards=reward, done=done, gamma=GAMMA, baseline=baseline)))
    peaks = {}
    for (name, theirs, ours), o, key in zip(cases, outs, ("return", "rtg")):
        for label, fn in (("torch", theirs), ("device", ours)):
            fn()
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            fn()
            torch.cuda.synchronize()
            peaks[(name, label)] = torch.cuda.max_memory_allocated(dev) - held
        scale = float(kept[key].abs().max())
        far = float((o["grad"] - kept[key]).abs().max()) / scale
        assert far < (1e-10 if dt == torch.float64 else 2e-3), f"the device call and the torch statements disagree ({name}): {far}"
        assert int(o["valid"].sum()) == N and int(o["steps"].sum()) == int(length.sum())
    emit(f"P = {P} policies, S = {S} samples, K = {K} steps, N = {N} lanes, D = {D}, {str(dt).split('.')[-1]}")
    walked = int(length.sum())
    shared = (walked * (D + 4) + N * D + 2) * esz + N * 4 + 2 * (2 * (D + 1) * N * esz + 4 * N * 4) + (2 * (D + 1) * P) * esz + 4 * P * 4
    nbytes = {"return": shared + N * esz, "reward-to-go": shared + walked * (esz + 1) + K * P * esz}
    for name, theirs, ours in cases:
        labels = (f"torch, {name}", f"device, {name}: policy_gradient_into")
        res = compare(torch, list(zip(labels, (theirs, ours))), reps, emit)
        med = res[labels[1]][0]
        emit(f"  device, {name}: {nbytes[name] / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes[name] / (med * 1e-3) / 1e9:.1f} GB/s, "
             f"{100 * nbytes[name] / (med * 1e-3) / PEAK:.2f} % of 8 TB/s")
        emit(f"  torch / device, {name}: {res[labels[0]][0] / med:.2f}; peak allocated above the arguments: torch "
             f"{peaks[(name, 'torch')] / 1e6:.1f} MB, device {peaks[(name, 'device')] / 1e6:.1f} MB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1,8192,500", "1,65536,50", "64,256,50", "4096,16,50", "65536,1,50"], help="P,S,K")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pg_rate: no GPU visible; nothing is measured without one")
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

    emit(f"HipSim.policy_gradient_into against the torch statements of examples/reinforce_balancing.py; HIP events; "
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
