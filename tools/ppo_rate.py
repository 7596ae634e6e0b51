#!/usr/bin/env python3
"""Time per call of HipSim.ppo_gradient_into (libos2r_ppo.so, include/os2r_ppo.h) against the batched torch statement of the same
epoch and against its sibling HipSim.policy_gradient_into on the same arrays, in one run.

  python tools/ppo_rate.py [--shapes 1,8192,500 1,65536,50 64,256,50 4096,16,50 65536,1,50] [--dtype f64 f32] [--reps 5]
                           [--out profiles/ppo_rate.txt]

A shape is P policies, S samples per policy, K steps; N = S P lanes, D = 10 observation slots (the free_hip robot's).  The inputs
are random on the device -- observations, noise, actions clipped to [-1, 1], advantages, lengths between K / 2 and K, weights a
step of 0.05 N(0, 1) from the old ones, sigma (0.2, 0.3), clip 0.2 --; a small handle of the free_hip robot is made for its
methods alone.  Every path is warmed up with three calls, a ten-call probe sizes its windows to about 0.3 s (at least 3 calls),
and the paths alternate window by window, --reps windows each after one untimed round: median, min and max per path, HIP events
on the current stream.  The paths:
  torch     the epoch written analytically (no autograd), the policy as a batch dimension: the cat that shifts the observation
            record by one, the mean shift as an einsum with the weight difference, z, rho = exp(0.5 sum(eps^2 - z^2)) over the
            components on which the clip did not bind, the gate, the coefficient tensor, the einsum and the sum for the bias
  sibling   policy_gradient_into(rewards=adv, done=..., gamma=0.0) with grad, lane_grad, lane_count, steps, clipped and valid: the
            on-policy gradient of the same arrays
  lean      ppo_gradient_into with grad, lane_grad, lane_stat, lane_count, stat, steps, clipped, gated and valid
  full      the same with ratio [K, N], lsig_grad and lane_lsig
Reported with each ppo path: its time minus the sibling's, against what the sibling's window range plus the share of the added
bytes allows (adv in place of reward with no done byte, the two weight arrays, lane_stat and the fifth row of lane_count written
and read again, the P-sized outputs; for `full` also ratio and lane_lsig) -- "within" or "BEYOND".  No ratio is fixed in
advance: the file says what was measured.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ilqr_steer_rate import compare, verdict  # noqa: E402

D, CLIP = 10, 0.2


def measure(torch, sim, P, S, K, reps, emit):
    dev, dt = sim.device, sim.dtype
    esz = 8 if dt == torch.float64 else 4
    N = S * P
    i32 = torch.int32
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, dtype=dt, device=dev, generator=gen)
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    obs, obs0, noise, act = rnd(K, N, D), rnd(N, D), rnd(K, N, 2), (rnd(K, N, 2) * 0.7).clamp(-1.0, 1.0)
    sigma = torch.tensor([0.2, 0.3], dtype=dt, device=dev)
    length = torch.randint(max(1, K // 2), K + 1, (N,), device=dev, generator=gen).to(i32)
    adv = rnd(K, N)
    done = new(K, N, dtype=torch.uint8)
    w_old = rnd(2, D + 1, P) * 0.3
    w = w_old + 0.05 * rnd(2, D + 1, P)
    counted = (torch.arange(K, device=dev).unsqueeze(1) < length.unsqueeze(0)).to(dt)           # [K, N]: made once
    lo, hi = 1.0 - CLIP, 1.0 + CLIP
    kept = {}
    sib = dict(grad=new(2, D + 1, P), lane=new(2, D + 1, N), count=new(4, N, dtype=i32), steps=new(P, dtype=i32), clipped=new(2, P, dtype=i32),
               valid=new(P, dtype=i32))
    outs = [dict(grad=new(2, D + 1, P), lane=new(2, D + 1, N), lane_stat=new(3, N), count=new(5, N, dtype=i32), stat=new(3, P),
                 steps=new(P, dtype=i32), clipped=new(2, P, dtype=i32), gated=new(P, dtype=i32), valid=new(P, dtype=i32)) for _ in range(2)]
    extra = dict(ratio=new(K, N), lsig_grad=new(2, P), lane_lsig=new(2, N))

    def sibling():
        sim.policy_gradient_into(obs, noise, sigma, sib["grad"], sib["lane"], sib["count"], policies=P, obs0=obs0, actions=act, length=length,
                                 rewards=adv, done=done, gamma=0.0, steps=sib["steps"], clipped=sib["clipped"], valid=sib["valid"])

    def device(o, **more):
        def fn():
            sim.ppo_gradient_into(obs, noise, sigma, w, w_old, adv, o["grad"], o["lane"], o["lane_stat"], o["count"], policies=P, clip=CLIP,
                                  obs0=obs0, actions=act, length=length, stat=o["stat"], steps=o["steps"], clipped=o["clipped"],
                                  gated=o["gated"], valid=o["valid"], **more)
        return fn

    def statement():
        prev = torch.cat([obs0.unsqueeze(0), obs[:-1]]).view(K, S, P, D)
        dW = w - w_old
        dmu = torch.einsum("kspd,jdp->kspj", prev, dW[:, :D, :]) + dW[:, D, :].t()
        eps = noise.view(K, S, P, 2)
        z = eps - dmu / sigma
        inside = (act.abs() < 1.0).to(dt).view(K, S, P, 2)
        rho = torch.exp(0.5 * (inside * (eps * eps - z * z)).sum(-1))
        psi = adv.view(K, S, P)
        closed = ((psi > 0) & (rho > hi)) | ((psi < 0) & (rho < lo))
        wgt = counted.view(K, S, P) * psi * rho * (~closed).to(dt)
        coef = inside * z / sigma * wgt.unsqueeze(-1)
        kept["grad"] = torch.cat([torch.einsum("kspj,kspd->jdp", coef, prev), coef.sum((0, 1)).t().unsqueeze(1)], 1)
        kept["gated"] = (closed & (counted.view(K, S, P) > 0)).sum((0, 1))
    lean, full = device(outs[0]), device(outs[1], **extra)
    for fn in (statement, sibling, lean, full):
        fn()
    torch.cuda.synchronize()
    scale = float(kept["grad"].abs().max())
    far = max(float((o["grad"] - kept["grad"]).abs().max()) / scale for o in outs)
    for o in outs:
        assert int(o["valid"].sum()) == N and int(o["steps"].sum()) == int(length.sum())
    # (in float a ratio within rounding of a bound gates on one side and not on the other: the distance is reported, not asserted)
    assert dt != torch.float64 or (far < 1e-10 and int((outs[0]["gated"] - kept["gated"]).abs().max()) <= 1), f"the device call and the torch statement disagree: {far}"
    assert torch.equal(outs[0]["grad"], outs[1]["grad"]) and int(sib["valid"].sum()) == N
    emit(f"P = {P} policies, S = {S} samples, K = {K} steps, N = {N} lanes, D = {D}, {str(dt).split('.')[-1]}; "
         f"gated {100.0 * int(outs[0]['gated'].sum()) / int(length.sum()):.1f} % of the counted steps, "
         f"grad {far:.1e} from the torch statement")
    walked = int(length.sum())
    moved = (walked * (D + 5) + N * D + 2) * esz + walked + N * 4 + 2 * (2 * (D + 1) * N * esz + 4 * N * 4) + (2 * (D + 1) * P) * esz + 4 * P * 4
    added_lean = 2 * 2 * (D + 1) * P * esz - walked + 2 * (3 * N * esz + N * 4) + 3 * P * esz + P * 4
    added_full = added_lean + K * N * esz + 2 * 2 * N * esz + 2 * P * esz
    labels = ("torch: the analytic epoch", "sibling: policy_gradient_into", "lean: ppo_gradient_into", "full: ppo_gradient_into, ratio and lsig_grad")
    res = compare(torch, list(zip(labels, (statement, sibling, lean, full))), reps, emit)
    for label, added in ((labels[2], added_lean), (labels[3], added_full)):
        verdict(res, labels[1], label, added, moved, emit)
    emit(f"  torch / lean: {res[labels[0]][0] / res[labels[2]][0]:.2f}; lean / sibling: {res[labels[2]][0] / res[labels[1]][0]:.2f}; "
         f"full / sibling: {res[labels[3]][0] / res[labels[1]][0]:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1,8192,500", "1,65536,50", "64,256,50", "4096,16,50", "65536,1,50"], help="P,S,K")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ppo_rate: no GPU visible; nothing is measured without one")
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

    emit(f"HipSim.ppo_gradient_into against the analytic torch epoch and against policy_gradient_into; HIP events; "
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
