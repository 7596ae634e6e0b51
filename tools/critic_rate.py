#!/usr/bin/env python3
"""Time per call of HipSim.gae_into and HipSim.value_fit_into (libos2r_critic.so, include/os2r_critic.h) against the torch
statements for the same quantities, in one run.

  python tools/critic_rate.py [--shapes 1,8192,500 1,65536,50 64,256,50 4096,16,50] [--dtype f64 f32] [--reps 5]
                              [--out profiles/critic_rate.txt]

A shape is P policies, S samples per policy, K steps; N = S P lanes, D = 10 observation slots (the free_hip robot's).  The inputs
are random on the device -- observations uniform in [-1, 1], rewards, done bytes (a fall with probability 0.01, a truncation with
0.01), terminal observations, lengths between K / 2 and K --; a small handle of the free_hip robot is made for its methods alone.
Every path is warmed up with three calls, a ten-call probe sizes its windows to about 0.3 s (at least 3 calls), and the paths
alternate window by window, --reps windows each after one untimed round: median, min and max per path, HIP events on the current
stream.
  GAE
    torch        the values of all K + 1 observation rows by one einsum, then a reverse loop over the K steps
    device       gae_into with adv, ret and values, its tensors made once
  value fit
    torch        einsum for the moments of every policy, linalg.solve for the weights
    device       value_fit_into with every output, its tensors made once
Reported with each device time: the compulsory bytes -- of the counted steps the observations and, for GAE, rewards and done bytes
read, values written and read again, adv and ret written; for the fit the targets read and lane_mom written and read again --
over the time, against 8 TB/s.  No ratio is fixed in advance: the file says what was measured.
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

D, GAMMA, LAM, RIDGE, PEAK = 10, 0.97, 0.9, 1e-3, 8e12


def measure(torch, sim, P, S, K, reps, emit):
    from gym_os2r_amd import critic
    dev, dt = sim.device, sim.dtype
    esz = 8 if dt == torch.float64 else 4
    N, E = S * P, critic.moments(D)
    gen = torch.Generator(device=dev).manual_seed(0)
    uni = lambda *s: torch.rand(*s, dtype=dt, device=dev, generator=gen) * 2 - 1
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    obs, obs0, term = uni(K, N, D), uni(N, D), uni(K, N, D)
    reward = torch.rand(K, N, dtype=dt, device=dev, generator=gen)
    u = torch.rand(K, N, device=dev, generator=gen)
    done = torch.where(u < 0.01, 1, torch.where(u < 0.02, 2, 0)).to(torch.uint8)
    length = torch.randint(max(1, K // 2), K + 1, (N,), device=dev, generator=gen).to(torch.int32)
    value_w = torch.randn(D + 1, P, dtype=dt, device=dev, generator=gen) * 0.5
    prev = torch.randn(D + 1, P, dtype=dt, device=dev, generator=gen) * 0.5
    adv, ret, values = new(K, N), new(K, N), new(K, N)
    w, lane_mom, mom, count = new(D + 1, P), new(E, N), new(E, P), new(2, N, dtype=torch.int32)
    failed, steps, valid = (new(P, dtype=torch.int32) for _ in range(3))
    counted = torch.arange(K, device=dev).unsqueeze(1) < length.unsqueeze(0)                     # [K, N]: made once
    hard, trunc = (done & 5) != 0, ((done & 5) == 0) & ((done & 2) != 0)
    cut = hard | trunc
    wl = value_w[:, torch.arange(N, device=dev) % P]                                             # [D+1, N]
    kept = {}

    def device_gae():
        sim.gae_into(obs, reward, done, value_w, adv, values, obs0=obs0, policies=P, term_obs=term, length=length, gamma=GAMMA, lam=LAM, ret=ret)

    def torch_gae():
        rows = torch.cat([obs0.unsqueeze(0), obs])                                              # [K+1, N, D]
        v_all = torch.einsum("knd,dn->kn", rows, wl[:D]) + wl[D]
        v, v_next = v_all[:-1], v_all[1:]
        v_term = torch.einsum("knd,dn->kn", term, wl[:D]) + wl[D]
        nv = torch.where(hard, 0.0, torch.where(trunc, v_term, v_next))
        delta = reward + GAMMA * nv - v
        trace, out = new(N), new(K, N)
        for k in range(K - 1, -1, -1):
            trace = torch.where(counted[k], torch.where(cut[k], delta[k], delta[k] + GAMMA * LAM * trace), trace)
            out[k] = trace
        kept["adv"] = out * counted
        kept["ret"] = (out + v) * counted

    def device_fit():
        sim.value_fit_into(obs, ret, w, lane_mom, mom, count, obs0=obs0, policies=P, length=length, prev=prev, ridge=RIDGE, failed=failed,
                           steps=steps, valid=valid)

    def torch_fit():
        rows = torch.cat([obs0.unsqueeze(0), obs[:-1]])
        phi = torch.cat([rows, torch.ones(K, N, 1, dtype=dt, device=dev)], 2) * counted.unsqueeze(-1)
        phi_p = phi.view(K, S, P, D + 1)
        M = torch.einsum("kspi,kspj->pij", phi_p, phi_p)
        b = torch.einsum("kspi,ksp->pi", phi_p, ret.view(K, S, P))
        A = M + RIDGE * torch.eye(D + 1, dtype=dt, device=dev)
        kept["w"] = torch.linalg.solve(A, b + RIDGE * prev.t()).t()

    device_gae()
    torch_gae()
    device_fit()
    torch_fit()
    torch.cuda.synchronize()
    tol = 1e-9 if dt == torch.float64 else 1e-2           # (both paths sum millions of terms in the dtype, in different orders)
    for name, got in (("adv", adv), ("ret", ret), ("w", w)):
        far = float((got - kept[name]).abs().max()) / float(kept[name].abs().max())
        assert far < tol, f"the device call and the torch statements disagree ({name}): {far}"
    assert int(valid.sum()) == N and int(steps.sum()) == int(length.sum()) and int(failed.sum()) == 0
    emit(f"P = {P} policies, S = {S} samples, K = {K} steps, N = {N} lanes, D = {D}, {str(dt).split('.')[-1]}")
    walked = int(length.sum())
    truncated = int((trunc & counted).sum())
    nbytes = {"GAE": (walked * D + N * D + truncated * D + (D + 1) * P) * esz + walked * (esz + 1) + N * 4 + (2 * K * N + 2 * K * N) * esz,
              "value fit": (walked * (D + 1) + N * D) * esz + N * 4 + 2 * (E * N * esz + 2 * N * 4) + (2 * E * P + 2 * (D + 1) * P) * esz + 3 * P * 4}
    for name, theirs, ours, call in (("GAE", torch_gae, device_gae, "gae_into"), ("value fit", torch_fit, device_fit, "value_fit_into")):
        labels = (f"torch, {name}", f"device, {name}: {call}")
        res = compare(torch, list(zip(labels, (theirs, ours))), reps, emit)
        med = res[labels[1]][0]
        emit(f"  device, {name}: {nbytes[name] / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes[name] / (med * 1e-3) / 1e9:.1f} GB/s, "
             f"{100 * nbytes[name] / (med * 1e-3) / PEAK:.2f} % of 8 TB/s")
        emit(f"  torch / device, {name}: {res[labels[0]][0] / med:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1,8192,500", "1,65536,50", "64,256,50", "4096,16,50"], help="P,S,K")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("critic_rate: no GPU visible; nothing is measured without one")
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

    emit(f"HipSim.gae_into and HipSim.value_fit_into against the torch statements; HIP events; "
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
