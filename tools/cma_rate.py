#!/usr/bin/env python3
"""Time per call of HipSim.cma_sample_into and HipSim.cma_update_into (libos2r_cma.so, include/os2r_cma.h) against the batched torch
statement of the same generation, in one run.

  python tools/cma_rate.py [--shapes 1,4096 64,256 4096,16 16384,4] [--dtype f64 f32] [--reps 5] [--out profiles/cma_rate.txt]

A shape is M populations and S samples each; N = S M lanes, D = 10 observation slots (the free_hip robot's), E = 22 entries of one
policy.  The state is a random positive definite covariance per population, paths ~ N(0, 0.3) and sigma = 0.3; the returns
~ N(0, 1) are random on the device; a small handle of the free_hip robot is made for its methods alone.  Every path is warmed up
with three calls, a ten-call probe sizes its windows to about 0.3 s (at least 3 calls), and the paths alternate window by window,
--reps windows each after one untimed round: median, min and max per path, HIP events on the current stream.
  sample, torch    linalg.cholesky of the covariances, randn [M, S, E], bmm, mean + sigma y
  sample, device   cma_sample_into without z, its tensors made once
  update, torch    on the z and y tensors that were kept from the sampling: argsort of the returns, gather of the parents' z and
                   y, three einsum, the paths, the covariance, exp
  update, device   cma_update_into without the optional outputs, its tensors made once; it reads neither z nor y
Reported with the device times: the compulsory bytes -- the sample call reads mean, sigma and the covariance's lower triangle and
writes factor, failed and the weights; the update reads the returns, the state, factor and failed and writes the state, count,
status and rank -- over the time, against 8 TB/s.  No ratio is fixed in advance: the file says what was measured.
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

D, GENERATION, AGE, PEAK = 10, 3, 3, 8e12


def measure(torch, sim, M, S, reps, emit):
    from gym_os2r_amd import cma
    dev, dt = sim.device, sim.dtype
    esz = 8 if dt == torch.float64 else 4
    N, E, i32 = S * M, 2 * (D + 1), torch.int32
    gen = torch.Generator(device=dev).manual_seed(0)
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    rnd = lambda *s: torch.randn(*s, dtype=dt, device=dev, generator=gen)
    B = torch.eye(E, dtype=dt, device=dev) + 0.15 * rnd(M, E, E)
    cov = B @ B.transpose(1, 2)
    cov = torch.tril(cov) + torch.tril(cov, -1).transpose(1, 2)
    state = (rnd(M, 2, D + 1) * 0.3, torch.full((M,), 0.3, dtype=dt, device=dev), cov.contiguous(), rnd(M, E) * 0.3, rnd(M, E) * 0.3)
    state_new = tuple(torch.zeros_like(t) for t in state)
    returns = rnd(N)
    factor, failed, weights, z = new(M, E, E), new(M, dtype=i32), new(N, 2, D + 1), new(N, 2, D + 1)
    count, status, rank = new(M, dtype=i32), new(M, dtype=i32), new(N, dtype=i32)
    rankw_host, k = cma.constants(E, S, age=AGE)
    mu = len(rankw_host)
    rankw = torch.tensor(rankw_host, dtype=torch.float64).to(dt).to(dev)
    held = {}
    sim.cma_sample_into(state, factor, failed, weights, samples=S, generation=GENERATION, z=z)
    mean, sigma = state[0].view(M, E), state[1]
    z_kept = z.view(S, M, E).transpose(0, 1).contiguous()                  # [M, S, E]: what the torch update reads, kept from the sampling
    y_kept = torch.bmm(z_kept, factor.transpose(1, 2))

    def device_sample():
        sim.cma_sample_into(state, factor, failed, weights, samples=S, generation=GENERATION)

    def torch_sample():
        A = torch.linalg.cholesky(state[2])
        zz = torch.randn(M, S, E, dtype=dt, device=dev, generator=gen)
        held["weights"] = mean.unsqueeze(1) + sigma.view(M, 1, 1) * torch.bmm(zz, A.transpose(1, 2))

    def device_update():
        sim.cma_update_into(returns, state, factor, failed, state_new, count, status, rank, samples=S, generation=GENERATION, rankw=rankw,
                            constants=k)

    def torch_update():
        order = torch.argsort(returns.view(S, M).t(), dim=1, descending=True, stable=True)[:, :mu]        # [M, mu]
        idx = order.unsqueeze(-1).expand(M, mu, E)
        zp, yp = z_kept.gather(1, idx), y_kept.gather(1, idx)
        zw, yw = torch.einsum("r,mre->me", rankw, zp), torch.einsum("r,mre->me", rankw, yp)
        R = torch.einsum("r,mri,mrj->mij", rankw, yp, yp)
        ps = k.a_sigma * state[3] + k.b_sigma * zw
        nrm = ps.norm(dim=1)
        h = (nrm < k.hsig_bound).to(dt)
        pc = k.a_c * state[4] + (h * k.b_c).unsqueeze(-1) * yw
        k0 = h * k.k0_moving + (1 - h) * k.k0_stalled
        held["mean"] = mean + sigma.unsqueeze(-1) * yw
        held["cov"] = k0.view(M, 1, 1) * state[2] + k.c_1 * pc.unsqueeze(2) * pc.unsqueeze(1) + k.c_mu * R
        held["sigma"] = (sigma * torch.exp(k.g_sigma * (nrm / k.chi - 1))).clamp(k.sigma_min, k.sigma_max)
        held["p_sigma"], held["p_c"] = ps, pc

    emit(f"M = {M} populations, S = {S} samples, N = {N} lanes, mu = {mu}, D = {D}, {str(dt).split('.')[-1]}")
    tol = 1e-9 if dt == torch.float64 else 2e-3             # (both paths sum in the dtype, in different orders)
    device_update()
    torch_update()
    torch.cuda.synchronize()
    assert int(failed.abs().sum()) == 0 and int(status.abs().sum()) == 0
    for name, have in zip(("mean", "sigma", "cov", "p_sigma", "p_c"), state_new):
        far = float((have.reshape(held[name].shape) - held[name]).abs().max()) / float(held[name].abs().max())
        assert far < tol, f"the device call and the torch statement disagree on {name}: {far}"
    labels = ("sample, torch: cholesky, randn, bmm", "sample, device: cma_sample_into")
    res = compare(torch, list(zip(labels, (torch_sample, device_sample))), reps, emit)
    med = res[labels[1]][0]
    nbytes = (M * E + M + M * E * (E + 1) // 2 + M * E * E + N * E) * esz + M * 4
    emit(f"  sample, device: {nbytes / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes / (med * 1e-3) / 1e9:.1f} GB/s, "
         f"{100 * nbytes / (med * 1e-3) / PEAK:.3f} % of 8 TB/s;  torch / device: {res[labels[0]][0] / med:.2f}")
    labels = ("update, torch: argsort, gather, einsum", "update, device: cma_update_into")
    res = compare(torch, list(zip(labels, (torch_update, device_update))), reps, emit)
    med = res[labels[1]][0]
    per_state = M * (3 * E + 1) + M * E * E
    nbytes = (N + mu + per_state + M * E * (E + 1) // 2 + M * (3 * E + 1) + M * E * E) * esz + 3 * M * 4 + N * 4
    emit(f"  update, device: {nbytes / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes / (med * 1e-3) / 1e9:.1f} GB/s, "
         f"{100 * nbytes / (med * 1e-3) / PEAK:.3f} % of 8 TB/s;  torch / device: {res[labels[0]][0] / med:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1,4096", "64,256", "4096,16", "16384,4"], help="M,S")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cma_rate: no GPU visible; nothing is measured without one")
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

    emit(f"HipSim.cma_sample_into and HipSim.cma_update_into against the batched torch statement; HIP events; "
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
