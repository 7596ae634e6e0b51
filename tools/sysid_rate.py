#!/usr/bin/env python3
"""Time per call of HipSim.sysid_perturb_into and HipSim.sysid_update_into (libos2r_sysid.so, include/os2r_sysid.h) against the
batched torch statement of the same iteration, in one run.

  python tools/sysid_rate.py [--shapes 1,4096,20,5 1,256,50,21 64,64,20,5 4096,4,10,3] [--dtype f64 f32] [--reps 5] [--out profiles/sysid_rate.txt]

A shape is T parameter sets, Q = M / T segments each, K steps and P identified parameters; N = (2 P + 1) M lanes, D = 10
observation slots (the free_hip robot's).  The lanes follow a random linear model about the measured observations, so every
system is positive definite; every segment is valid and every point is accepted (the state is fresh), which is the branch that
does all the work.  A small handle of the free_hip robot is made for its methods alone.  Every path is warmed up with three
calls, a ten-call probe sizes its windows to about 0.3 s (at least 3 calls), and the paths alternate window by window, --reps
windows each after one untimed round: median, min and max per path, HIP events on the current stream.
  perturb, torch   expand of base over the lanes, min / max of the two points, three indexed stores
  perturb, device  sysid_perturb_into, its tensors made once
  update, torch    the differences, two einsum for J'WJ and J'Wr and one for the cost, where() for the verdict and the damping,
                   linalg.cholesky and cholesky_solve, clamp
  update, device   sysid_update_into without the optional outputs, its tensors made once
Reported with the device times: the compulsory bytes -- the perturb call reads theta and base and writes the lanes; the update
reads obs, meas, done and the state and writes the state and theta_next (its scratch is not counted) -- over the time, against
8 TB/s.  No ratio is fixed in advance: the file says what was measured, LOSSES in capitals.
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

D, PEAK = 10, 8e12


def measure(torch, sim, T, Q, K, P, reps, emit):
    from gym_os2r_amd import abi, sysid
    dev, dt = sim.device, sim.dtype
    esz = 8 if dt == torch.float64 else 4
    M, S, F, i32 = T * Q, 2 * P + 1, sysid.rows(sim.nq), torch.int32
    N, E = S * M, P * (P + 1) // 2 + P + 1
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, dtype=dt, device=dev, generator=gen)
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    h = [0.01 * (1 + p / 4) for p in range(P)]
    lo, hi = [-10.0] * P, [10.0] * P
    ht, lot, hit = (torch.tensor(v, dtype=dt, device=dev) for v in (h, lo, hi))
    meas = rnd(K, M, D)
    nominal = meas + 0.1 * rnd(K, M, D)
    slope = rnd(K, P, M, D) * ht.view(1, P, 1, 1)
    obs = torch.cat([nominal.unsqueeze(1), nominal.unsqueeze(1) + slope, nominal.unsqueeze(1) - slope], 1).reshape(K, N, D).contiguous()
    del slope, nominal
    done, prec, theta = new(K, N, dtype=torch.uint8), 0.5 + torch.rand(D, dtype=dt, device=dev, generator=gen), rnd(T, P)
    state = sim.sysid_init(theta + 0.125)
    state_new = tuple(torch.zeros_like(t) for t in state)
    theta_next, sums, counts = new(T, P), new(E * (M + T)), new(M + T, dtype=i32)
    base, params = rnd(F, M), new(F, N)
    fields = [abi.PARAM_MASS_SCALE, abi.PARAM_DAMPING, abi.PARAM_FRICTION, abi.PARAM_MU]
    sel = ([(abi.PARAM_GRAVITY, 0)] + [(f, i) for f in fields for i in range(sim.nq)])[:P]
    rows = torch.tensor([sysid.row(sim.nq, f, i) for f, i in sel], device=dev)
    k = sysid.constants()
    steps = dict(h=h, lo=lo, hi=hi)
    held = {}
    sets = torch.arange(M, device=dev) % T
    plus_lane, minus_lane = 1 + torch.arange(P, device=dev), 1 + P + torch.arange(P, device=dev)

    def device_perturb():
        sim.sysid_perturb_into(theta, base, params, sel=sel, **steps)

    def torch_perturb():
        out = base.unsqueeze(1).expand(F, S, M).clone()
        th = theta[sets].t()                                           # [P, M]
        out[rows] = th.unsqueeze(1)
        out[rows, plus_lane] = torch.minimum(th + ht.unsqueeze(1), hit.unsqueeze(1))
        out[rows, minus_lane] = torch.maximum(th - ht.unsqueeze(1), lot.unsqueeze(1))
        held["params"] = out.view(F, N)

    def device_update():
        sim.sysid_update_into(obs, meas, prec, theta, state, state_new, theta_next, sums, counts, constants=k, done=done, **steps)

    def torch_update():
        lanes = obs.view(K, S, Q, T, D)
        bad = (done.view(K, S, Q, T) != 0).any(0).any(0)                                      # [Q, T]
        w = prec.view(1, 1, 1, D) * (~bad).to(dt).view(1, Q, T, 1)
        Delta = torch.minimum(theta + ht, hit) - torch.maximum(theta - ht, lot)               # [T, P]
        r = lanes[:, 0] - meas.view(K, Q, T, D)
        jac = (lanes[:, 1:1 + P] - lanes[:, 1 + P:]) / Delta.t().view(1, P, 1, T, 1)
        H = torch.einsum("kpqtd,kqtd,krqtd->tpr", jac, w, jac)
        g = torch.einsum("kpqtd,kqtd,kqtd->tp", jac, w, r)
        cost = 0.5 * torch.einsum("kqtd,kqtd,kqtd->t", r, w, r)
        accept = cost < state[1]
        lam = torch.where(accept, (state[4] * k.shrink).clamp_min(k.lam_min), state[4] * k.grow)
        Hs = torch.where(accept.view(T, 1, 1), H, state[2])
        gs = torch.where(accept.view(T, 1), g, state[3])
        best = torch.where(accept.view(T, 1), theta, state[0])
        A = Hs + torch.diag_embed(lam.view(T, 1) * torch.diagonal(Hs, dim1=1, dim2=2).clamp_min(k.diag_floor))
        L = torch.linalg.cholesky(A)
        delta = torch.cholesky_solve(-gs.unsqueeze(-1), L).squeeze(-1)
        held.update(theta_best=best, cost_best=torch.where(accept, cost, state[1]), hess=Hs, grad=gs, lam=lam,
                    theta_next=torch.maximum(torch.minimum(best + delta, hit), lot))

    emit(f"T = {T} sets, Q = {Q} segments each, K = {K} steps, P = {P} parameters, N = {N} lanes, D = {D}, {str(dt).split('.')[-1]}")
    tol = 1e-9 if dt == torch.float64 else 5e-3             # (both paths sum in the dtype, in different orders)
    device_perturb(); torch_perturb(); device_update(); torch_update()
    torch.cuda.synchronize()
    assert torch.equal(params, held["params"]), "the device call and the torch statement disagree on the lanes"
    assert int(state_new[5].abs().sum()) == 0 and int(state_new[6].sum()) == T
    for name, have in zip(("theta_best", "cost_best", "hess", "grad", "lam"), state_new):
        far = float((have - held[name]).abs().max()) / float(held[name].abs().max())
        assert far < tol, f"the device call and the torch statement disagree on {name}: {far}"
    far = float((theta_next - held["theta_next"]).abs().max()) / float(held["theta_next"].abs().max())
    assert far < 100 * tol, f"the device call and the torch statement disagree on theta_next: {far}"

    def verdict(ratio):
        return f"torch / device: {ratio:.2f}" + ("" if ratio >= 1 else "  LOSES")
    labels = ("perturb, torch: expand, min / max, indexed stores", "perturb, device: sysid_perturb_into")
    res = compare(torch, list(zip(labels, (torch_perturb, device_perturb))), reps, emit)
    med = res[labels[1]][0]
    nbytes = (T * P + F * M + F * N) * esz
    emit(f"  perturb, device: {nbytes / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes / (med * 1e-3) / 1e9:.1f} GB/s, "
         f"{100 * nbytes / (med * 1e-3) / PEAK:.3f} % of 8 TB/s;  {verdict(res[labels[0]][0] / med)}")
    labels = ("update, torch: einsum, cholesky, cholesky_solve", "update, device: sysid_update_into")
    res = compare(torch, list(zip(labels, (torch_update, device_update))), reps, emit)
    med = res[labels[1]][0]
    per_state = T * (2 * P + P * P + 2) * esz + 2 * T * 4
    nbytes = (K * N * D + K * M * D + D + T * P) * esz + K * N + 2 * per_state + T * P * esz
    emit(f"  update, device: {nbytes / 1e6:.3f} MB compulsory in {med:.4f} ms = {nbytes / (med * 1e-3) / 1e9:.1f} GB/s, "
         f"{100 * nbytes / (med * 1e-3) / PEAK:.3f} % of 8 TB/s;  {verdict(res[labels[0]][0] / med)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1,4096,20,5", "1,256,50,21", "64,64,20,5", "4096,4,10,3"], help="T,Q,K,P")
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sysid_rate: no GPU visible; nothing is measured without one")
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

    emit(f"HipSim.sysid_perturb_into and HipSim.sysid_update_into against the batched torch statement; HIP events; "
         f"{torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    for dtype in args.dtype:
        sim = HipSim(make_config("free_hip", "BalancingV2", False, num_envs=4, contact=True, seed=1,
                                 dtype=abi.F64 if dtype == "f64" else abi.F32)[0])
        assert sim.D == D
        for shape in args.shapes:
            T, Q, K, P = (int(v) for v in shape.split(","))
            measure(torch, sim, T, Q, K, P, args.reps, emit)
            torch.cuda.empty_cache()
        sim.close()


if __name__ == "__main__":
    main()
