#!/usr/bin/env python3
"""Time per line search of os2rs_ilqr_line_search (include/os2r_search.h) against the torch statement of steps 3, 6 and 7 of
examples/ilqr_balancing.py made per-trajectory, on identical inputs, and against the bytes the call must move.

  python tools/ilqr_line_search_rate.py [--knots 50] [--traj 64 4096 16384] [--dtype f64 f32] [--reps 5]
                                        [--out profiles/ilqr_line_search_rate.txt]

The free_hip robot (nq 5, n = 10, D = 10 raw observation slots: Monopod-nonorm-balance-v1's layout), K knots, the four step
sizes 1, 1/2, 1/4, 1/8 (N = 4 M candidate lanes), the example's costs: Q diagonal (1 on the positions, 0.01 on the velocities),
R = 0.1 I.  The candidates are synthetic: observations N(0,1) around the targets, actions uniform in [-1.3, 1.3], no episode
ends.  Paths, each timed with HIP events on the current stream, alternating within one process --reps times after one untimed
round (median, min and max per path):
  device    sim.ilqr_line_search_into(...) with every output and always=True, so that every call accepts a candidate for every
            trajectory and writes the whole nominal (a call that accepts nothing writes only choice and index)
  raw       the same launch through ctypes with its arguments built once, as a C caller makes it: HipSim's checks of Q, R and
            of every tensor run on the host per call, while the launch before is still on the device
  torch     cost of every candidate (cat, repeat, two reductions, an einsum), argmin per trajectory, the acceptance test against
            a cost that every candidate beats, one bool(any()) read back by the host -- the synchronisation an iteration needs to
            steer mu --, then gather of the accepted rows into the nominal, lx = Q (x - x*) by scatter, lu = R a, p_final, and the
            copy_envs_from index; every tensor it writes is allocated by torch as it goes
Every path is warmed up with three calls, then a ten-call probe sizes its windows to about 0.3 s (at least 3 calls, at most
20 000).  Before anything is timed the two paths' choices are compared (a difference is reported) and the largest differences
of their costs and gradients printed.
The byte floor: the call reads K N (D + 2) + N D elements and K N done bytes, the accepted rows once more (K M (D + 2) + M D),
and writes the nominal (K M (2 + D + n + 2) + M (D + n + 1) elements), index, choice and cand_cost; over the 8 TB/s HBM rate that
bench.py uses for its roofline.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lqr_gains_rate import make_sim, window  # noqa: E402

ALPHAS = (1.0, 0.5, 0.25, 0.125)
HBM_PEAK_GBS = 8000.0          # bench.py's


def measure(torch, sim, K, M, reps, emit):
    from gym_os2r_amd.control import slot_columns
    dev, dt, nq, D = sim.device, sim.dtype, sim.nq, sim.D
    n, nal = 2 * nq, len(ALPHAS)
    N, L = nal * M, K * M
    cols = slot_columns(sim.cfg.task, nq)
    slots = [d for d in range(D) if cols[d] >= 0]
    shown = [cols[d] for d in slots]
    assert len(set(shown)) == len(shown)
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, dtype=dt, device=dev, generator=gen)
    target = rnd(M, D)
    kobs = target.repeat(nal, 1)[None] + rnd(K, N, D)
    eobs = target.repeat(nal, 1) + rnd(N, D)
    act = torch.rand(K, N, 2, dtype=dt, device=dev, generator=gen) * 2.6 - 1.3
    done = torch.zeros(K, N, dtype=torch.uint8, device=dev)
    qdiag = torch.tensor([0.0 if c not in shown else (1.0 if c < nq else 0.01) for c in range(n)], dtype=torch.float64)
    Q, R = torch.diag(qdiag), 0.1 * torch.eye(2, dtype=torch.float64)
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    nom = dict(cost=new(M), act_nom=new(K, M, 2), obs_nom=new(K, M, D), end_nom=new(M, D), lx=new(n, L), lu=new(2, L), p_final=new(n, M))
    choice, index, cand_cost = new(M, dtype=torch.int32), new(L, dtype=torch.int32), new(nal, M)

    def device():
        sim.ilqr_line_search_into(kobs, eobs, act, target, Q, R, choice=choice, done=done, always=True, index=index, cand_cost=cand_cost, **nom)

    import ctypes as C
    from gym_os2r_amd import abi, control, search
    lib = search.load()
    lay = control.layout(abi.F64 if dt == torch.float64 else abi.F32, nq, sim.cfg.device, cols)
    p = lambda t: C.c_void_p(t.data_ptr())
    raw_args = (C.byref(lay), K, M, nal, search.ACCEPT_ALWAYS, p(kobs), p(eobs), p(act), p(done), p(target),
                (C.c_double * (n * n))(*Q.reshape(-1).tolist()), (C.c_double * 4)(*R.reshape(-1).tolist()), None, p(nom["cost"]),
                p(nom["act_nom"]), p(nom["obs_nom"]), p(nom["end_nom"]), p(nom["lx"]), p(nom["lu"]), p(nom["p_final"]), p(choice), p(index),
                p(cand_cost), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))

    def raw():
        if lib.os2rs_ilqr_line_search(*raw_args) != abi.OK:
            raise RuntimeError(lib.os2rs_last_error().decode())

    qs, Rd, tgt = qdiag[shown].to(dev, dt), R.to(dev, dt), target[:, slots]
    cost0 = torch.full((M,), 1e30, dtype=dt, device=dev)
    lane = torch.arange(L, device=dev)
    keep = dict(act=new(K, M, 2), obs=new(K, M, D), end=new(M, D))
    out = {}

    def torch_path():
        obs_seq = torch.cat([kobs, eobs[None]])
        err = obs_seq[:, :, slots] - tgt.repeat(nal, 1)
        a = act.clamp(-1.0, 1.0)
        J_c = (0.5 * (err * err * qs).sum(dim=(0, 2)) + 0.5 * torch.einsum("kbi,ij,kbj->b", a, Rd, a)).view(nal, M)
        best = J_c.argmin(0)
        J_b = J_c.gather(0, best[None])[0]
        acc = J_b < cost0
        out["any"] = bool(acc.any())                                             # the host's one look, to steer mu
        pick = best.view(1, 1, M, 1)
        sel_a = a.view(K, nal, M, 2).gather(1, pick.expand(K, 1, M, 2))[:, 0]
        sel_o = kobs.view(K, nal, M, D).gather(1, pick.expand(K, 1, M, D))[:, 0]
        sel_e = eobs.view(nal, M, D).gather(0, best.view(1, M, 1).expand(1, M, D))[0]
        act_nom = torch.where(acc[None, :, None], sel_a, keep["act"])
        obs_nom = torch.where(acc[None, :, None], sel_o, keep["obs"])
        end_nom = torch.where(acc[:, None], sel_e, keep["end"])
        lx = torch.zeros(L, n, dtype=dt, device=dev)
        lx[:, shown] = qs * (obs_nom.view(L, D)[:, slots] - tgt.repeat(K, 1))
        lu = act_nom.view(L, 2) @ Rd
        p_final = torch.zeros(M, n, dtype=dt, device=dev)
        p_final[:, shown] = qs * (end_nom[:, slots] - tgt)
        m = lane % M
        idx = torch.where(acc[m], (lane // M) * N + best[m] * M + m, -1).to(torch.int32)
        out.update(choice=torch.where(acc, best, -1), cost=torch.where(acc, J_b, cost0), J_c=J_c, act=act_nom, obs=obs_nom, end=end_nom, lx=lx,
                   lu=lu, p_final=p_final, index=idx)

    device()
    torch_path()
    torch.cuda.synchronize()
    rel = lambda got, ref: float((got - ref).abs().max() / ref.abs().max())
    differ = int((choice.long() != out["choice"]).sum())          # (two candidates within rounding of each other could swap)
    if differ == 0:
        assert torch.equal(index, out["index"]) and torch.equal(nom["act_nom"], out["act"]) and torch.equal(nom["obs_nom"], out["obs"])
        assert torch.equal(nom["end_nom"], out["end"])
    else:
        emit(f"  the two paths chose differently for {differ} of {M} trajectories: the gradients below are not comparable")
    took = torch.bincount(choice + 1, minlength=nal + 1).tolist()
    emit(f"K = {K}, M = {M}, {str(dt).split('.')[-1]}, {nal} step sizes; trajectories per step size {took[1:]}, none {took[0]}; largest differences "
         f"from the torch path, relative to the largest entry: costs {rel(cand_cost, out['J_c']):.2e}, lx {rel(nom['lx'].T, out['lx']):.2e}, "
         f"lu {rel(nom['lu'].T, out['lu']):.2e}, p_final {rel(nom['p_final'].T, out['p_final']):.2e}")
    cases = [("device: HipSim.ilqr_line_search_into", device), ("raw: the launch alone, through ctypes", raw),
             ("torch: steps 3, 6, 7 per trajectory, one sync", torch_path)]
    sized = []
    for label, fn in cases:                          # warmed up, then sized by a ten-call probe to fill about 0.3 s
        window(torch, fn, 3)
        sized.append((label, fn, max(3, min(20000, int(300.0 / max(window(torch, fn, 10), 1e-3))))))
    cases = sized
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
        emit(f"  {label:<46} {med[label]:10.4f} ms per call  (min {t[0]:.4f}, max {t[-1]:.4f}; {c} per window, {reps} windows)")
    d_, r_, t_ = (c[0] for c in cases)
    r = sorted(a / b for a in times[t_] for b in times[d_])
    emit(f"  {'torch / device':<46} {med[t_] / med[d_]:10.2f} x  (over all pairs of windows: {r[0]:.2f} .. {r[-1]:.2f})")
    d_ = r_                                          # the floor is held against the launch itself
    esz = kobs.element_size()
    read = (K * N * (D + 2) + N * D + M * D + M) * esz + K * N + (K * M * (D + 2) + M * D) * esz
    wrote = (K * M * (2 + D + n + 2) + M * (D + n + 1) + N) * esz + 4 * (L + M)
    floor_ms = (read + wrote) / (HBM_PEAK_GBS * 1e9) * 1e3
    emit(f"  byte floor: {read / 1e6:.2f} MB read, {wrote / 1e6:.2f} MB written, {floor_ms:.4f} ms at {HBM_PEAK_GBS / 1000:.0f} TB/s; the launch "
         f"moves them at {(read + wrote) / med[d_] * 1e-6:.1f} GB/s: {floor_ms / med[d_]:.3f} of the floor's rate; "
         f"{K * N / med[d_] * 1e-6:.3f} G candidate-knots / s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--knots", type=int, default=50)
    ap.add_argument("--traj", type=int, nargs="+", default=[64, 4096, 16384])
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ilqr_line_search_rate: no GPU visible; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"os2rs_ilqr_line_search against the torch statement of the example's steps 3, 6 and 7, time per line search over HIP events; "
         f"{torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    for dtype in args.dtype:
        sim = make_sim(dtype)
        for M in args.traj:
            measure(torch, sim, args.knots, M, args.reps, emit)
        sim.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
