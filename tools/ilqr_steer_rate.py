#!/usr/bin/env python3
"""Time per call of the two kernels of libos2r_steer.so (include/os2r_steer.h) against their siblings, and per iteration of the
steered iLQR loop of examples/ilqr_balancing.py against its --line-search device loop, in one run.

  python tools/ilqr_steer_rate.py [--knots 50] [--traj 64 4096 16384] [--dtype f64 f32] [--reps 5] [--loop-iters 4]
                                  [--no-loop] [--out profiles/ilqr_steer_rate.txt]

The free_hip robot (nq 5, n = 10, D = 10), K knots, the four step sizes 1, 1/2, 1/4, 1/8, the example's costs.  Every path is
warmed up with three calls, a ten-call probe sizes its windows to about 0.3 s (at least 3 calls), and the paths of one comparison
alternate window by window, --reps windows each after one untimed round: median, min and max per path, HIP events on the current
stream.
  (a) os2rt_ilqr_backward_mu against os2rc_ilqr_backward with mu = 0.5 and the same weight table (gains, ff, flags, dv and the
      table for four step sizes asked of both; synthetic A, B of tools/ilqr_backward_rate.py's kind), both through ctypes with
      their arguments built once.  The added compulsory bytes are M words of mu.
  (b) os2rt_ilqr_steer with armijo = 0 and with armijo = 1e-4 against os2rs_ilqr_line_search on the inputs of
      tools/ilqr_line_search_rate.py, through ctypes.  Before every call of every path the nominal cost is filled with 1e30 (one
      fill kernel, the same for all three), so every trajectory accepts a candidate and the whole nominal is written, as a
      line search that makes progress does.  The added compulsory bytes are M words of mu (and 2 M of status and iters) and, with
      armijo != 0, 2 K M words of dv.
  (c) one whole iteration on real handles, M trajectories from the reset posture under zero torque: linearize, the backward pass,
      copy_envs_from, the recorded rollout_schedule of 4 M candidates, the line search, copy_envs_from.  `device`: mu a host
      scalar steered by bool((choice >= 0).any()), read back every iteration (examples/ilqr_balancing.py --line-search device);
      `steered`: ilqr_backward(mu_dev=...) and ilqr_steer, nothing read back.  Windows of --loop-iters iterations.
The yardsticks are the siblings and the existing loop.  (a) or (b) is called slower than its sibling only beyond the sibling's
own window range plus the share of the added compulsory bytes in what the sibling moves.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lqr_gains_rate import window  # noqa: E402

ALPHAS = (1.0, 0.5, 0.25, 0.125)


def make_sim(dtype, num_envs=64):
    import gym_os2r_amd as g
    from gym_os2r_amd import abi, rewards
    from gym_os2r_amd.sim import HipSim
    from gym_os2r_amd.tasks.monopod_no_norm import MonopodTask
    task = MonopodTask(1000, task_mode="free_hip", reward_class=rewards.BalancingV1, reset_positions=["stand"])
    task.create_spaces()
    model = g.get_model(g.config.SettingsConfig().get_config("task_modes/free_hip/model"))
    spec = task.kernel_spec(model, reset_mode=abi.RESET_FIXED, randomize_params=False, max_episode_steps=0)
    return HipSim(abi.config_struct(model, spec, num_envs=num_envs, seed=1, contact=True, dtype=abi.F64 if dtype == "f64" else abi.F32))


def compare(torch, cases, reps, emit, unit="call"):
    """cases: [(label, fn)], the first one the yardstick -> {label: (median, min, max)}; the paths alternate window by window."""
    sized = []
    for label, fn in cases:
        window(torch, fn, 3)
        sized.append((label, fn, max(3, min(20000, int(300.0 / max(window(torch, fn, 10), 1e-3))))))
    times = {label: [] for label, _ in cases}
    for rep in range(reps + 1):                      # round 0 is the warm-up of every path
        for label, fn, c in sized:
            ms = window(torch, fn, c)
            if rep:
                times[label].append(ms)
    out = {}
    for label, _, c in sized:
        t = sorted(times[label])
        out[label] = (t[len(t) // 2], t[0], t[-1])
        emit(f"  {label:<58} {out[label][0]:10.4f} ms per {unit}  (min {t[0]:.4f}, max {t[-1]:.4f}; {c} per window, {reps} windows)")
    return out


def verdict(res, yard, label, added_bytes, moved_bytes, emit):
    med, lo, hi = res[yard]
    allowed = (hi - lo) + med * added_bytes / moved_bytes
    diff = res[label][0] - med
    emit(f"  {label.split(':')[0]} - {yard.split(':')[0]}: {diff:+.4f} ms ({100 * diff / med:+.1f} %); the sibling's window range {hi - lo:.4f} ms plus "
         f"the added bytes' share {100 * added_bytes / moved_bytes:.2f} % allow {allowed:.4f} ms: {'within' if diff <= allowed else 'BEYOND'}")


def kernels(torch, sim, K, M, reps, emit):
    from gym_os2r_amd import abi, control, search, steer
    from gym_os2r_amd.control import slot_columns
    dev, dt, nq, D = sim.device, sim.dtype, sim.nq, sim.D
    n, nal = 2 * nq, len(ALPHAS)
    N, L = nal * M, K * M
    esz = 8 if dt == torch.float64 else 4
    cols = slot_columns(sim.cfg.task, nq)
    shown = [c for c in cols if c >= 0]
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, dtype=dt, device=dev, generator=gen)
    new = lambda *s, dtype=dt: torch.zeros(*s, dtype=dtype, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    lay = control.layout(abi.F64 if dt == torch.float64 else abi.F32, nq, sim.cfg.device, cols)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    qdiag = [0.0 if c not in shown else (1.0 if c < nq else 0.01) for c in range(n)]
    q = (C.c_double * (n * n))(*[qdiag[i] if i == j else 0.0 for i in range(n) for j in range(n)])
    r = (C.c_double * 4)(0.1, 0.0, 0.0, 0.1)
    al = (C.c_double * nal)(*ALPHAS)
    emit(f"K = {K}, M = {M}, {str(dt).split('.')[-1]}, {nal} step sizes")

    # (a) the backward pass
    A = torch.eye(n, dtype=dt, device=dev)[:, :, None] + 0.3 * rnd(n, n, L) / n ** 0.5
    B = 0.5 * rnd(n, 2, L)
    lx, lu, pv = rnd(n, L), 0.3 * rnd(2, L), rnd(n, M)
    act, obs = torch.rand(L, 2, dtype=dt, device=dev, generator=gen) * 2.6 - 1.3, rnd(L, D)
    mu_dev = torch.full((M,), 0.5, dtype=dt, device=dev)
    outs = [dict(gain=new(K, 2, n, M), ff=new(K, 2, M), flag=new(K, M, dtype=torch.uint8), dv=new(K, 2, M), w=new(K, 2, D + 1, N)) for _ in range(2)]
    clib, tlib = control.load(), steer.load()

    def args(o, mu):
        return (C.byref(lay), K, M, p(A), p(B), p(lx), p(lu), q, r, mu, None, p(pv), p(o["gain"]), p(o["ff"]), None, None, p(o["flag"]), p(o["dv"]),
                p(act), p(obs), al, nal, p(o["w"]), stream)
    a_theirs, a_ours = args(outs[0], 0.5), args(outs[1], p(mu_dev))

    def backward():
        if clib.os2rc_ilqr_backward(*a_theirs) != abi.OK:
            raise RuntimeError(clib.os2rc_last_error().decode())

    def backward_mu():
        if tlib.os2rt_ilqr_backward_mu(*a_ours) != abi.OK:
            raise RuntimeError(tlib.os2rt_last_error().decode())
    backward(), backward_mu()
    torch.cuda.synchronize()
    same = lambda x, y: torch.equal(x.view(torch.uint8), y.view(torch.uint8))             # (bytes: a NaN equals itself)
    assert all(same(outs[0][k], outs[1][k]) for k in outs[0]), "os2rt_ilqr_backward_mu differs from os2rc_ilqr_backward"
    labels = ("os2rc_ilqr_backward: mu = 0.5", "os2rt_ilqr_backward_mu: mu_dev = 0.5 everywhere")
    res = compare(torch, list(zip(labels, (backward, backward_mu))), reps, emit)
    moved = (L * (n * n + 2 * n + n + 2 + 2 + D) + n * M + K * M * (2 * n + 2 + 2) + K * 2 * (D + 1) * N) * esz + K * M
    verdict(res, labels[0], labels[1], M * esz, moved, emit)

    # (b) the line search
    target = rnd(M, D)
    kobs = target.repeat(nal, 1)[None] + rnd(K, N, D)
    eobs = target.repeat(nal, 1) + rnd(N, D)
    acts = torch.rand(K, N, 2, dtype=dt, device=dev, generator=gen) * 2.6 - 1.3
    done = new(K, N, dtype=torch.uint8)
    dv = -torch.rand(K, 2, M, dtype=dt, device=dev, generator=gen)
    sets = [dict(cost=new(M), act_nom=new(K, M, 2), obs_nom=new(K, M, D), end_nom=new(M, D), lx=new(n, L), lu=new(2, L), p_final=new(n, M),
                 choice=new(M, dtype=torch.int32), index=new(L, dtype=torch.int32), cand_cost=new(nal, M), mu=new(M), status=new(M, dtype=torch.int32),
                 iters=new(M, dtype=torch.int32)) for _ in range(3)]
    slib = search.load()
    nominal = ("cost", "act_nom", "obs_nom", "end_nom", "lx", "lu", "p_final")

    def search_args(o):
        return (C.byref(lay), K, M, nal, 0, p(kobs), p(eobs), p(acts), p(done), p(target), q, r, None, *[p(o[k]) for k in nominal], p(o["choice"]),
                p(o["index"]), p(o["cand_cost"]), stream)

    def steer_args(o, armijo):
        rule = steer.rule(armijo=armijo)
        return (C.byref(lay), K, M, nal, p(kobs), p(eobs), p(acts), p(done), p(target), q, r, None, p(dv), al, C.byref(rule),
                *[p(o[k]) for k in nominal], p(o["mu"]), p(o["status"]), p(o["iters"]), p(o["choice"]), p(o["index"]), p(o["cand_cost"]), stream), rule
    b_theirs, (b_free, rule0), (b_armijo, rule1) = search_args(sets[0]), steer_args(sets[1], 0.0), steer_args(sets[2], 1e-4)

    def line_search():
        sets[0]["cost"].fill_(1e30)
        if slib.os2rs_ilqr_line_search(*b_theirs) != abi.OK:
            raise RuntimeError(slib.os2rs_last_error().decode())

    def steered(o, a):
        def fn():
            o["cost"].fill_(1e30)
            if tlib.os2rt_ilqr_steer(*a) != abi.OK:
                raise RuntimeError(tlib.os2rt_last_error().decode())
        return fn
    fns = (line_search, steered(sets[1], b_free), steered(sets[2], b_armijo))
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    for k in nominal + ("choice", "index", "cand_cost"):
        assert same(sets[0][k], sets[1][k]), f"os2rt_ilqr_steer (armijo 0) differs from os2rs_ilqr_line_search in {k}"
    emit(f"  (every trajectory accepts: {int((sets[0]['choice'] >= 0).sum())} of {M}; with armijo 1e-4: {int((sets[2]['choice'] >= 0).sum())})")
    labels = ("os2rs_ilqr_line_search: cost refilled", "os2rt_ilqr_steer, armijo 0: cost refilled", "os2rt_ilqr_steer, armijo 1e-4: cost refilled")
    res = compare(torch, list(zip(labels, fns)), reps, emit)
    moved = (K * N * (D + 2) + N * D + M * D + M) * esz + K * N + (K * M * (D + 2) + M * D) * esz + \
        (K * M * (2 + D + n + 2) + M * (D + n + 1) + N) * esz + 4 * (L + M)
    verdict(res, labels[0], labels[1], M * esz + 8 * M, moved, emit)
    verdict(res, labels[0], labels[2], M * esz + 8 * M + 2 * K * M * esz, moved, emit)


def loop(torch, dtype, K, M, iters, reps, emit):
    nal = len(ALPHAS)
    nom, knots, cand, cand_knots = (make_sim(dtype, num) for num in (M, K * M, nal * M, K * nal * M))
    dev, dt, D, n = nom.device, nom.dtype, nom.D, 2 * nom.nq
    from gym_os2r_amd.control import slot_columns
    cols = slot_columns(nom.cfg.task, nom.nq)
    qdiag = torch.tensor([0.0 if c not in cols else (1.0 if c < nom.nq else 0.01) for c in range(n)], dtype=torch.float64)
    Q, R = torch.diag(qdiag), 0.1 * torch.eye(2, dtype=torch.float64)
    first = torch.arange(M, dtype=torch.int32, device=dev).repeat(nal)
    start = nom.checkpoint()
    state = {}

    def begin():
        """The first nominal, recorded: zero torque from the reset posture; the target is where it starts."""
        nom.restore(start)
        table0 = torch.zeros(M, K, 2, D + 1, dtype=dt, device=dev)
        _, _, (o_n, _, d_n, _, _), (a_n, _), kobs = nom.rollout_schedule(K, table0, want_outputs=True, want_actions=True, knots=knots,
                                                                         want_knot_obs=True)
        target = kobs[0].clone()
        _, _, _, nominal = nom.ilqr_line_search(kobs, o_n[K - 1], a_n, target, Q, R, done=d_n, want_cand_cost=False)
        nominal["mu"] = torch.zeros(M, dtype=dt, device=dev)
        state.update(target=target, nominal=nominal, mu=0.0, a_k=nominal["actions"].view(K * M, 2), obs_k=nominal["obs"].view(K * M, D))

    def iteration(steered):
        nominal, target, a_k, obs_k = state["nominal"], state["target"], state["a_k"], state["obs_k"]
        _, _, A, B = knots.linearize(a_k, want_next=False)
        mu_kw = dict(mu_dev=nominal["mu"]) if steered else dict(mu=state["mu"])
        _, _, _, _, _, dv, table = nom.ilqr_backward(A, B, Q, R, knots=K, lx=nominal["lx_view"], lu=nominal["lu_view"], p_final=nominal["p_final_view"],
                                                     actions=a_k, obs=obs_k, alphas=ALPHAS, want_gains=False, want_ff=False, want_flags=False,
                                                     want_weights=True, **mu_kw)
        cand.copy_envs_from(knots, first)
        _, _, (o_c, _, d_c, _, _), (a_c, _), kobs_c = cand.rollout_schedule(K, table, want_outputs=True, want_actions=True, knots=cand_knots,
                                                                          want_knot_obs=True)
        if steered:
            _, index, _, _ = nom.ilqr_steer(kobs_c, o_c[K - 1], a_c, target, Q, R, dv, ALPHAS, nominal=nominal, done=d_c, want_cand_cost=False)
            knots.copy_envs_from(cand_knots, index)
        else:
            choice, index, _, _ = nom.ilqr_line_search(kobs_c, o_c[K - 1], a_c, target, Q, R, nominal=nominal, done=d_c, want_cand_cost=False)
            knots.copy_envs_from(cand_knots, index)
            if bool((choice >= 0).any()):                                            # the iteration's one decision on the host
                state["mu"] = 0.5 * state["mu"] if state["mu"] > 1e-3 else 0.0
            else:
                state["mu"] = max(10.0 * state["mu"], 0.1)
    emit(f"one iteration of the example's loop: K = {K}, M = {M}, {str(dt).split('.')[-1]}, {nal} step sizes, handles of {M}, {K * M}, {nal * M} and "
         f"{K * nal * M} environments; windows of {iters} iterations from a fresh nominal")
    times = {False: [], True: []}
    for rep in range(reps + 1):                      # round 0 is the warm-up of both loops
        for steered in (False, True):
            begin()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                iteration(steered)
            e1.record()
            e1.synchronize()
            if rep:
                times[steered].append(e0.elapsed_time(e1) / iters)
            if rep == reps:
                st = torch.bincount(state["nominal"]["status"], minlength=3).tolist() if steered else None
                emit(f"  ({'steered' if steered else 'device'}: mean cost after the last window {float(state['nominal']['cost'].mean()):.6e}"
                     + (f", active {st[0]} converged {st[1]} stalled {st[2]}, mu 0 for {int((state['nominal']['mu'] == 0).sum())})" if steered
                        else f", mu {state['mu']:.3e})"))
    med = {}
    for steered, label in ((False, "device: os2rc_ilqr_backward, os2rs_ilqr_line_search, one readback"), (True, "steered: os2rt_ilqr_backward_mu, os2rt_ilqr_steer, none")):
        t = sorted(times[steered])
        med[steered] = t[len(t) // 2]
        emit(f"  {label:<70} {med[steered]:10.4f} ms per iteration  (min {t[0]:.4f}, max {t[-1]:.4f}; {reps} windows)")
    emit(f"  steered / device: {med[True] / med[False]:.3f}")
    for s in (nom, knots, cand, cand_knots):
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--knots", type=int, default=50)
    ap.add_argument("--traj", type=int, nargs="+", default=[64, 4096, 16384])
    ap.add_argument("--dtype", choices=["f64", "f32"], nargs="+", default=["f64", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-iters", type=int, default=4)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ilqr_steer_rate: no GPU visible; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                   # (kept as it grows: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"os2rt_ilqr_backward_mu and os2rt_ilqr_steer against their siblings, and the steered loop against the device loop; HIP events; "
         f"{torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}")
    for dtype in args.dtype:
        sim = make_sim(dtype)
        for M in args.traj:
            kernels(torch, sim, args.knots, M, args.reps, emit)
        sim.close()
    if not args.no_loop:
        for M in args.traj:
            for dtype in args.dtype:
                loop(torch, dtype, args.knots, M, args.loop_iters, args.reps, emit)


if __name__ == "__main__":
    main()
