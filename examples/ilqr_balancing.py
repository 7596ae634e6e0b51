#!/usr/bin/env python3
"""iLQR on Monopod-nonorm-balance-v1 with every piece of an iteration on the device: M trajectories of K knots are optimised side
by side towards a target posture, the backward pass in one os2rc_ilqr_backward launch.

  python examples/ilqr_balancing.py [--envs 64] [--steps 40] [--iters 10] [--settle 300] [--perturb 0.05] [--mu 0.0] [--eps 1e-4]
                                    [--knots recorded|loop] [--line-search torch|device|steered] [--armijo 0] [--tol 0] [--poll P]
                                    [--box] [--timing]

The cost of a trajectory is sum_k 1/2 (x_k - x*)'Q(x_k - x*) + 1/2 a_k'R a_k plus 1/2 (x_K - x*)'Q(x_K - x*), read off the raw
observation slots (state components the task does not observe carry no weight); x* is the posture the PD of lqr_balancing.py
settles in, the starts are that posture perturbed, the first nominal is zero torque.  Each iteration (--knots loop):
  1. the nominal is replayed from the start and knot k of trajectory m forked into lane k M + m of a K M-lane handle
     (copy_envs_from, one launch per knot: 2 K launches);
  2. one os2r_linearize launch returns A_k, B_k of every knot;
  3. lx = Q (x_k - x*), lu = R a_k and p_final = Q (x_K - x*) are formed in torch;
  4. one ilqr_backward launch returns the refusal flags, the two terms of the expected cost change and ONE table of weights
     for the step sizes 1, 1/2, 1/4, 1/8;
  5. one rollout_schedule launch on a handle of 4 M environments, forked from knot 0, runs all four candidates of every
     trajectory with the table as it came;
  6. their costs are read off the returned observations and actions;
  7. the best step size that lowers the summed cost is accepted (its applied actions are the new nominal); if none does, mu is
     raised and the iteration repeated.
With --knots recorded (the default) step 1 is gone: the rollout of step 5 records the knots of every candidate into a handle of
K 4 M lanes and their observations (rollout_schedule(..., knots=..., want_knot_obs=True): the same launch), and accepting a step
size moves its knots into the K M-lane handle with one copy_envs_from; the observations at the knots and the actions are views
of what that launch returned.  An iteration is five launches: linearize, ilqr_backward, copy_envs_from (knot 0 -> candidates),
rollout_schedule, copy_envs_from (the accepted knots).  The first nominal comes from one recorded rollout whose table has zero
gains and the actions as bias.  Both modes visit the same states bit for bit and print the same costs (as long as no episode ends
inside a trajectory: an auto-reset draws from the lane's own random stream, and a candidate's lane is not the nominal's).
With --line-search device (needs --knots recorded) steps 3, 6 and 7 are one os2rs_ilqr_line_search launch
(HipSim.ilqr_line_search): it scores every candidate, accepts a step size PER TRAJECTORY, updates the nominal in place where one
was accepted -- actions, knot observations, cost, and lx, lu, p_final in the layout the backward pass reads -- and returns the
index with which one copy_envs_from moves exactly the accepted knots.  An iteration is then six launches with no tensor
reshuffled in between; the host reads back one flag, (choice >= 0).any(), to steer mu (raised only when no trajectory accepted
anything), and for its printed line the mean cost and how many trajectories took which step size.  The first nominal is
initialised by the same call with one candidate per trajectory.  The default, --line-search torch, is the iteration above with
one step size for the whole batch.
With --line-search steered (needs --knots recorded) mu is one number per trajectory and lives on the device: the backward pass
reads it there (ilqr_backward(mu_dev=...): os2rt_ilqr_backward_mu), and the line search is os2rt_ilqr_steer (HipSim.ilqr_steer),
which in its one launch also halves the mu of every trajectory that accepted a step, raises the mu of every trajectory that did
not -- the rule above, per trajectory --, applies an Armijo test on the predicted change (--armijo c: a step must lower the
cost by at least c times what the model predicts; 0: none) and freezes a trajectory whose accepted step lowered its cost by no
more than --tol times its cost (converged) or whose mu would pass 1e6 (stalled).  The iteration is linearize, ilqr_backward,
copy_envs_from, rollout_schedule, ilqr_steer, copy_envs_from, with nothing read back inside the loop: the host launches the
iterations back to back and every --poll P iterations (default: only after the last) reads status, mu, iters and the costs
once, and prints the mean cost, the histogram of mu and how many trajectories are active, converged and stalled.  Frozen
trajectories still run through the backward pass and the rollout; they are just never accepted.
Printed per iteration: the cost (mean over the trajectories), the step size, mu, the refused knots, and the predicted against
the actual change.  The script prints what happened; it claims no control quality: a quotient across a change of contact mode
is a secant, the default eps is not tuned, and the actions saturate, which the model knows nothing about -- unless --box is given.
With --box, in all three --line-search modes, the backward pass is the control-limited one (ilqr_backward(box=True):
os2rb_ilqr_backward_box): where the step of the unconstrained model would leave [-1, 1] it is the exact minimum on the box, the
feedback row of a clamped actuator is zero, and the value recursion sees both.  Every printed line of an iteration then ends with
the share of knots at which a component is clamped (steered: of the iteration that was polled).  --timing (steered) adds the wall
time per iteration of the whole loop, read after the last poll.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gym_os2r_amd as g
from gym_os2r_amd.control import slot_columns
from lqr_balancing import weights_of_gain

ALPHAS = (1.0, 0.5, 0.25, 0.125)


def backward(sim, box, *args, **kw):
    """sim.ilqr_backward, with --box the control-limited pass -> (its seven results, clamped [K, M] uint8 or None)"""
    if not box:
        return sim.ilqr_backward(*args, **kw), None
    out = sim.ilqr_backward(*args, box=True, **kw)
    return out[:7], out[7]


def clamped_share(clamped):
    """the end of a printed line: nothing without --box"""
    return "" if clamped is None else f"; clamped {float((clamped != 0).double().mean()):.3f} of the knots"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64, help="M: trajectories optimised side by side")
    ap.add_argument("--steps", type=int, default=40, help="K: knots (env-steps) of a trajectory")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--settle", type=int, default=300, help="env-steps under the PD before the target posture is read")
    ap.add_argument("--perturb", type=float, default=0.05, help="standard deviation of the start perturbation [rad, rad/s]")
    ap.add_argument("--mu", type=float, default=0.0, help="initial control-space regularisation")
    ap.add_argument("--eps", type=float, default=None, help="finite-difference step (default: HipSim.linearize's)")
    ap.add_argument("--kp", type=float, default=8.0)
    ap.add_argument("--kd", type=float, default=0.15)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--knots", choices=("recorded", "loop"), default="recorded",
                    help="recorded: the candidates' rollout records the knots (five launches per iteration); loop: the nominal is "
                         "replayed and forked knot by knot")
    ap.add_argument("--line-search", choices=("torch", "device", "steered"), default="torch",
                    help="torch: costs and one step size for the whole batch in torch; device: one os2rs_ilqr_line_search launch, a step "
                         "size per trajectory (needs --knots recorded); steered: one os2rt_ilqr_steer launch, which also keeps a mu per "
                         "trajectory on the device (needs --knots recorded)")
    ap.add_argument("--armijo", type=float, default=0.0, help="steered: a step must lower the cost by this times the predicted change")
    ap.add_argument("--tol", type=float, default=0.0, help="steered: a trajectory converges when a step lowers its cost by no more than tol |cost|")
    ap.add_argument("--poll", type=int, default=0, help="steered: read the device every P iterations (0: only after the last)")
    ap.add_argument("--box", action="store_true", help="the control-limited backward pass: steps inside [-1, 1], clamped feedback rows zero")
    ap.add_argument("--timing", action="store_true", help="steered: print the wall time per iteration after the last poll")
    args = ap.parse_args()
    M, K, nal = args.envs, args.steps, len(ALPHAS)
    recorded = args.knots == "recorded"
    if args.line_search in ("device", "steered") and not recorded:
        ap.error(f"--line-search {args.line_search} needs --knots recorded")
    # one task, three handles: the nominal (M trajectories), the knots (K M lanes, knot-major), the candidates (4 M environments);
    # recorded: a fourth for the knots of every candidate (K 4 M lanes, knot-major)
    envs = [g.make("Monopod-nonorm-balance-v1", num_envs=n, seed=args.seed) for n in (M, K * M, nal * M) + ((K * nal * M,) if recorded else ())]
    for e in envs:
        e.reset()
    nom, knots, cand = (e.sim for e in envs[:3])
    cand_knots = envs[3].sim if recorded else None
    dev, dt, nq, D = nom.device, nom.dtype, nom.nq, nom.D
    n = 2 * nq
    cols = slot_columns(nom.cfg.task, nq)
    slots = [d for d in range(D) if cols[d] >= 0]                                     # the raw slots and the state column each shows
    shown = [cols[d] for d in slots]
    ih, ik = envs[0].model["act_dof"]
    print(f"iLQR on Monopod-nonorm-balance-v1: {M} trajectories of {K} knots, nq {nq}, unobserved state columns "
          f"{sorted(set(range(n)) - set(shown))}, step sizes {ALPHAS}", flush=True)

    # the target posture: where the posture PD settles; the starts: that posture, perturbed on the observed components
    obs0 = nom.copy_envs_from(nom, want_obs=True)
    K_pd = torch.zeros(M, 2, n, dtype=dt, device=dev)
    for j, dof in enumerate((ih, ik)):
        K_pd[:, j, dof] = args.kp / 2.5
        K_pd[:, j, nq + dof] = args.kd / 2.5
    nom.rollout_policy(args.settle, weights_of_gain(K_pd, torch.zeros(M, 2, dtype=dt, device=dev), obs0, cols))
    target_obs = nom.copy_envs_from(nom, want_obs=True)                               # [M, D]
    target = target_obs[:, slots]                                                     # [M, raw slots]
    q, qd = nom.get_state()
    gen = torch.Generator(device=dev).manual_seed(args.seed + 1)
    observed = torch.tensor([c in shown for c in range(n)], dtype=dt, device=dev)
    noise = args.perturb * torch.randn(n, M, dtype=dt, device=dev, generator=gen) * observed[:, None]
    nom.set_state(q + noise[:nq], qd + noise[nq:])
    start = nom.checkpoint()

    qdiag = torch.tensor([0.0 if c not in shown else (1.0 if c < nq else 0.01) for c in range(n)], dtype=dt, device=dev)
    Q, R = torch.diag(qdiag), 0.1 * torch.eye(2, dtype=dt, device=dev)
    qs = qdiag[shown]

    def cost(obs_seq, act):
        """obs_seq [K+1, B, D] (the knots and the end), act [K, B, 2] -> [B]; B is a multiple of M"""
        err = obs_seq[:, :, slots] - target.repeat(obs_seq.shape[1] // M, 1)
        a = act.clamp(-1.0, 1.0)
        return 0.5 * (err * err * qs).sum(dim=(0, 2)) + 0.5 * torch.einsum("kbi,ij,kbj->b", a, R, a)

    lanes = torch.arange(K * M, dtype=torch.int32, device=dev)
    fork = [torch.where(lanes // M == k, lanes % M, -1).to(torch.int32) for k in range(K)]   # (a negative entry keeps the lane)
    first = torch.arange(M, dtype=torch.int32, device=dev).repeat(nal)                # knot 0 of trajectory m, once per step size
    U = torch.zeros(K, M, 2, dtype=dt, device=dev)
    mu, it, tries, shown_cost = args.mu, 0, 0, None
    if args.line_search in ("device", "steered"):
        loop = line_search_on_device if args.line_search == "device" else steered_on_device
        loop(args, nom, knots, cand, cand_knots, start, target_obs, Q.cpu(), R.cpu(), first)
        for e in envs:
            e.close()
        return
    if recorded:
        # the first nominal, recorded: zero gains, the actions as bias (b + 0 o = b: the open-loop actions, bit for bit)
        table0 = torch.zeros(M, K, 2, D + 1, dtype=dt, device=dev)
        table0[:, :, :, D] = U.permute(1, 0, 2)
        nom.restore(start)
        _, _, (o_n, _, d_n, _, _), _, kobs = nom.rollout_schedule(K, table0, want_outputs=True, knots=knots, want_knot_obs=True)
        ended, end_obs, obs_k = int((d_n != 0).sum()), o_n[K - 1], kobs.view(K * M, D)
        lane = torch.arange(K * M, dtype=torch.int32, device=dev)
        best_lanes = [(lane // M) * (nal * M) + b * M + lane % M for b in range(nal)]    # knot k of trajectory m under step size b
    while it < args.iters and tries < 4 * args.iters:
        tries += 1
        if not recorded:
            # 1. replay the nominal, fork the knots
            nom.restore(start)
            ended = 0
            for k in range(K):
                knots.copy_envs_from(nom, fork[k])
                _, _, done, _ = nom.step(U[k], want_terminal=False)
                ended += int((done != 0).sum())
            end_obs = nom.copy_envs_from(nom, want_obs=True)
            obs_k = knots.copy_envs_from(knots, want_obs=True)                        # [K M, D]: the observation at each knot
        J = cost(torch.cat([obs_k.view(K, M, D), end_obs[None]]), U)
        if shown_cost is None:
            shown_cost = float(J.mean())
            print(f"iter {0:2d} cost {shown_cost:.6e} (the nominal: zero torque; {ended} episode ends inside it)", flush=True)
        # 2. every knot's Jacobians in one launch
        a_k = U.reshape(K * M, 2)
        _, _, A, B = knots.linearize(a_k, args.eps, want_next=False)
        # 3. the cost's gradients at the knots and behind the last one
        lx = torch.zeros(K * M, n, dtype=dt, device=dev)
        lx[:, shown] = qs * (obs_k[:, slots] - target.repeat(K, 1))
        lu = a_k.clamp(-1.0, 1.0) @ R
        p_final = torch.zeros(M, n, dtype=dt, device=dev)
        p_final[:, shown] = qs * (end_obs[:, slots] - target)
        # 4. the backward pass and the candidates' table in one launch
        (_, _, _, _, flags, dv, table), clamped = backward(nom, args.box, A, B, Q.cpu(), R.cpu(), knots=K, lx=lx, lu=lu, mu=mu, p_final=p_final,
                                                           actions=a_k, obs=obs_k, alphas=ALPHAS, want_gains=False, want_ff=False,
                                                           want_weights=True)
        refused = int(flags.sum())
        # 5. all candidates of all trajectories in one launch, from knot 0
        cand.copy_envs_from(knots, first)
        if recorded:
            _, _, (o_c, _, d_c, _, _), (a_c, _), kobs_c = cand.rollout_schedule(K, table, want_outputs=True, want_actions=True,
                                                                              knots=cand_knots, want_knot_obs=True)
        else:
            _, _, (o_c, _, d_c, _, _), (a_c, _) = cand.rollout_schedule(K, table, want_outputs=True, want_actions=True)
        # 6. their costs
        J_c = cost(torch.cat([obs_k[:M].repeat(nal, 1)[None], o_c]), a_c).view(nal, M)
        # 7. the best step size that lowers the summed cost, or more regularisation
        total = J_c.sum(1)
        best = int(total.argmin())
        if float(total[best]) < float(J.sum()):
            it += 1
            alpha = ALPHAS[best]
            predicted = float((alpha * dv[:, :, 0].sum(0) + alpha ** 2 * dv[:, :, 1].sum(0)).mean())
            actual = float((J_c[best] - J).mean())
            shown_cost = float(J_c[best].mean())
            print(f"iter {it:2d} cost {shown_cost:.6e} alpha {alpha:5.3f} mu {mu:.3e} refused {refused} of {K * M} knots, predicted change "
                  f"{predicted:+.4e} actual {actual:+.4e}; {int((d_c.view(K, nal, M)[:, best] != 0).any(0).sum())} of {M} episodes ended"
                  + clamped_share(clamped), flush=True)
            U = a_c.view(K, nal, M, 2)[:, best].contiguous()
            if recorded:
                # the accepted candidate is the new nominal: its knots in one launch, its observations as they were recorded
                knots.copy_envs_from(cand_knots, best_lanes[best])
                obs_k = kobs_c.view(K, nal, M, D)[:, best].reshape(K * M, D)
                end_obs = o_c[K - 1].view(nal, M, D)[best]
            mu = 0.5 * mu if mu > 1e-3 else 0.0
        else:
            print(f"        no step size lowers the cost at mu {mu:.3e} (best alpha {ALPHAS[best]}: {float(total[best] - J.sum()) / M:+.4e}, "
                  f"refused {refused} of {K * M} knots): mu raised" + clamped_share(clamped), flush=True)
            mu = max(10.0 * mu, 0.1)
    while it < args.iters:                                                            # (kept: every iteration has its line)
        it += 1
        print(f"iter {it:2d} cost {shown_cost:.6e} (no step size was accepted)", flush=True)
    for e in envs:
        e.close()


def line_search_on_device(args, nom, knots, cand, cand_knots, start, target, Q, R, first):
    """The iteration with HipSim.ilqr_line_search: linearize, ilqr_backward, copy_envs_from (knot 0 -> candidates),
    rollout_schedule (recorded), ilqr_line_search, copy_envs_from (the accepted knots)."""
    M, K, nal = args.envs, args.steps, len(ALPHAS)
    dev, dt, D = nom.device, nom.dtype, nom.D
    alphas = torch.tensor(ALPHAS, dtype=dt, device=dev)
    # the first nominal, recorded: zero gains, zero bias; the line search with one candidate per trajectory initialises it
    table0 = torch.zeros(M, K, 2, D + 1, dtype=dt, device=dev)
    nom.restore(start)
    _, _, (o_n, _, d_n, _, _), (a_n, _), kobs = nom.rollout_schedule(K, table0, want_outputs=True, want_actions=True, knots=knots,
                                                                     want_knot_obs=True)
    choice, _, _, nominal = nom.ilqr_line_search(kobs, o_n[K - 1], a_n, target, Q, R, done=d_n, want_cand_cost=False)
    print(f"iter {0:2d} cost {float(nominal['cost'].mean()):.6e} (the nominal: zero torque; {int((choice < 0).sum())} of {M} trajectories "
          f"had an episode end inside it and stay out)", flush=True)
    a_k, obs_k = nominal["actions"].view(K * M, 2), nominal["obs"].view(K * M, D)        # views: updated in place by every call
    mu, it, tries = args.mu, 0, 0
    while it < args.iters and tries < 4 * args.iters:
        tries += 1
        _, _, A, B = knots.linearize(a_k, args.eps, want_next=False)
        (_, _, _, _, flags, dv, table), clamped = backward(nom, args.box, A, B, Q, R, knots=K, lx=nominal["lx_view"], lu=nominal["lu_view"],
                                                           mu=mu, p_final=nominal["p_final_view"], actions=a_k, obs=obs_k, alphas=ALPHAS,
                                                           want_gains=False, want_ff=False, want_weights=True)
        cand.copy_envs_from(knots, first)
        _, _, (o_c, _, d_c, _, _), (a_c, _), kobs_c = cand.rollout_schedule(K, table, want_outputs=True, want_actions=True,
                                                                          knots=cand_knots, want_knot_obs=True)
        before = nominal["cost"].clone()
        choice, index, _, _ = nom.ilqr_line_search(kobs_c, o_c[K - 1], a_c, target, Q, R, nominal=nominal, done=d_c, want_cand_cost=False)
        knots.copy_envs_from(cand_knots, index)
        accepted = bool((choice >= 0).any())                                          # the iteration's one decision on the host
        # (what follows is read back for the printed line only)
        took = torch.bincount(choice + 1, minlength=nal + 1).tolist()
        refused = int(flags.sum())
        if accepted:
            it += 1
            al = torch.where(choice >= 0, alphas[choice.clamp(min=0).long()], torch.zeros((), dtype=dt, device=dev))
            predicted = float((al * dv[:, :, 0].sum(0) + al * al * dv[:, :, 1].sum(0)).sum()) / M
            actual = float((nominal["cost"] - before).sum()) / M
            steps = ", ".join(f"{took[i + 1]} x {ALPHAS[i]}" for i in range(nal))
            print(f"iter {it:2d} cost {float(nominal['cost'].mean()):.6e} step sizes {steps}, none {took[0]}; mu {mu:.3e} refused {refused} of "
                  f"{K * M} knots, predicted change {predicted:+.4e} actual {actual:+.4e}" + clamped_share(clamped), flush=True)
            mu = 0.5 * mu if mu > 1e-3 else 0.0
        else:
            print(f"        no trajectory accepted a step size at mu {mu:.3e} (refused {refused} of {K * M} knots): mu raised"
                  + clamped_share(clamped), flush=True)
            mu = max(10.0 * mu, 0.1)
    while it < args.iters:                                                            # (kept: every iteration has its line)
        it += 1
        print(f"iter {it:2d} cost {float(nominal['cost'].mean()):.6e} (no step size was accepted)", flush=True)


def steered_on_device(args, nom, knots, cand, cand_knots, start, target, Q, R, first):
    """The iteration with HipSim.ilqr_steer and a mu per trajectory on the device: linearize, ilqr_backward(mu_dev=...),
    copy_envs_from (knot 0 -> candidates), rollout_schedule (recorded), ilqr_steer, copy_envs_from (the accepted knots); the host
    reads nothing inside the loop."""
    M, K, nal = args.envs, args.steps, len(ALPHAS)
    dev, dt, D = nom.device, nom.dtype, nom.D
    table0 = torch.zeros(M, K, 2, D + 1, dtype=dt, device=dev)
    nom.restore(start)
    _, _, (o_n, _, d_n, _, _), (a_n, _), kobs = nom.rollout_schedule(K, table0, want_outputs=True, want_actions=True, knots=knots,
                                                                     want_knot_obs=True)
    choice, _, _, nominal = nom.ilqr_line_search(kobs, o_n[K - 1], a_n, target, Q, R, done=d_n, want_cand_cost=False)
    nominal["mu"] = torch.full((M,), args.mu, dtype=dt, device=dev)
    print(f"iter {0:2d} cost {float(nominal['cost'].mean()):.6e} (the nominal: zero torque; {int((choice < 0).sum())} of {M} trajectories "
          f"had an episode end inside it and stay out)", flush=True)
    a_k, obs_k = nominal["actions"].view(K * M, 2), nominal["obs"].view(K * M, D)        # views: updated in place by every call
    edges = (0.0, 1e-3, 1e-1, 1e1, 1e3)
    if args.timing:
        import time
        torch.cuda.synchronize()
        began = time.perf_counter()
    for it in range(1, args.iters + 1):
        _, _, A, B = knots.linearize(a_k, args.eps, want_next=False)
        (_, _, _, _, _, dv, table), clamped = backward(nom, args.box, A, B, Q, R, knots=K, lx=nominal["lx_view"], lu=nominal["lu_view"],
                                                       mu_dev=nominal["mu"], p_final=nominal["p_final_view"], actions=a_k, obs=obs_k,
                                                       alphas=ALPHAS, want_gains=False, want_ff=False, want_flags=False, want_weights=True)
        cand.copy_envs_from(knots, first)
        _, _, (o_c, _, d_c, _, _), (a_c, _), kobs_c = cand.rollout_schedule(K, table, want_outputs=True, want_actions=True,
                                                                          knots=cand_knots, want_knot_obs=True)
        _, index, _, _ = nom.ilqr_steer(kobs_c, o_c[K - 1], a_c, target, Q, R, dv, ALPHAS, nominal=nominal, done=d_c, want_cand_cost=False,
                                        armijo=args.armijo, tol=args.tol)
        knots.copy_envs_from(cand_knots, index)
        if it == args.iters or (args.poll > 0 and it % args.poll == 0):
            # the poll: one look at the device
            cost, mu, status, iters = (nominal[k].cpu() for k in ("cost", "mu", "status", "iters"))
            hist = [int((mu == 0).sum())] + [int(((mu > lo) & (mu <= hi)).sum()) for lo, hi in zip(edges, edges[1:])] + [int((mu > edges[-1]).sum())]
            names = ["0"] + [f"<={hi:g}" for hi in edges[1:]] + [f">{edges[-1]:g}"]
            state = torch.bincount(status, minlength=3).tolist()
            print(f"iter {it:2d} cost {float(cost.mean()):.6e} mu " + ", ".join(f"{c} x {nm}" for c, nm in zip(hist, names)) +
                  f"; active {state[0]} converged {state[1]} stalled {state[2]}; accepted steps per trajectory {int(iters.min())}.."
                  f"{int(iters.max())}" + clamped_share(clamped), flush=True)
    if args.timing:
        torch.cuda.synchronize()
        print(f"time per iteration {1e3 * (time.perf_counter() - began) / max(args.iters, 1):.3f} ms (wall, polls included)", flush=True)


if __name__ == "__main__":
    main()
