"""libos2r_steer.so (include/os2r_steer.h) on the MI355X.  os2rt_ilqr_backward_mu against os2rc_ilqr_backward on the device and
against its numpy restatement run once per distinct mu; os2rt_ilqr_steer against os2rs_ilqr_line_search on the device and against
the numpy restatement of tests/test_ilqr_steer_host.py, bit for bit (the sign of a zero aside: it is not part of the contract);
stream order, the refusals that need a device, three steered iterations on real handles, and the example's steered mode."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import make_config
from gym_os2r_amd import abi
from test_gpu_ilqr_backward import ALL, OUTPUTS, R_COST, _dev, _np_dtype, _run, gradients, sims, synthetic, torch_mod  # noqa: F401  (fixtures)
from test_gpu_ilqr_backward import restate as restate_backward
from test_gpu_ilqr_line_search import IMARK, MARK, NOMINAL, PAD, Call, _same_bits, restate_crafted
from test_ilqr_steer_host import BRANCH_RULE, BRANCH_SHAPE, DEFAULTS, crafted_steer, restate_steer

pytestmark = pytest.mark.gpu

STATE = ("mu", "status", "iters")
NAMES_OF = dict(zip(NOMINAL, ("cost", "actions", "obs", "end_obs", "lx", "lu", "p_final")))       # the kernel's names -> HipSim's nominal


# ---------------------------------------------------------------------------------------
# os2rt_ilqr_backward_mu
# ---------------------------------------------------------------------------------------
def _backward_inputs(sim, K, M):
    n = 2 * sim.nq
    A, B, Q = synthetic(n, K * M)
    lx, lu, pv = gradients(n, K * M, M)
    rng = np.random.default_rng(11)
    return A, B, Q, dict(lx=lx, lu=lu, p_final=pv, P_final=Q[:, :, None] * (1.0 + 0.01 * np.arange(M)),
                         actions=rng.uniform(-1.3, 1.3, (K * M, 2)), obs=rng.uniform(-2.0, 2.0, (K * M, sim.D)))


# the smallest robot and the largest, K in {1, 2, 7}, M in {1, 33, 70}: one live lane, the 32-trajectory tail, three workgroups
BACKWARD_SHAPES = [("simple", abi.F64, 1, 1), ("simple", abi.F32, 2, 33), ("free_hip", abi.F64, 7, 70), ("free_hip", abi.F32, 2, 33),
                   ("simple", abi.F32, 7, 70), ("free_hip", abi.F64, 1, 1)]


@pytest.mark.parametrize("c", [0.0, 0.5])
@pytest.mark.parametrize("mode,dtype,K,M", BACKWARD_SHAPES)
def test_a_constant_mu_dev_is_the_scalar_mu_bit_for_bit(sims, torch_mod, mode, dtype, K, M, c):
    torch = torch_mod
    sim = sims(mode, dtype)
    A, B, Q, kw = _backward_inputs(sim, K, M)
    al = (1.0, 0.5, 0.0)
    want = _run(torch, sim, A, B, Q, R_COST, K, mu=c, alphas=al, **dict(kw), **ALL)
    mu_dev = torch.full((M,), c, dtype=sim.dtype, device=sim.device)
    got = _run(torch, sim, A, B, Q, R_COST, K, mu_dev=mu_dev, alphas=al, **dict(kw), **ALL)
    for o in OUTPUTS:
        assert torch.equal(got[o], want[o]), o
    assert not bool(want["flags"].any()) and bool((want["ff"] != 0).any()) and bool(torch.equal(mu_dev, torch.full_like(mu_dev, c)))


@pytest.mark.parametrize("mode,dtype,K,M", BACKWARD_SHAPES[1:5])
def test_a_mixed_mu_dev_equals_the_restatement_run_once_per_value(sims, torch_mod, mode, dtype, K, M):
    """0, 0.1, 3, one negative and one NaN entry side by side: every trajectory gets what the restatement gives the whole batch
    under its mu.  The invalid entries run as mu = 0 with every knot refused: the restatement with B = 0 and R = 0, whose 2 x 2
    system is refused at every knot and whose P' and p' are Q + A'PA and Qx with zero products added."""
    from gym_os2r_amd.control import slot_columns
    torch = torch_mod
    sim = sims(mode, dtype)
    dt = _np_dtype(sim)
    A, B, Q, kw = _backward_inputs(sim, K, M)
    al = (1.0, 0.5, 0.0)
    values = np.array([0.0, 0.1, 3.0, -1.0, np.nan])
    pick = np.arange(M) % 5
    mu = values[pick]
    got = _run(torch, sim, A, B, Q, R_COST, K, mu_dev=_dev(torch, sim, mu.astype(dt)), alphas=al, **dict(kw), **ALL)
    cols = slot_columns(sim.cfg.task, sim.nq)
    lanes = dict(gains=1, ff=1, P=1, p=1, flags=1, dv=1, weights=len(al))          # how often the trajectory index repeats in the last axis
    for v in range(5):
        ms = pick == v
        if v < 3:
            want = restate_backward(A, B, Q, R_COST, K, dt, mu=values[v], cols=cols, alphas=al, **kw)
            assert not want["flags"].any()
        else:
            want = restate_backward(A, np.zeros_like(B), Q, np.zeros((2, 2)), K, dt, mu=0.0, cols=cols, alphas=al, **kw)
            assert want["flags"].all() and not want["gains"].any() and not want["ff"].any() and not want["dv"].any()
        for o in OUTPUTS:
            sel = np.tile(ms, lanes[o])
            _same_bits(got[o].cpu().numpy()[..., sel], np.ascontiguousarray(want[o][..., sel]), f"mu {values[v]}: {o}")
        assert np.isfinite(want["P"]).all() and np.isfinite(want["p"]).all()


def test_backward_mu_is_ordered_on_the_stream_it_is_given(sims, torch_mod):
    """mu_dev holds 0; on a non-default stream a fill with 0.5 is enqueued and the call right behind it, with nothing between
    them but the stream's order (every tensor is on the device before): the call sees 0.5."""
    torch = torch_mod
    sim = sims("free_hip", abi.F64)
    K, M, n = 2, 33, 2 * sim.nq
    A, B, Q, kw = _backward_inputs(sim, K, M)
    a, b, lx, lu = (_dev(torch, sim, x) for x in (A, B, kw["lx"], kw["lu"]))
    new = lambda: dict(gains_out=torch.zeros(K, 2, n, M, dtype=sim.dtype, device=sim.device),
                       ff_out=torch.zeros(K, 2, M, dtype=sim.dtype, device=sim.device), dv_out=torch.zeros(K, 2, M, dtype=sim.dtype, device=sim.device))
    want, zero, got = new(), new(), new()
    sim.ilqr_backward_into(a, b, Q, R_COST, knots=K, lx=lx, lu=lu, mu=0.5, **want)
    sim.ilqr_backward_into(a, b, Q, R_COST, knots=K, lx=lx, lu=lu, mu=0.0, **zero)
    mu_dev = torch.zeros(M, dtype=sim.dtype, device=sim.device)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert not torch.equal(want["gains_out"], zero["gains_out"])
    with torch.cuda.stream(side):
        mu_dev.fill_(0.5)
        sim.ilqr_backward_into(a, b, Q, R_COST, knots=K, lx=lx, lu=lu, mu_dev=mu_dev, **got)
    torch.cuda.synchronize()
    for o in want:
        assert torch.equal(got[o], want[o]), o


# ---------------------------------------------------------------------------------------
# os2rt_ilqr_steer: the raw call on torch tensors
# ---------------------------------------------------------------------------------------
class SteerCall(Call):
    """One os2rt_ilqr_steer call through ctypes: test_gpu_ilqr_line_search.Call's buffers (every nominal and output array between
    guard bands), and mu, status, iters and dv next to them."""

    def __init__(self, torch, c, nq, dtype):
        super().__init__(torch, c, nq, dtype)
        from gym_os2r_amd import steer
        self.steer = steer.load()
        dt = np.float64 if dtype == abi.F64 else np.float32
        dev = torch.device("cuda:0")
        put = lambda x, t: torch.as_tensor(np.ascontiguousarray(np.asarray(x).astype(t))).to(dev)
        self.dv = put(c["dv"], dt)
        for name, t in (("mu", dt), ("status", np.int32), ("iters", np.int32)):
            band = np.full(PAD, IMARK if t is np.int32 else MARK, t)
            self.bufs[name] = put(np.concatenate([band, np.asarray(c[name]).astype(t), band]), t)
            self.inner[name] = self.bufs[name][PAD:-PAD]
            self.before[name] = self.bufs[name].clone()

    def run(self, rule=DEFAULTS, leave_out=(), stream=None, device=0, no_done=False):
        from gym_os2r_amd import control, steer
        torch, c, n = self.torch, self.c, 2 * self.nq
        K, M, nal = self.dims
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        arg = lambda name: None if name in leave_out else p(self.inner[name])
        lay = control.layout(self.dtype, self.nq, device, c["cols"])
        q = (ctypes.c_double * (n * n))(*c["Q"].reshape(-1))
        r = (ctypes.c_double * 4)(*c["R"].reshape(-1))
        qf = (ctypes.c_double * (n * n))(*c["Qf"].reshape(-1))
        al = (ctypes.c_double * nal)(*c["alphas"][:nal])
        st = stream if stream is not None else torch.cuda.current_stream()
        ins = [p(t) for t in self.inputs]
        if no_done:
            ins[3] = None
        self.rc = self.steer.os2rt_ilqr_steer(ctypes.byref(lay), K, M, nal, *ins, q, r, qf, p(self.dv), al, ctypes.byref(steer.Os2rSteerRule(**rule)),
                                              p(self.inner["cost"]), *[arg(k) for k in NOMINAL[1:]], p(self.inner["mu"]),
                                              p(self.inner["status"]), arg("iters"), p(self.inner["choice"]), arg("index"), arg("cand_cost"),
                                              ctypes.c_void_p(st.cuda_stream))
        self.error = self.steer.os2rt_last_error()
        return self

    def check(self, want, what, leave_out=()):
        super().check(want, what, leave_out)            # every buffer against the restatement, the guard bands, the refused trajectories
        frozen = self.torch.as_tensor(self.c["status"] != 0).to(self.bufs["mu"].device)
        for name in STATE + ("cost",):                  # a frozen trajectory: byte for byte what it was
            was = self.before[name][PAD:-PAD]
            assert self.torch.equal(was[frozen].view(self.torch.uint8), self.inner[name][frozen].view(self.torch.uint8)), (what, name)


def _np(dtype):
    return np.float64 if dtype == abi.F64 else np.float32


# nq, D, K, M, nalpha: K in {1, 2, 7}, M in {1, 33, 70} (the 64-trajectory tail), nalpha in {1, 3, 16}
STEER_SHAPES = [(2, 4, 1, 1, 1), (2, 4, 2, 33, 3), (5, 10, 7, 70, 16), (5, 10, 2, 33, 3), (2, 5, 7, 70, 16)]


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("nq,D,K,M,nalpha", STEER_SHAPES)
def test_without_armijo_and_with_every_status_0_it_is_the_line_search_on_the_device(torch_mod, dtype, nq, D, K, M, nalpha):
    """choice, index, cost, every nominal array and cand_cost against os2rs_ilqr_line_search on the same inputs, buffer by buffer
    with the guard bands; mu, status and iters (and once more everything else) against the restated rule."""
    torch = torch_mod
    c = crafted_steer(nq, D, K, M, nalpha, _np(dtype))
    c["status"] = np.zeros(M, np.int32)
    theirs = Call(torch, c, nq, dtype).run()
    assert theirs.rc == abi.OK, theirs.error
    ours = SteerCall(torch, c, nq, dtype).run(rule=DEFAULTS)
    want = restate_steer(c, _np(dtype), DEFAULTS)
    ours.check(want, f"{(nq, D, K, M, nalpha)} {dtype}")
    for name in theirs.bufs:
        assert torch.equal(ours.bufs[name].view(torch.uint8), theirs.bufs[name].view(torch.uint8)), name
    assert np.array_equal(want["choice"], restate_crafted(c, _np(dtype))["choice"])


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_every_branch_of_the_rule_equals_the_restatement_bit_for_bit(torch_mod, dtype):
    """The inputs tests/test_ilqr_steer_host.py holds to reach every branch: accepted with mu shrunk or set to 0, converged,
    refused by Armijo, a non-finite predicted change, raised, stalled, an invalid mu, frozen on entry, a done flag, a tie."""
    nq, D, K, M, nalpha = BRANCH_SHAPE
    c = crafted_steer(nq, D, K, M, nalpha, _np(dtype))
    want = restate_steer(c, _np(dtype), BRANCH_RULE)
    assert want["branches"]["converged"].any() and want["branches"]["stalled"].any() and (c["status"] != 0).any()
    SteerCall(torch_mod, c, nq, dtype).run(rule=BRANCH_RULE).check(want, f"branches {dtype}")


def test_each_nullable_argument_left_out_leaves_the_others_as_they_are(torch_mod):
    nq, D, K, M, nalpha = BRANCH_SHAPE
    c = crafted_steer(nq, D, K, M, nalpha, np.float64)
    want = restate_steer(c, np.float64, BRANCH_RULE)
    every = NOMINAL[1:] + ("index", "cand_cost", "iters")
    for name in every:
        SteerCall(torch_mod, c, nq, abi.F64).run(rule=BRANCH_RULE, leave_out=(name,)).check(want, f"without {name}", leave_out=(name,))
    SteerCall(torch_mod, c, nq, abi.F64).run(rule=BRANCH_RULE, leave_out=every).check(want, "the required ones alone", leave_out=every)
    want2 = restate_steer(dict(c, done=np.zeros_like(c["done"])), np.float64, BRANCH_RULE)
    assert not np.array_equal(want2["choice"], want["choice"])
    SteerCall(torch_mod, c, nq, abi.F64).run(rule=BRANCH_RULE, no_done=True).check(want2, "without done")


def test_steer_is_ordered_on_the_stream_it_is_given(torch_mod):
    """The device holds saturating actions; on a non-default stream a fill with 0.25 is enqueued and the call right behind it."""
    torch = torch_mod
    nq, D, K, M, nalpha = STEER_SHAPES[3]
    c = crafted_steer(nq, D, K, M, nalpha, np.float64)
    want = restate_steer(dict(c, act=np.full_like(c["act"], 0.25)), np.float64, BRANCH_RULE)
    c_dev = dict(c, act=np.full_like(c["act"], 7.0))
    assert not np.array_equal(restate_steer(c_dev, np.float64, BRANCH_RULE)["cand_cost"], want["cand_cost"])
    call = SteerCall(torch, c_dev, nq, abi.F64)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        call.inputs[2].fill_(0.25)
    call.run(rule=BRANCH_RULE, stream=side).check(want, "side stream")


def test_refusals_on_the_device(torch_mod, sims):
    torch = torch_mod
    from gym_os2r_amd import control, steer
    nq, D, K, M, nalpha = STEER_SHAPES[1]
    c = crafted_steer(nq, D, K, M, nalpha, np.float64)
    call = SteerCall(torch, c, nq, abi.F64).run(device=1000)
    assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(b"os2rt_ilqr_steer: "), (call.rc, call.error)
    torch.cuda.synchronize()
    assert all(torch.equal(call.bufs[k].view(torch.uint8), call.before[k].view(torch.uint8)) for k in call.bufs)       # a refused call wrote nothing (mu holds NaNs: bytes)
    bad = dict(c, Q=np.where(np.eye(2 * nq, k=1) > 0, 0.5, c["Q"]))
    call = SteerCall(torch, bad, nq, abi.F64).run()
    assert call.rc == abi.ERR_INVALID and call.error == b"os2rt_ilqr_steer: Q must be exactly symmetric"
    call = SteerCall(torch, c, nq, abi.F64).run(rule=dict(DEFAULTS, grow=0.5))
    assert call.rc == abi.ERR_INVALID and call.error == b"os2rt_ilqr_steer: rule grow must be >= 1"
    # os2rt_ilqr_backward_mu, raw: no such device, then a null mu_dev behind a valid one
    lib = steer.load()
    sim = sims("simple", abi.F64)
    n, Kb, Mb = 2 * sim.nq, 2, 3
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device="cuda:0")
    a, b, mu, gain = z(n, n, Kb * Mb), z(n, 2, Kb * Mb), z(Mb), torch.full((Kb, 2, n, Mb), MARK, dtype=torch.float64, device="cuda:0")
    q, r = (ctypes.c_double * (n * n))(*np.eye(n).reshape(-1)), (ctypes.c_double * 4)(0.1, 0.0, 0.0, 0.1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def backward(device, mu_arg):
        lay = control.layout(abi.F64, sim.nq, device, None)
        rc = lib.os2rt_ilqr_backward_mu(ctypes.byref(lay), Kb, Mb, p(a), p(b), None, None, q, r, mu_arg, None, None, p(gain), None, None, None,
                                        None, None, None, None, None, 0, None, None)
        return rc, lib.os2rt_last_error()
    rc, err = backward(1000, p(mu))
    assert rc == abi.ERR_NO_DEVICE and err.startswith(b"os2rt_ilqr_backward_mu: "), (rc, err)
    assert backward(0, None) == (abi.ERR_INVALID, b"os2rt_ilqr_backward_mu: null mu_dev")
    torch.cuda.synchronize()
    assert bool((gain == MARK).all())
    rc, err = backward(0, p(mu))
    torch.cuda.synchronize()
    assert rc == abi.OK and bool((gain == 0).all()), (rc, err)                     # B = 0: no gain
    # through HipSim: mu_dev together with a nonzero mu, on a handle that has a device
    A, B = z(Kb * Mb, n, n), z(Kb * Mb, n, 2)
    with pytest.raises(ValueError, match="^ilqr_backward: mu_dev and a nonzero mu"):
        sim.ilqr_backward(A, B, np.eye(n), 0.1 * np.eye(2), knots=Kb, mu=0.5, mu_dev=mu)
    with pytest.raises(ValueError, match="^ilqr_backward: mu_dev"):
        sim.ilqr_backward(A, B, np.eye(n), 0.1 * np.eye(2), knots=Kb, mu_dev=mu.float())


# ---------------------------------------------------------------------------------------
# three steered iterations on real handles
# ---------------------------------------------------------------------------------------
def test_three_steered_iterations_on_real_handles(torch_mod):
    """nq 5, M = 6, K = 5, four step sizes, no host value fed back: linearize, ilqr_backward(mu_dev), copy_envs_from, the recorded
    rollout, ilqr_steer, copy_envs_from.  After every launch pair ilqr_steer's outputs equal the restatement on the same device
    inputs, no trajectory's cost rises, and the knots handle holds exactly the accepted knots."""
    torch = torch_mod
    from gym_os2r_amd.control import slot_columns
    from gym_os2r_amd.sim import HipSim
    K, M, alphas = 5, 6, (1.0, 0.5, 0.25, 0.125)
    nal = len(alphas)
    N = nal * M
    rule = dict(DEFAULTS, armijo=1e-4, tol=1e-6)

    def make(num):
        cfg = make_config("free_hip", "BalancingV1", False, num_envs=num, contact=True, seed=5, auto_reset=False, dtype=abi.F64)[0]
        return HipSim(cfg)
    nom_h, cand, cand_knots, knots, knots_ref = make(M), make(N), make(K * N), make(K * M), make(K * M)
    D, n, dev = nom_h.D, 2 * nom_h.nq, nom_h.device
    assert nom_h.nq == 5
    cols = slot_columns(nom_h.cfg.task, nom_h.nq)
    qdiag = np.array([0.0 if c not in cols else (1.0 if c < nom_h.nq else 0.01) for c in range(n)])
    Q, R = np.diag(qdiag), 0.1 * np.eye(2)
    # the first nominal: zero torque, recorded; the target: where it starts
    table0 = torch.zeros(M, K, 2, D + 1, dtype=torch.float64, device=dev)
    _, _, (o_n, _, d_n, _, _), (a_n, _), kobs = nom_h.rollout_schedule(K, table0, want_outputs=True, want_actions=True, knots=knots,
                                                                       want_knot_obs=True)
    target = kobs[0].clone()
    _, _, _, nominal = nom_h.ilqr_line_search(kobs, o_n[K - 1], a_n, target, Q, R, done=d_n, want_cand_cost=False)
    nominal["mu"] = torch.tensor([0.0, 0.0, 0.1, 0.1, 1.0, 1e6], dtype=torch.float64, device=dev)
    nominal["status"], nominal["iters"] = (torch.zeros(M, dtype=torch.int32, device=dev) for _ in range(2))
    knots_ref.copy_envs_from(knots)
    first = torch.arange(M, dtype=torch.int32, device=dev).repeat(nal)
    a_k, obs_k = nominal["actions"].view(K * M, 2), nominal["obs"].view(K * M, D)
    lane = torch.arange(K * M, device=dev)
    cpu = lambda t: t.detach().cpu().numpy().copy()
    accepted = 0
    for it in range(3):
        _, _, A, B = knots.linearize(a_k, want_next=False)
        _, _, _, _, _, dv, table = nom_h.ilqr_backward(A, B, Q, R, knots=K, lx=nominal["lx_view"], lu=nominal["lu_view"], mu_dev=nominal["mu"],
                                                       p_final=nominal["p_final_view"], actions=a_k, obs=obs_k, alphas=alphas,
                                                       want_gains=False, want_ff=False, want_flags=False, want_weights=True)
        cand.copy_envs_from(knots, first)
        _, _, (o_c, _, d_c, _, _), (a_c, _), kobs_c = cand.rollout_schedule(K, table, want_outputs=True, want_actions=True,
                                                                          knots=cand_knots, want_knot_obs=True)
        torch.cuda.synchronize()                        # (the test looks; the iteration does not need it)
        c = dict(knot_obs=cpu(kobs_c), end_obs=cpu(o_c[K - 1]), act=cpu(a_c), done=cpu(d_c), target=cpu(target), Q=Q, R=R, Qf=None, cols=cols,
                 nominal={k: cpu(nominal[v]) for k, v in NAMES_OF.items()}, dv=cpu(dv.permute(0, 2, 1)), alphas=alphas,
                 **{k: cpu(nominal[k]) for k in STATE})
        choice, index, cand_cost, same = nom_h.ilqr_steer(kobs_c, o_c[K - 1], a_c, target, Q, R, dv, alphas, nominal=nominal, done=d_c, rule=rule)
        knots.copy_envs_from(cand_knots, index)
        torch.cuda.synchronize()
        assert same is nominal
        want = restate_steer(c, np.float64, rule)
        _same_bits(choice, want["choice"], f"iteration {it}: choice")
        _same_bits(index, want["index"], f"iteration {it}: index")
        _same_bits(cand_cost, want["cand_cost"], f"iteration {it}: cand_cost")
        for k, v in NAMES_OF.items():
            _same_bits(nominal[v], want["nominal"][k], f"iteration {it}: {v}")
        for k in STATE:
            _same_bits(nominal[k], want["nominal"][k], f"iteration {it}: {k}")
        assert (cpu(nominal["cost"]) <= c["nominal"]["cost"]).all(), it
        accepted += int((want["choice"] >= 0).sum())
        # exactly the accepted knots moved: a hand-made index on a second knots handle
        hand = torch.where(choice.long()[lane % M] >= 0, (lane // M) * N + choice.long()[lane % M] * M + lane % M, -1).to(torch.int32)
        knots_ref.copy_envs_from(cand_knots, hand)
        torch.cuda.synchronize()
        assert torch.equal(hand, index)

        def same_tree(x, y, key):
            if isinstance(x, dict):
                assert x.keys() == y.keys(), key
                for k in x:
                    same_tree(x[k], y[k], (key, k))
            else:
                assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y), key
        same_tree(knots.checkpoint(), knots_ref.checkpoint(), f"iteration {it}: checkpoint")
        assert torch.equal(knots.copy_envs_from(knots, want_obs=True).view(K, M, D), nominal["obs"])
    assert accepted > 0 and int(nominal["iters"].sum()) == accepted
    for s in (nom_h, cand, cand_knots, knots, knots_ref):
        s.close()


# ---------------------------------------------------------------------------------------
# the example's steered mode runs to its end
# ---------------------------------------------------------------------------------------
def test_example_with_the_steered_line_search_never_raises_the_mean_cost(torch_mod):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ilqr_balancing.py"), "--line-search", "steered", "--envs", "8",
                          "--steps", "6", "--iters", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    costs = [float(c) for c in re.findall(r"^iter +\d+ +cost +([-+0-9.eE]+)", out.stdout, re.M)]
    assert len(costs) == 2, out.stdout[-2000:]                      # the nominal and the one poll after the last iteration
    assert all(b <= a for a, b in zip(costs, costs[1:])), costs
    state = re.findall(r"active (\d+) converged (\d+) stalled (\d+)", out.stdout)
    assert len(state) == 1 and sum(int(v) for v in state[0]) == 8, out.stdout[-2000:]
