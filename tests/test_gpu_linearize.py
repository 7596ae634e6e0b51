"""os2r_linearize (include/os2r.h) on the MI355X: finite-difference Jacobians of one env-step in one launch.  The yardstick is
never the new code against itself: (a) the path a caller had to compose before -- a fork handle of P*N environments,
copy_envs_from, perturb in torch, set_state, set_solver_state, step, get_state, quotients in torch -- compared with
torch.equal; (d) the fp64 CPU oracle evaluated at the same points, within the one-step bound of
test_one_step_matches_oracle_f64."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import lying_states, make_config, mixed_axis_chain
from gym_os2r_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def HipSim(torch_mod):
    from gym_os2r_amd.sim import HipSim
    return HipSim


def _default_eps(torch, dtype):
    return float(torch.finfo(dtype).eps) ** (1.0 / 3.0)


def _factory(HipSim, mode, dtype=abi.F64, dr=False, binding=None, **kw):
    """-> (make(n, contact=True) -> HipSim without auto-reset, model dict): handles that differ in num_envs / contact only."""
    extra = dict(reset_mode=abi.RESET_RANDOM, randomize_params=True) if dr else {}
    reward = "StraightV1" if mode == "simple" else "BalancingV1"
    model = make_config(mode, reward, True, num_envs=1)[2]

    def make(n, contact=True):
        cfg = make_config(mode, reward, True, num_envs=n, contact=contact, seed=5, auto_reset=False, dtype=dtype, **extra, **kw)[0]
        return HipSim(cfg, binding=binding)
    return make, model


def _actions(torch, sim, eps_a, seed=3):
    """Nominal actions over [-1.3, 1.3] with, as far as N allows, exact +-1, values within eps_a of a limit, values outside."""
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(sim.N, 2, generator=g, dtype=torch.float64) * 2.6 - 1.3)
    special = [(1.0, -1.2)] if sim.N == 1 else [(1.0, -1.0), (1.0 - 0.5 * eps_a, -1.0 + 0.25 * eps_a), (1.2, -1.5), (-1.0, 1.0 - 0.9 * eps_a)]
    for k, v in enumerate(special[:sim.N]):
        a[k] = torch.tensor(v, dtype=torch.float64)
    return a.to(sim.dtype).to(sim.device)


def _points(torch, q, qd, act, eps, N):
    """The evaluation points by the rule of include/os2r.h, in the tensors' dtype: blocks of N environments, block 2c the upper
    and 2c + 1 the lower point of column c (the 2nq state columns, then the two action columns), the last block the nominal
    point.  q, qd [nq, P*N] and act [P*N, 2] hold P copies of the nominal values and are perturbed in place; the clamp of the
    nominal action comes first."""
    nq = q.shape[0]
    dt = q.dtype
    h = [torch.tensor(e, dtype=dt, device=q.device) for e in eps]
    one = torch.tensor(1.0, dtype=dt, device=q.device)
    act.clamp_(-1.0, 1.0)
    for c in range(2 * nq):
        x, row, step = (q, c, h[0]) if c < nq else (qd, c - nq, h[1])
        hi, lo = slice(2 * c * N, (2 * c + 1) * N), slice((2 * c + 1) * N, (2 * c + 2) * N)
        x[row, hi] = x[row, hi] + step
        x[row, lo] = x[row, lo] - step
    for j in range(2):
        c = 2 * nq + j
        hi, lo = slice(2 * c * N, (2 * c + 1) * N), slice((2 * c + 1) * N, (2 * c + 2) * N)
        act[hi, j] = torch.minimum(act[hi, j] + h[2], one)
        act[lo, j] = torch.maximum(act[lo, j] - h[2], -one)


def _quotients(torch, x_in, f_out, N, nq):
    """x_in [2nq + 2, P*N] (q, qd, the two actions as evaluated), f_out [2nq, P*N], host tensors -> next [2nq, N], A [N, 2nq, 2nq],
    B [N, 2nq, 2]: one rounded subtraction above, one below, one IEEE division."""
    n2 = 2 * nq
    cols = []
    for c in range(n2 + 2):
        hi, lo = slice(2 * c * N, (2 * c + 1) * N), slice((2 * c + 1) * N, (2 * c + 2) * N)
        cols.append((f_out[:, hi] - f_out[:, lo]) / (x_in[c, hi] - x_in[c, lo])[None, :])     # [2nq, N]
    J = torch.stack(cols, dim=1)                       # [2nq, 2nq + 2, N]
    nominal = slice(2 * (n2 + 2) * N, (2 * (n2 + 2) + 1) * N)
    return f_out[:, nominal], J[:, :n2].permute(2, 0, 1), J[:, n2:].permute(2, 0, 1)


def _composed(torch, make, sim, actions, eps):
    """What a caller had to do before: about ten launches, two host synchronisations, a P-fold copy of every array."""
    N, nq = sim.N, sim.nq
    P = 2 * (2 * nq + 2) + 1
    fork = make(P * N)
    index = torch.arange(N, dtype=torch.int32, device=sim.device).repeat(P)
    fork.copy_envs_from(sim, index)
    q, qd = fork.get_state()
    lam, flags = fork.get_solver_state()
    act = actions.repeat(P, 1).contiguous()
    _points(torch, q, qd, act, eps, N)
    fork.set_state(q, qd)
    fork.set_solver_state(lam, flags)
    fork.step(act)
    fq, fqd = fork.get_state()
    torch.cuda.synchronize()
    x_in = torch.cat([q, qd, act.t()]).cpu()
    out = _quotients(torch, x_in, torch.cat([fq, fqd]).cpu(), N, nq)
    fork.close()
    return out


def _assert_equal(torch, got, want, what):
    """torch.equal; in f32 an entry whose reference quotient is subnormal may also be zero (fixed in advance: every other entry
    is exact)."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert bool(torch.isfinite(want).all()), what
    bad = got != want
    if got.dtype == torch.float32:
        tiny = torch.finfo(torch.float32).tiny
        bad &= ~((want.abs() < tiny) & (got == 0))
    assert not bool(bad.any()), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


def _violations(torch, sim):
    v = torch.zeros(1, dtype=torch.int32, device=sim.device)
    sim.action_violations_into(v, clear=False)
    torch.cuda.synchronize()
    return int(v[0])


def _check_case(torch, make, sim, contact_flags, differs_from_contact_off):
    """(a) for one prepared handle: next, A and B of the fused call equal the composed path's, bit for bit; the contact path was
    exercised where the case says so; the handle counted no violation."""
    eps = (_default_eps(torch, sim.dtype),) * 3
    actions = _actions(torch, sim, eps[2])
    assert bool((actions.abs() > 1).any()) and bool((actions.abs() == 1).any())
    nq = sim.nq
    next_q, next_qd, A, B = sim.linearize(actions, eps)
    assert A.shape == (sim.N, 2 * nq, 2 * nq) and B.shape == (sim.N, 2 * nq, 2) and next_q.shape == (nq, sim.N)
    want_next, want_A, want_B = _composed(torch, make, sim, actions, eps)
    _assert_equal(torch, torch.cat([next_q, next_qd]), want_next, "next")
    _assert_equal(torch, A, want_A, "A")
    _assert_equal(torch, B, want_B, "B")
    assert bool((A != 0).any()) and bool((B != 0).any())
    # one-sided at a torque limit: the environments whose nominal action sits on +1 / -1 still have a finite column of B
    assert bool(torch.isfinite(B).all())
    if contact_flags:
        touching = (sim.get_solver_state()[1] & ((1 << nq) - 1)) != 0
        assert int(touching.sum()) * 2 >= sim.N, int(touching.sum())
    if differs_from_contact_off:
        # A contact flag says that a body was within the contact margin in the last physics iteration, not that the ground
        # pushed: under random torques the robots bounce, and an environment in flight at all its evaluation points has,
        # correctly, the Jacobian of the contact-off handle, bit for bit; others graze the ground at some points only.  With
        # the fp64 oracle on the CPU, A differs from the contact-off A in 28 to 32 of the 64 / 65 environments of these states
        # (54 of the 130 with per-env parameters, 25 of 65 with the sweeps-only solver).
        # Which environments those are is decided by the path that existed before, not by the new code: the composed path
        # on contact-off handles from the same states.  The fused call must name exactly the same environments, and they must
        # be at least a quarter of all (the oracle's count with a margin), or the contact path was not exercised.
        off = make(sim.N, contact=False)
        off.copy_envs_from(sim)
        A_off = off.linearize(actions, eps, want_next=False, want_B=False)[2]
        want_A_off = _composed(torch, lambda n: make(n, contact=False), off, actions, eps)[1]
        off.close()
        _assert_equal(torch, A_off, want_A_off, "A, contact off")
        differs = (A != A_off).flatten(1).any(1).cpu()
        differs_composed = (want_A != want_A_off).flatten(1).any(1)
        print(f"[linearize, contact] {sim.N} environments: A differs from contact-off in {int(differs.sum())} (composed path: {int(differs_composed.sum())})")
        assert torch.equal(differs, differs_composed)
        assert int(differs_composed.sum()) * 4 >= sim.N, int(differs_composed.sum())
    assert _violations(torch, sim) == 0 and int(sim.violation_mirror()[0]) == 0


def _lying(torch, sim, model, preroll=150):
    """Fallen robots (helpers.lying_states, seed 5) after `preroll` env-steps with device-drawn actions: on the ground, the
    solver state populated.  With the fp64 oracle on the CPU, 80-95 % of the environments of every case below carry a contact
    at that point (free_hip with per-env parameters N = 130: 0.80; fixed_hip_simple 65: 0.91; fixed 64: 0.89; free_hip 65:
    0.91)."""
    q, qd = lying_states(model, sim.N, np.random.default_rng(5))
    sim.set_state(q, qd)
    for _ in range(preroll):
        sim.step(None, want_terminal=False)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_free_hip_with_contact_and_per_env_parameters_equals_the_composed_path(HipSim, torch_mod, dtype):
    """nq 5, ground contact, randomised per-env parameters, N = 130: two full waves and a tail of 2."""
    make, model = _factory(HipSim, "free_hip", dtype, dr=True)
    sim = make(130)
    _lying(torch_mod, sim, model)
    mass = sim.get_params(abi.PARAM_MASS_SCALE)
    assert bool((mass != mass[:, :1]).any())                 # the parameters do differ between the environments
    _check_case(torch_mod, make, sim, contact_flags=dtype == abi.F64, differs_from_contact_off=dtype == abi.F64)
    sim.close()


@pytest.mark.parametrize("mode,n,binding", [("fixed_hip_simple", 65, "ctypes"), ("fixed", 64, "ctypes"), ("fixed", 64, "pybind11")])
def test_compiled_in_robots_with_uniform_parameters_equal_the_composed_path(HipSim, torch_mod, mode, n, binding):
    make, model = _factory(HipSim, mode, binding=binding)
    sim = make(n)
    assert sim.binding == binding
    _lying(torch_mod, sim, model)
    _check_case(torch_mod, make, sim, contact_flags=True, differs_from_contact_off=True)
    sim.close()


def test_two_dof_robot_without_contact_candidates_single_environment(HipSim, torch_mod):
    make, model = _factory(HipSim, "simple")
    sim = make(1)
    rng = np.random.default_rng(5)
    sim.set_state(rng.uniform(-1.2, 1.2, (2, 1)), rng.uniform(-3, 3, (2, 1)))
    for _ in range(20):
        sim.step(None, want_terminal=False)
    _check_case(torch_mod, make, sim, contact_flags=False, differs_from_contact_off=False)
    sim.close()


@pytest.mark.parametrize("mode,solver", [("free_hip", dict(pgs_exact=0, pgs_iters=abi.DEFAULT_PGS_ITERS)),
                                         ("fixed_hip", dict(pgs_exact=3, pgs_iters=9, pgs_normal_iters=3))])
def test_non_default_solver_settings_equal_the_composed_path(HipSim, torch_mod, mode, solver):
    """pgs_exact = 0: the fp64 sweeps-only kernels (no solver state is carried); a non-default exact finish: run-time sweep
    counts."""
    make, model = _factory(HipSim, mode, **solver)
    sim = make(65)
    _lying(torch_mod, sim, model)
    _check_case(torch_mod, make, sim, contact_flags=solver["pgs_exact"] > 0, differs_from_contact_off=True)
    sim.close()


def test_run_time_chain_on_the_generic_kernels_equals_the_composed_path(HipSim, torch_mod, tmp_path, monkeypatch):
    """helpers.mixed_axis_chain (3 dofs, axes z, y, x, candidates on every body) on the run-time-model kernels (OS2R_JIT=0);
    after 150 env-steps from its reset every environment rests on the ground (oracle: contact fraction 1.0)."""
    monkeypatch.setenv("OS2R_JIT", "0")
    torch = torch_mod
    m, spec = mixed_axis_chain(tmp_path)

    def make(n, contact=True):
        return HipSim(abi.config_struct(m, spec, num_envs=n, dtype=abi.F64, contact=contact, auto_reset=False, seed=5))
    sim = make(65)
    assert not sim.specialised
    for _ in range(150):
        sim.step(None, want_terminal=False)
    _check_case(torch, make, sim, contact_flags=True, differs_from_contact_off=True)
    sim.close()


# ---------------------------------------------------------------------------------------
# (b) the handle is only read
# ---------------------------------------------------------------------------------------
def _flat(ck):
    out = {k: v for k, v in ck.items() if k not in ("params", "step_count")}
    out.update({f"param{f}": v for f, v in ck["params"].items()})
    return out


def _assert_untouched(torch, sim, before, count, mirror, what):
    torch.cuda.synchronize()
    after = _flat(sim.checkpoint())
    for k, v in _flat(before).items():
        assert after[k].dtype == v.dtype and torch.equal(after[k], v), (what, k)
    assert sim.step_count == count == before["step_count"], what
    assert list(sim.violation_mirror()) == mirror, what
    assert _violations(torch, sim) == 0, what


def test_the_handle_is_untouched(HipSim, torch_mod):
    torch = torch_mod
    make, model = _factory(HipSim, "free_hip", dr=True)
    sim = make(130)
    _lying(torch, sim, model, preroll=30)
    torch.cuda.synchronize()
    before, count, mirror = sim.checkpoint(), sim.step_count, list(sim.violation_mirror())
    assert bool((before["solver_flags"] != 0).any()) and count == 30
    actions = _actions(torch, sim, 1e-5)
    full = sim.linearize(actions)
    _assert_untouched(torch, sim, before, count, mirror, "all outputs")
    for which in ("next", "A", "B"):
        out = sim.linearize(actions, want_next=which == "next", want_A=which == "A", want_B=which == "B")
        _assert_untouched(torch, sim, before, count, mirror, which)
        for i, (got, ref) in enumerate(zip(out, full)):       # an output alone is the same output
            assert (got is not None) == (i in {"next": (0, 1), "A": (2,), "B": (3,)}[which]), (which, i)
            if got is not None:
                assert torch.equal(got, ref), which
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = sim.linearize(actions)
    torch.cuda.current_stream().wait_stream(side)
    _assert_untouched(torch, sim, before, count, mirror, "side stream")
    for got, ref in zip(out, full):
        assert torch.equal(got, ref)
    # and the handle goes on as if nothing had happened: the next step equals a twin's that never linearised
    twin = make(130)
    twin.restore(before)
    a = actions.clamp(-1, 1)
    for x, y in zip(sim.step(a), twin.step(a)):
        assert torch.equal(x, y)
    sim.close(); twin.close()


# ---------------------------------------------------------------------------------------
# (c) no write outside the outputs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
def test_no_write_outside_the_outputs(HipSim, torch_mod, n):
    torch = torch_mod
    make, model = _factory(HipSim, "fixed_hip_simple")
    sim = make(n)
    _lying(torch, sim, model, preroll=5)
    n2, pad, mark = 2 * sim.nq, 64, -12345.5
    bufs = {name: torch.full((pad + rows * n + pad,), mark, dtype=sim.dtype, device=sim.device)
            for name, rows in (("next", n2), ("A", n2 * n2), ("B", n2 * 2))}
    actions = _actions(torch, sim, 1e-5)
    eps = (ctypes.c_double * 3)(1e-5, 1e-4, 1e-3)
    at = lambda t: ctypes.c_void_p(t.data_ptr() + pad * t.element_size())
    lib = sim._lib
    rc = lib.os2r_linearize(sim._h, ctypes.c_void_p(actions.data_ptr()), eps, at(bufs["next"]), at(bufs["A"]), at(bufs["B"]),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == abi.OK, lib.os2r_last_error(sim._h)
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t[:pad] == mark).all()) and bool((t[-pad:] == mark).all()), name
        assert not bool((t[pad:-pad] == mark).any()), name          # and every element of the extent was written
    # the raw layout is the documented one: [2nq][width][N], the environment index fastest
    _, _, A, B = sim.linearize(actions, (1e-5, 1e-4, 1e-3), want_next=False)
    assert torch.equal(bufs["A"][pad:-pad].view(n2, n2, n).permute(2, 0, 1), A)
    assert torch.equal(bufs["B"][pad:-pad].view(n2, 2, n).permute(2, 0, 1), B)
    sim.close()


# ---------------------------------------------------------------------------------------
# (d) the fp64 oracle at the same points
# ---------------------------------------------------------------------------------------
T1 = 3e-9     # the one-step bound of test_one_step_matches_oracle_f64 for these configurations


@pytest.mark.parametrize("mode,contact", [("fixed_hip", False), ("free_hip", True)])
def test_jacobians_match_the_oracle_within_the_one_step_bound(HipSim, torch_mod, oracle, mode, contact):
    """Both sides evaluate f at the same 2 (2nq + 2) + 1 points per environment; each evaluation is within T1 max(|f|, 1) of the
    oracle's (the asserted one-step bound), so a quotient is within 2 T1 max(|f|, 1) / (hi - lo)."""
    torch = torch_mod
    n = 64
    cfg, _, model = make_config(mode, "BalancingV2", True, num_envs=n, contact=contact, auto_reset=False, dtype=abi.F64)
    rng = np.random.default_rng(3)
    sim = HipSim(cfg)
    nq = sim.nq
    if contact:
        q, qd = lying_states(model, n, rng)
        sim.set_state(q, qd)
        for _ in range(5):
            sim.step(torch.as_tensor(rng.uniform(-1, 1, (n, 2))), want_terminal=False)
    else:
        sim.set_state(rng.uniform(-1.2, 1.2, (nq, n)), rng.uniform(-8, 8, (nq, n)))
    eps = (_default_eps(torch, torch.float64),) * 3
    actions = _actions(torch, sim, eps[2])
    next_q, next_qd, A, B = sim.linearize(actions, eps)
    torch.cuda.synchronize()
    P = 2 * (2 * nq + 2) + 1
    q, qd = (t.cpu().repeat(1, P) for t in sim.get_state())
    lam, flags = sim.get_solver_state()
    if contact:
        assert int(((flags & ((1 << nq) - 1)) != 0).sum()) * 2 >= n
    act = actions.cpu().repeat(P, 1).contiguous()
    _points(torch, q, qd, act, eps, n)
    ocfg = make_config(mode, "BalancingV2", True, num_envs=P * n, contact=contact, auto_reset=False, dtype=abi.F64)[0]
    orc = oracle.OracleSim(ocfg, threads=8)
    orc.set_state(q.numpy(), qd.numpy())
    orc.set_solver_state(lam.cpu().repeat(1, P).numpy(), flags.cpu().repeat(P).numpy().view(np.uint32))
    orc.step(act.numpy())
    f = torch.from_numpy(np.concatenate(orc.get_state()))
    x_in = torch.cat([q, qd, act.t()])
    o_next, o_A, o_B = _quotients(torch, x_in, f, n, nq)
    scale = f.abs().clamp(min=1.0)                                             # max(|f|, 1) per evaluation
    r_next = ((torch.cat([next_q, next_qd]).cpu() - o_next).abs() / (T1 * scale[:, -n:])).max()
    ratios = {"next": float(r_next)}
    for name, got, want, c0, ncol in (("A", A, o_A, 0, 2 * nq), ("B", B, o_B, 2 * nq, 2)):
        worst = 0.0
        for j in range(ncol):
            c = c0 + j
            hi, lo = slice(2 * c * n, (2 * c + 1) * n), slice((2 * c + 1) * n, (2 * c + 2) * n)
            bound = 2 * T1 * torch.maximum(scale[:, hi], scale[:, lo]) / (x_in[c, hi] - x_in[c, lo])[None, :]     # [2nq, N]
            err = (got.cpu()[:, :, j] - want[:, :, j]).abs().t()                                                     # [2nq, N]
            worst = max(worst, float((err / bound).max()))
        ratios[name] = worst
    print(f"[linearize vs oracle, {mode}, contact={contact}] largest error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert all(np.isfinite(v) and v <= 1.0 for v in ratios.values()), ratios
    sim.close(); orc.close()


# ---------------------------------------------------------------------------------------
# (e) refusals
# ---------------------------------------------------------------------------------------
def test_refusals_name_their_cause(HipSim, torch_mod):
    torch = torch_mod
    make, _ = _factory(HipSim, "fixed")
    sim = make(64)
    before = sim.checkpoint()
    lib = sim._lib
    n2 = 2 * sim.nq
    act = torch.zeros(64, 2, dtype=sim.dtype, device=sim.device)
    out = torch.zeros(n2 * n2 * 64, dtype=sim.dtype, device=sim.device)
    a, o = ctypes.c_void_p(act.data_ptr()), ctypes.c_void_p(out.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    E = lambda *v: (ctypes.c_double * 3)(*v)
    nan, inf = float("nan"), float("inf")
    assert lib.os2r_linearize(None, a, E(1e-6, 1e-6, 1e-6), o, None, None, st) == abi.ERR_INVALID
    assert b"null handle" in lib.os2r_last_error(None)
    for args, msg in (((None, E(1e-6, 1e-6, 1e-6), o, None, None), b"null actions"),
                      ((a, None, o, None, None), b"null eps"),
                      ((a, E(1e-6, 1e-6, 1e-6), None, None, None), b"outputs are null"),
                      ((a, E(nan, 1e-6, 1e-6), None, o, None), b"finite"),
                      ((a, E(1e-6, -nan, 1e-6), None, o, None), b"finite"),
                      ((a, E(1e-6, 1e-6, inf), None, o, None), b"finite"),
                      ((a, E(0.0, 1e-6, 1e-6), None, o, None), b"positive"),
                      ((a, E(1e-6, -1e-6, 1e-6), None, o, None), b"positive"),
                      ((a, E(1e-6, 1e-6, 1.0), None, o, None), b"< 1"),
                      ((a, E(1e-6, 1e-6, 2.5), None, o, None), b"< 1")):
        rc = lib.os2r_linearize(sim._h, *args, st)
        assert rc == abi.ERR_INVALID and msg in lib.os2r_last_error(sim._h), (msg, rc, lib.os2r_last_error(sim._h))
    from gym_os2r_amd.sim import Os2rError
    f32 = _factory(HipSim, "fixed", abi.F32)[0](64)
    with pytest.raises(Os2rError, match="rounds to zero"):          # positive as a double, zero in the handle's dtype
        f32.linearize(torch.zeros(64, 2), (1e-60, 1e-3, 1e-3))
    torch.cuda.synchronize()
    assert not bool((out != 0).any())
    after = _flat(sim.checkpoint())
    for k, v in _flat(before).items():
        assert torch.equal(after[k], v), k
    sim.close(); f32.close()


# ---------------------------------------------------------------------------------------
# (f) the example runs to its end
# ---------------------------------------------------------------------------------------
def test_lqr_example_runs(torch_mod):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "lqr_balancing.py"), "--envs", "256", "--steps", "60",
                          "--riccati-iters", "200"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PD only" in out.stdout and "LQR" in out.stdout, out.stdout[-2000:]
