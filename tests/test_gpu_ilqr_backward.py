"""os2rc_ilqr_backward (include/os2r_control.h) on the MI355X: the backward pass of iLQR in one launch.  The yardstick is a plain
numpy restatement of the header's steps 1-10 (`restate` below), written in the header's order: every product rounded on its
own, every sum of products ((x0 y0 + x1 y1) + x2 y2) + ..., in the layout's dtype.  The kernel must reproduce it bit for bit
(the sign of a zero aside where a test says so: it is not part of the contract)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import lying_states, make_config
from gym_os2r_amd import abi
from test_gpu_lqr_gains import R_COST, _bits, _dot, synthetic
from test_gpu_lqr_gains import restate as restate_lqr

pytestmark = pytest.mark.gpu

OUTPUTS = ("gains", "ff", "P", "p", "flags", "dv", "weights")


# ---------------------------------------------------------------------------------------
# the restatement (needs no device; tests/test_ilqr_backward_host.py checks it against the textbook recursion)
# ---------------------------------------------------------------------------------------
def restate(A, B, Q, R, K, dtype, mu=0.0, lx=None, lu=None, P_final=None, p_final=None, actions=None, obs=None, cols=None,
            alphas=None):
    """Kernel layouts: A [n, n, L], B [n, 2, L], lx [n, L], lu [2, L] (L = K M), Q [n, n], R [2, 2], P_final [n, n, M],
    p_final [n, M], actions [L, 2], obs [L, D] -> dict of gains [K, 2, n, M], ff [K, 2, M], P [n, n, M], p [n, M],
    flags [K, M] uint8, dv [K, 2, M], weights [K, 2, D+1, nalpha M] or None."""
    n, L = A.shape[0], A.shape[2]
    M = L // K
    A, B = A.astype(dtype), B.astype(dtype)
    Q, R = np.asarray(Q, np.float64).astype(dtype), np.asarray(R, np.float64).astype(dtype)     # rounded once
    mu = np.float64(mu).astype(dtype)
    reg = mu != 0
    zero = np.zeros(M, dtype)
    lx = np.zeros((n, L), dtype) if lx is None else lx.astype(dtype)
    lu = np.zeros((2, L), dtype) if lu is None else lu.astype(dtype)
    P = [[None] * n for _ in range(n)]
    for i in range(n):
        for j in range(i, n):      # only the upper triangle of P_final is read
            P[i][j] = P[j][i] = (np.full(M, Q[i, j], dtype) if P_final is None else P_final[i, j].astype(dtype))
    p = [zero if p_final is None else p_final[j].astype(dtype) for j in range(n)]
    gains, ff, dv = np.zeros((K, 2, n, M), dtype), np.zeros((K, 2, M), dtype), np.zeros((K, 2, M), dtype)
    flags = np.zeros((K, M), np.uint8)
    weights = None
    if cols is not None:
        D = len(cols)
        al = np.asarray(alphas, np.float64).astype(dtype)
        weights = np.zeros((K, 2, D + 1, len(al) * M), dtype)
    half, two = dtype(0.5), dtype(2)
    with np.errstate(all="ignore"):
        for k in range(K - 1, -1, -1):
            s = slice(k * M, (k + 1) * M)
            a = [[A[i, j, s] for j in range(n)] for i in range(n)]
            b = [[B[i, c, s] for c in range(2)] for i in range(n)]
            # 1.
            PB = [[_dot([P[i][l] for l in range(n)], [b[l][c] for l in range(n)]) for c in range(2)] for i in range(n)]
            S00 = R[0, 0] + _dot([b[l][0] for l in range(n)], [PB[l][0] for l in range(n)])
            S01 = R[0, 1] + _dot([b[l][0] for l in range(n)], [PB[l][1] for l in range(n)])
            S11 = R[1, 1] + _dot([b[l][1] for l in range(n)], [PB[l][1] for l in range(n)])
            T00, T11, T01 = (S00 + mu, S11 + mu, S01) if reg else (S00, S11, S01)
            # 2.
            det = T00 * T11 - T01 * T01
            ok = (T00 > 0) & (det > 0) & np.isfinite(det)
            # 3.
            PA = [[_dot([P[i][l] for l in range(n)], [a[l][j] for l in range(n)]) for j in range(n)] for i in range(n)]
            G = [[_dot([b[l][c] for l in range(n)], [PA[l][j] for l in range(n)]) for j in range(n)] for c in range(2)]
            # 4.
            Kk = [[np.where(ok, (T11 * G[0][j] - T01 * G[1][j]) / det, zero) for j in range(n)],
                  [np.where(ok, (T00 * G[1][j] - T01 * G[0][j]) / det, zero) for j in range(n)]]
            # 5.
            Qx = [lx[j, s] + _dot([a[l][j] for l in range(n)], p) for j in range(n)]
            Qu = [lu[c, s] + _dot([b[l][c] for l in range(n)], p) for c in range(2)]
            # 6.
            k0 = np.where(ok, -((T11 * Qu[0] - T01 * Qu[1]) / det), zero)
            k1 = np.where(ok, -((T00 * Qu[1] - T01 * Qu[0]) / det), zero)
            # 7.
            Pn = [[None] * n for _ in range(n)]
            for i in range(n):
                for j in range(i, n):
                    v = (Q[i, j] + _dot([a[l][i] for l in range(n)], [PA[l][j] for l in range(n)])) - \
                        (G[0][i] * Kk[0][j] + G[1][i] * Kk[1][j])
                    if reg:
                        v = v - mu * (Kk[0][i] * Kk[0][j] + Kk[1][i] * Kk[1][j])
                    Pn[i][j] = Pn[j][i] = v
            # 8.
            pn = []
            for j in range(n):
                v = Qx[j] + (G[0][j] * k0 + G[1][j] * k1)
                if reg:
                    v = v + mu * (Kk[0][j] * k0 + Kk[1][j] * k1)
                pn.append(v)
            P, p = Pn, pn
            # 9.
            dv[k, 0] = k0 * Qu[0] + k1 * Qu[1]
            dv[k, 1] = half * (((S00 * k0) * k0 + (S11 * k1) * k1) + two * ((S01 * k0) * k1))
            for c in range(2):
                for j in range(n):
                    gains[k, c, j] = Kk[c][j]
            ff[k, 0], ff[k, 1] = k0, k1
            flags[k] = (~ok).astype(np.uint8)
            # 10.
            if weights is not None:
                o0 = obs[s].astype(dtype)
                a0 = np.clip(actions[s].astype(dtype), dtype(-1), dtype(1))
                raw = [d for d in range(D) if cols[d] >= 0]
                for j, kj in enumerate((k0, k1)):
                    w = {d: -Kk[j][cols[d]] for d in raw}
                    acc = _dot([w[d] for d in raw], [o0[:, d] for d in raw]) if raw else zero
                    for i in range(len(al)):
                        for d in raw:
                            weights[k, j, d, i * M:(i + 1) * M] = w[d]
                        weights[k, j, D, i * M:(i + 1) * M] = (a0[:, j] + al[i] * kj) - acc
    return dict(gains=gains, ff=ff, P=np.stack([np.stack(row) for row in P]), p=np.stack(p), flags=flags, dv=dv, weights=weights)


def gradients(n, L, M):
    """The gradients of the issue: with default_rng(7), lx = N(0,1) [n, L], then lu = 0.3 N(0,1) [2, L], then p_final = N(0,1)
    [n, M] (kernel layouts, float64)."""
    rng = np.random.default_rng(7)
    lx = rng.standard_normal((n, L))
    lu = 0.3 * rng.standard_normal((2, L))
    return lx, lu, rng.standard_normal((n, M))


def _same(got, want, what, zero_sign_free=False):
    """Bit for bit (a NaN on either side fails: the inputs are chosen finite); zero_sign_free: a zero equals a zero."""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else got
    got = np.ascontiguousarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.isfinite(want).all(), what
    bad = _bits(got) != _bits(want)
    if zero_sign_free:
        bad &= ~((got == 0) & (want == 0))
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


# ---------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


_SIMS = {}


@pytest.fixture(scope="module")
def sims(torch_mod):
    """Handles by (mode, dtype, normalized): a call takes from its handle the dtype, nq, the device and the observation layout
    only: 8 environments do."""
    from gym_os2r_amd.sim import HipSim

    def get(mode="free_hip", dtype=abi.F64, normalized=False, binding=None):
        key = (mode, dtype, normalized, binding)
        if key not in _SIMS:
            reward = "StraightV1" if mode == "simple" else "BalancingV1"
            cfg = make_config(mode, reward, normalized, num_envs=8, contact=True, seed=5, auto_reset=False, dtype=dtype)[0]
            _SIMS[key] = HipSim(cfg, binding=binding)
        return _SIMS[key]
    yield get
    for s in _SIMS.values():
        s.close()
    _SIMS.clear()


def _np_dtype(sim):
    import torch
    return np.float64 if sim.dtype == torch.float64 else np.float32


def _dev(torch, sim, x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(sim.device)


def _run(torch, sim, A, B, Q, R, K, **kw):
    """HipSim.ilqr_backward on kernel-layout numpy inputs, handed over in the public layouts (A and B as the permuted views
    linearize() returns) -> dict of the outputs, back in the kernel's layouts (views, no copy), None where not asked for."""
    dt = _np_dtype(sim)
    a = _dev(torch, sim, A.astype(dt)).permute(2, 0, 1)
    b = _dev(torch, sim, B.astype(dt)).permute(2, 0, 1)
    perm = dict(lx=(1, 0), lu=(1, 0), P_final=(2, 0, 1), p_final=(1, 0), actions=(0, 1), obs=(0, 1))
    for name, pm in perm.items():
        if kw.get(name) is not None:
            kw[name] = _dev(torch, sim, kw[name].astype(dt)).permute(*pm)
    out = sim.ilqr_backward(a, b, Q, R, knots=K, **kw)
    torch.cuda.synchronize()
    back = dict(gains=(0, 2, 3, 1), ff=(0, 2, 1), P=(1, 2, 0), p=(1, 0), flags=(0, 1), dv=(0, 2, 1), weights=(1, 2, 3, 0))
    res = {}
    for name, t in zip(OUTPUTS, out):
        res[name] = None if t is None else t.permute(*back[name])
        assert t is None or res[name].is_contiguous(), name           # the public shapes are permuted views of the kernel's layouts
    return res


ALL = dict(want_gains=True, want_ff=True, want_P=True, want_p=True, want_flags=True, want_dv=True, want_weights=True)


def _compare_all(torch, sim, A, B, Q, K, mu, what, alphas=(1.0, 0.5, 0.0), with_inputs=True, raw_slots=2, zero_sign_free=False):
    """Every output of one call against the restatement; -> the restatement's outputs."""
    from gym_os2r_amd.control import slot_columns
    dt = _np_dtype(sim)
    n, L = A.shape[0], A.shape[2]
    M = L // K
    assert n == 2 * sim.nq
    cols = slot_columns(sim.cfg.task, sim.nq)
    assert sum(c >= 0 for c in cols) >= raw_slots, cols
    rng = np.random.default_rng(11)
    actions = rng.uniform(-1.3, 1.3, (L, 2))        # some outside [-1, 1]: clamped as os2r_linearize clamps them
    obs = rng.uniform(-2.0, 2.0, (L, sim.D))
    kw = {}
    if with_inputs:
        lx, lu, pv = gradients(n, L, M)
        pm = Q[:, :, None] * (1.0 + 0.01 * np.arange(M))      # a value Hessian of its own per trajectory
        kw = dict(lx=lx, lu=lu, P_final=pm, p_final=pv)
    want = restate(A, B, Q, R_COST, K, dt, mu=mu, actions=actions, obs=obs, cols=cols, alphas=alphas, **kw)
    assert not want["flags"].any(), what                  # the restatement itself: nothing refused, everything finite
    assert all(np.isfinite(want[o]).all() for o in OUTPUTS), what
    if with_inputs:                                       # only the upper triangle of P_final is read
        kw["P_final"] = np.where(np.tril(np.ones((n, n), bool), -1)[:, :, None], 99.0, kw["P_final"])
    got = _run(torch, sim, A, B, Q, R_COST, K, mu=mu, actions=actions, obs=obs, alphas=alphas, **kw, **ALL)
    assert tuple(got["weights"].shape) == (K, 2, sim.D + 1, len(alphas) * M)
    for o in OUTPUTS:
        _same(got[o], want[o], f"{what}: {o}", zero_sign_free)
    return want


# ---------------------------------------------------------------------------------------
# 1. + 2. bit-exact against the restatement
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_main_case_equals_the_restatement_bit_for_bit(sims, torch_mod, dtype):
    """free_hip (nq 5), K = 3, M = 70: three workgroups of 32 trajectories, the last one partial; mu = 0.5, every input given,
    every output asked for.  Then every nullable input NULL: ff, p and dv are zeros there, of either sign."""
    sim = sims("free_hip", dtype)
    K, M = 3, 70
    A, B, Q = synthetic(10, K * M)
    want = _compare_all(torch_mod, sim, A, B, Q, K, 0.5, f"main {dtype}")
    assert all(np.abs(want[o]).max() > 0.01 for o in ("ff", "p", "dv"))
    null = _compare_all(torch_mod, sim, A, B, Q, K, 0.5, f"main {dtype}, NULL inputs", with_inputs=False, zero_sign_free=True)
    assert not null["ff"].any() and not null["p"].any() and not null["dv"].any()


@pytest.mark.parametrize("mode,dtype,K,M,mu,normalized", [("simple", abi.F64, 1, 1, 0.0, False), ("simple", abi.F32, 1, 1, 0.5, False),
                                                          ("free_hip", abi.F64, 1, 65, 0.5, False), ("free_hip", abi.F32, 1, 65, 0.0, False),
                                                          ("fixed", abi.F64, 2, 33, 0.0, False), ("fixed", abi.F32, 2, 33, 0.5, False),
                                                          ("fixed_hip_torque", abi.F64, 2, 33, 0.5, False),
                                                          ("fixed_hip_torque", abi.F32, 2, 33, 0.0, False),
                                                          ("free_hip", abi.F64, 2, 33, 0.5, True)])
def test_edges_equal_the_restatement_bit_for_bit(sims, torch_mod, mode, dtype, K, M, mu, normalized):
    """The smallest robot with a single trajectory (one lane of a workgroup is live); nq 5 with M = 65 (two full workgroups and
    a tail of one); the kernels of nq 3 and nq 4, a layout with two torque slots and an unobserved state column; and the
    normalised task, none of whose slots is raw: every weight 0, the bias a0 + alpha k."""
    sim = sims(mode, dtype, normalized)
    A, B, Q = synthetic(2 * sim.nq, K * M)
    alphas = (1.0, 0.5, 0.0)
    want = _compare_all(torch_mod, sim, A, B, Q, K, mu, f"{mode} {dtype} {normalized}", alphas=alphas, raw_slots=0 if normalized else 2)
    if normalized:
        W, dt = want["weights"], _np_dtype(sim)
        assert not W[:, :, :sim.D].any()
        a0 = np.clip(np.random.default_rng(11).uniform(-1.3, 1.3, (K * M, 2)), -1, 1).astype(dt).reshape(K, M, 2)
        for i, al in enumerate(alphas):
            assert np.array_equal(W[:, :, sim.D, i * M:(i + 1) * M], a0.transpose(0, 2, 1) + dt(al) * want["ff"])


# ---------------------------------------------------------------------------------------
# 3. without its affine terms it is os2r_lqr_gains
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_without_affine_terms_it_is_lqr_gains_on_the_device(sims, torch_mod, dtype):
    torch = torch_mod
    sim = sims("free_hip", dtype)
    K, M, dt = 3, 70, _np_dtype(sim)
    A, B, Q = synthetic(10, K * M)
    rng = np.random.default_rng(11)
    a, b = _dev(torch, sim, A.astype(dt)).permute(2, 0, 1), _dev(torch, sim, B.astype(dt)).permute(2, 0, 1)
    act, obs = _dev(torch, sim, rng.uniform(-1.3, 1.3, (K * M, 2)).astype(dt)), _dev(torch, sim, rng.uniform(-2, 2, (K * M, sim.D)).astype(dt))
    g0, P0, f0, W0 = sim.lqr_gains(a, b, Q, R_COST, knots=K, sweeps=1, actions=act, obs=obs, want_P=True, want_weights=True)
    g1, ff, P1, p1, f1, dv, W1 = sim.ilqr_backward(a, b, Q, R_COST, knots=K, mu=0.0, actions=act, obs=obs, alphas=(0.0,), **ALL)
    torch.cuda.synchronize()
    assert torch.equal(g1, g0) and torch.equal(P1, P0) and torch.equal(f1, f0) and torch.equal(W1, W0)
    assert not bool(ff.any()) and not bool(p1.any()) and not bool(dv.any()) and bool((g0 != 0).any())


# ---------------------------------------------------------------------------------------
# 4. composition
# ---------------------------------------------------------------------------------------
def test_splits_compose_bit_for_bit(sims, torch_mod):
    torch = torch_mod
    sim = sims("free_hip", abi.F64)
    K, M, n, K1 = 4, 33, 10, 1
    A, B, Q = synthetic(n, K * M)
    lx, lu, pv = gradients(n, K * M, M)
    kw = dict(mu=0.5, want_P=True, want_p=True)
    one = _run(torch, sim, A, B, Q, R_COST, K, lx=lx, lu=lu, p_final=pv, **kw)
    cut = K1 * M
    last = _run(torch, sim, A[:, :, cut:], B[:, :, cut:], Q, R_COST, K - K1, lx=lx[:, cut:], lu=lu[:, cut:], p_final=pv, **kw)
    first = _run(torch, sim, A[:, :, :cut], B[:, :, :cut], Q, R_COST, K1, lx=lx[:, :cut], lu=lu[:, :cut],
                 P_final=last["P"].cpu().numpy(), p_final=last["p"].cpu().numpy(), **kw)
    for o in ("gains", "ff", "flags", "dv"):
        assert torch.equal(torch.cat([first[o], last[o]]), one[o]), o
    assert torch.equal(first["P"], one["P"]) and torch.equal(first["p"], one["p"])
    assert bool(torch.isfinite(one["P"]).all()) and not bool(one["flags"].any()) and not torch.equal(last["p"], one["p"])


# ---------------------------------------------------------------------------------------
# 5. a refused knot
# ---------------------------------------------------------------------------------------
def test_refused_knot_is_flagged_and_leaves_its_neighbours_alone(sims, torch_mod):
    torch = torch_mod
    sim = sims("free_hip", abi.F64)
    K, M, n, bad = 1, 40, 10, 7
    A, B, Q = synthetic(n, K * M)
    lx, lu, pv = gradients(n, K * M, M)
    # R = 0 for the whole call; B = 0 in trajectory `bad` only: there S = 0, everywhere else S = B'PB > 0
    R0 = np.zeros((2, 2))
    B[:, :, bad] = 0.0
    kw = dict(lx=lx, lu=lu, p_final=pv, want_P=True, want_p=True)
    want = restate(A, B, Q, R0, K, np.float64, mu=0.0, lx=lx, lu=lu, p_final=pv)
    assert want["flags"][0, bad] == 1 and want["flags"].sum() == 1
    got = _run(torch, sim, A, B, Q, R0, K, mu=0.0, **kw)
    for o in OUTPUTS[:-1]:
        _same(got[o], want[o], o, zero_sign_free=True)
    assert int(got["flags"][0, bad]) == 1 and int(got["flags"].sum()) == 1
    assert not bool((got["gains"][0, :, :, bad] != 0).any()) and not bool((got["ff"][0, :, bad] != 0).any())      # exactly zero
    assert not want["gains"][0, :, :, bad].any() and not want["ff"][0, :, bad].any()
    # p' = lx + A'p there, in the header's order
    for j in range(n):
        v = lx[j, bad] + _dot([A[l, j, bad] for l in range(n)], [pv[l, bad] for l in range(n)])
        assert float(got["p"][j, bad]) == v == want["p"][j, bad], j
    # the neighbours in its workgroup equal the run without it
    keep = [m for m in range(M) if m != bad]
    kept = _run(torch, sim, A[:, :, keep], B[:, :, keep], Q, R0, K, mu=0.0, lx=lx[:, keep], lu=lu[:, keep], p_final=pv[:, keep],
                want_P=True, want_p=True)
    for o in OUTPUTS[:-1]:
        assert torch.equal(got[o][..., keep], kept[o]), o
    assert not bool(kept["flags"].any())
    # the same inputs with mu = 0.5: T = mu I in that trajectory, nothing is refused, K = 0 and k = -lu / mu there
    want = restate(A, B, Q, R0, K, np.float64, mu=0.5, lx=lx, lu=lu, p_final=pv)
    got = _run(torch, sim, A, B, Q, R0, K, mu=0.5, **kw)
    for o in OUTPUTS[:-1]:
        _same(got[o], want[o], o + " (mu)", zero_sign_free=True)
    assert not want["flags"].any() and not bool(got["flags"].any())
    assert not bool((got["gains"][0, :, :, bad] != 0).any())
    assert np.allclose(got["ff"][0, :, bad].cpu().numpy(), -lu[:, bad] / 0.5, rtol=1e-14, atol=0)
    assert np.allclose(want["ff"][0, :, bad], -lu[:, bad] / 0.5, rtol=1e-14, atol=0)


# ---------------------------------------------------------------------------------------
# 6. no write outside the outputs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 65])
def test_no_write_outside_the_outputs(sims, torch_mod, M):
    torch = torch_mod
    from gym_os2r_amd import control
    sim = sims("free_hip", abi.F64)
    K, n, D, alphas = 2, 10, sim.D, (1.0, 0.25)
    L, nal = K * M, len(alphas)
    A, B, Q = synthetic(n, L)
    lxn, lun, pvn = gradients(n, L, M)
    a, b, lx, lu, pv = (_dev(torch, sim, x) for x in (A, B, lxn, lun, pvn))
    rng = np.random.default_rng(2)
    act, obs = _dev(torch, sim, rng.uniform(-1, 1, (L, 2))), _dev(torch, sim, rng.uniform(-1, 1, (L, D)))
    pad, mark = 64, -12345.5
    sizes = {"gain": K * 2 * n * M, "ff": K * 2 * M, "pmat": n * n * M, "pvec": n * M, "dv": K * 2 * M, "weights": K * 2 * (D + 1) * nal * M}
    bufs = {k: torch.full((pad + v + pad,), mark, dtype=sim.dtype, device=sim.device) for k, v in sizes.items()}
    flag = torch.full((pad + K * M + pad,), 77, dtype=torch.uint8, device=sim.device)
    at = lambda t: ctypes.c_void_p(t.data_ptr() + pad * t.element_size())
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    q = (ctypes.c_double * (n * n))(*Q.reshape(-1))
    r = (ctypes.c_double * 4)(*R_COST.reshape(-1))
    lib = control.load()
    lay = control.layout(abi.F64, sim.nq, sim.device.index or 0, control.slot_columns(sim.cfg.task, sim.nq))
    rc = lib.os2rc_ilqr_backward(ctypes.byref(lay), K, M, p(a), p(b), p(lx), p(lu), q, r, 0.5, None, p(pv), at(bufs["gain"]), at(bufs["ff"]),
                                 at(bufs["pmat"]), at(bufs["pvec"]), at(flag), at(bufs["dv"]), p(act), p(obs),
                                 (ctypes.c_double * nal)(*alphas), nal, at(bufs["weights"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == abi.OK, lib.os2rc_last_error()
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t[:pad] == mark).all()) and bool((t[-pad:] == mark).all()), name
        assert not bool((t[pad:-pad] == mark).any()), name                      # and every element of the extent was written
    assert bool((flag[:pad] == 77).all()) and bool((flag[-pad:] == 77).all()) and not bool((flag[pad:-pad] == 77).any())
    # the raw layouts are the documented ones
    kw = dict(knots=K, lx=lx.permute(1, 0), lu=lu.permute(1, 0), mu=0.5, p_final=pv.permute(1, 0))
    gains, ff, P, pvec, fl, dv, W = sim.ilqr_backward(a.permute(2, 0, 1), b.permute(2, 0, 1), Q, R_COST, actions=act, obs=obs, alphas=alphas,
                                                      **kw, **ALL)
    inner = lambda name: bufs[name][pad:-pad]
    assert torch.equal(inner("gain").view(K, 2, n, M).permute(0, 3, 1, 2), gains) and torch.equal(inner("ff").view(K, 2, M).permute(0, 2, 1), ff)
    assert torch.equal(inner("pmat").view(n, n, M).permute(2, 0, 1), P) and torch.equal(inner("pvec").view(n, M).permute(1, 0), pvec)
    assert torch.equal(inner("dv").view(K, 2, M).permute(0, 2, 1), dv) and torch.equal(flag[pad:-pad].view(K, M), fl)
    assert torch.equal(inner("weights").view(K, 2, D + 1, nal * M).permute(3, 0, 1, 2), W)
    # pmat_out may alias pmat_final and pvec_out pvec_final: in place
    pm, pv2 = inner("pmat").clone().view(n, n, M), inner("pvec").clone().view(n, M)
    kw.update(P_final=pm.permute(2, 0, 1), p_final=pv2.permute(1, 0))
    want = sim.ilqr_backward(a.permute(2, 0, 1), b.permute(2, 0, 1), Q, R_COST, want_P=True, want_p=True, **kw)
    sim.ilqr_backward_into(a, b, Q, R_COST, knots=K, lx=lx, lu=lu, mu=0.5, P_final=pm, p_final=pv2, P_out=pm, p_out=pv2)
    torch.cuda.synchronize()
    assert torch.equal(pm.permute(2, 0, 1), want[2]) and torch.equal(pv2.permute(1, 0), want[3])
    assert not torch.equal(pm, inner("pmat").view(n, n, M))


# ---------------------------------------------------------------------------------------
# 7. real Jacobians, fed through unchanged, into a batch of line-search candidates
# ---------------------------------------------------------------------------------------
def test_linearize_output_through_the_backward_pass_into_a_scheduled_rollout(torch_mod):
    torch = torch_mod
    from gym_os2r_amd.control import slot_columns
    from gym_os2r_amd.sim import HipSim
    K, M, alphas = 4, 16, (1.0, 0.5, 0.0)

    def make(n):
        cfg, _, model = make_config("free_hip", "BalancingV1", False, num_envs=n, contact=True, seed=5, auto_reset=False, dtype=abi.F64)
        return HipSim(cfg), model
    knots, model = make(K * M)
    q, qd = lying_states(model, knots.N, np.random.default_rng(5))
    knots.set_state(q, qd)
    for _ in range(200):
        knots.step(None, want_terminal=False)
    g = torch.Generator().manual_seed(3)
    actions = (torch.rand(knots.N, 2, generator=g, dtype=torch.float64) * 2.4 - 1.2).to(knots.device)
    obs = knots.copy_envs_from(knots, want_obs=True)
    _, _, A, B = knots.linearize(actions, want_next=False)
    n = 2 * knots.nq
    cols = slot_columns(knots.cfg.task, knots.nq)
    qdiag = np.array([0.0 if c not in cols else (1.0 if c < knots.nq else 0.01) for c in range(n)])
    Q, R = np.diag(qdiag), 0.1 * np.eye(2)
    lx = (0.01 * torch.randn(knots.N, n, generator=g, dtype=torch.float64)).to(knots.device)
    lu = (0.01 * torch.randn(knots.N, 2, generator=g, dtype=torch.float64)).to(knots.device)
    gains, ff, _, _, fl, dv, table = knots.ilqr_backward(A, B, Q, R, knots=K, lx=lx, lu=lu, mu=0.0, actions=actions, obs=obs, alphas=alphas,
                                                         want_weights=True)
    assert A.permute(1, 2, 0).is_contiguous()                                         # taken as it came: no copy was needed
    _, _, _, table_lqr = knots.lqr_gains(A, B, Q, R, knots=K, actions=actions, obs=obs, want_weights=True)
    torch.cuda.synchronize()
    want = restate(A.permute(1, 2, 0).cpu().numpy(), B.permute(1, 2, 0).cpu().numpy(), Q, R, K, np.float64, mu=0.0,
                   lx=lx.permute(1, 0).cpu().numpy(), lu=lu.permute(1, 0).cpu().numpy(), actions=actions.cpu().numpy(),
                   obs=obs.cpu().numpy(), cols=cols, alphas=alphas)
    _same(table.permute(1, 2, 3, 0), want["weights"], "table")
    _same(gains.permute(0, 2, 3, 1), want["gains"], "gains")
    _same(ff.permute(0, 2, 1), want["ff"], "ff")
    _same(dv.permute(0, 2, 1), want["dv"], "dv")
    _same(fl, want["flags"], "flags")
    assert bool((gains != 0).any()) and bool((ff != 0).any())
    # the 48-lane table as it is into rollout_schedule, against the same rollout on a twin handle given the restatement's table
    assert tuple(table.shape) == (len(alphas) * M, K, 2, knots.D + 1) and table.permute(1, 2, 3, 0).is_contiguous()
    table_ref = torch.as_tensor(want["weights"]).to(knots.device).permute(3, 0, 1, 2)
    index = torch.arange(M, dtype=torch.int32, device=knots.device).repeat(len(alphas))     # knot 0 of trajectory m, once per alpha
    acts = []
    for tab, idx in ((table, index), (table_ref, index), (table_lqr, index[:M])):
        trk, _ = make(int(idx.numel()))
        trk.copy_envs_from(knots, idx)
        _, _, _, (act, _) = trk.rollout_schedule(K, tab, want_actions=True)
        torch.cuda.synchronize()
        acts.append(act)
        trk.close()
    assert all(bool(torch.isfinite(a).all()) for a in acts)
    assert torch.equal(acts[0], acts[1]), int((acts[0] != acts[1]).sum())
    assert torch.equal(acts[0][:, 2 * M:], acts[2])                                       # alpha = 0: the nominal under lqr_gains' table
    assert not torch.equal(acts[0][:, :M], acts[2])                                       # alpha = 1 steps away from it
    assert bool((acts[0].abs() < 1).any())                                                # not every action saturates
    knots.close()


# ---------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------
def test_refusals_name_their_cause(sims, torch_mod):
    torch = torch_mod
    from gym_os2r_amd import control
    sim = sims("fixed", abi.F64)
    lib = control.load()
    n, M = 2 * sim.nq, 4
    buf = torch.zeros(n * n * M * 8, dtype=sim.dtype, device=sim.device)
    d = ctypes.c_void_p(buf.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")
    cols = control.slot_columns(sim.cfg.task, sim.nq)

    def Lay(**kw):
        lay = control.layout(abi.F64, sim.nq, sim.device.index or 0, cols)
        for k, v in kw.items():
            if k == "slot0":
                lay.slot_col[0] = v
            else:
                setattr(lay, k, v)
        return ctypes.byref(lay)

    def Qm(i=None, j=None, v=0.0):
        m = np.eye(n)
        if i is not None:
            m[i, j] = v
        return (ctypes.c_double * (n * n))(*m.reshape(-1))

    def Rm(*v):
        return (ctypes.c_double * 4)(*(v or (0.1, 0.0, 0.0, 0.1)))

    def Al(*v):
        return (ctypes.c_double * len(v))(*v)
    good = dict(lay=Lay(), K=1, M=M, a=d, b=d, lx=None, lu=None, q=Qm(), r=Rm(), mu=0.0, pf=None, vf=None, g=d, ff=None, po=None, vo=None,
                fl=None, dv=None, act=None, obs=None, al=None, nal=0, w=None)
    table = dict(w=d, act=d, obs=d, al=Al(1.0, 0.5), nal=2)

    def call(**kw):
        a = dict(good, **kw)
        return lib.os2rc_ilqr_backward(*[a[k] for k in good], st)
    for kw, msg in [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype"), (dict(lay=Lay(nq=1)), b"nq"), (dict(lay=Lay(nq=6)), b"nq"),
                    (dict(K=0), b"nknots"), (dict(M=0), b"ntraj"), (dict(K=-1), b"nknots"),
                    (dict(a=None), b"null a_dev"), (dict(b=None), b"null b_dev"), (dict(q=None), b"null q_host"), (dict(r=None), b"null r_host"),
                    (dict(q=Qm(1, 2, nan)), b"Q must be finite"), (dict(q=Qm(0, 0, -inf)), b"Q must be finite"),
                    (dict(q=Qm(1, 2, 0.5)), b"Q must be exactly symmetric"),
                    (dict(r=Rm(0.1, nan, nan, 0.1)), b"R must be finite"), (dict(r=Rm(0.1, 0.01, 0.02, 0.1)), b"R must be exactly symmetric"),
                    (dict(mu=nan), b"mu must be finite"), (dict(mu=inf), b"mu must be finite"), (dict(mu=-0.5), b"mu must be >= 0"),
                    (dict(g=None), b"all outputs are null"), (dict(g=None, fl=d), b"all outputs are null"),
                    (dict(table, act=None), b"weights need"), (dict(table, obs=None), b"weights need"), (dict(table, al=None), b"weights need"),
                    (dict(table, nal=0), b"nalpha"), (dict(table, al=Al(*[1.0] * 17), nal=17), b"nalpha"),
                    (dict(table, al=Al(1.0, nan)), b"alpha must be finite"),
                    (dict(table, lay=Lay(obs_dim=0)), b"obs_dim"), (dict(table, lay=Lay(obs_dim=13)), b"obs_dim"),
                    (dict(table, lay=Lay(slot0=n)), b"slot_col"), (dict(table, lay=Lay(slot0=-2)), b"slot_col")]:
        rc = call(**kw)
        err = lib.os2rc_last_error()
        assert rc == abi.ERR_INVALID and msg in err and b"os2rc_ilqr_backward" in err, (kw.keys(), msg, rc, err)
    rc = call(lay=Lay(device=1000))
    assert rc == abi.ERR_NO_DEVICE and b"os2rc_ilqr_backward" in lib.os2rc_last_error(), (rc, lib.os2rc_last_error())
    torch.cuda.synchronize()
    assert not bool((buf != 0).any())                               # a refused call wrote nothing
    assert call() == abi.OK and call(**table) == abi.OK             # and the same arguments without the fault are taken
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------
# 9. the example runs to its end
# ---------------------------------------------------------------------------------------
def test_example_runs_and_never_accepts_a_worse_cost(torch_mod):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ilqr_balancing.py"), "--envs", "8", "--steps", "20", "--iters", "3"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    costs = [float(c) for c in re.findall(r"^iter +\d+ +cost +([-+0-9.eE]+)", out.stdout, re.M)]
    assert len(costs) == 4, out.stdout[-2000:]                      # the nominal and three iterations
    assert all(b <= a for a, b in zip(costs, costs[1:])), costs
