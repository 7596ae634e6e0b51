"""libos2r_box.so (include/os2r_box.h): the host side.  The numpy restatement of B1-B5 the GPU tests compare with (`restate_box`,
its QP in `box_qp`) against
  (a) projected gradient in float64, 20 000 iterations, on 3 000 random 2-D problems whose bounds come from random nominals:
      the restatement stands MEASURED_PG off it (float64: 3.4e-15, float32: 4.2e-7, in units of max(1, |k|)); asserted at
      eight times that,
  (b) the general value update of Tassa, Mansard and Todorov on the restatement's K and k with mu = 0.3, in float64 on 500 knots:
      steps 7 and 8 of os2r_control.h stand MEASURED_VALUE = 2.1e-16 off it, relative to the largest entry; asserted at eight
      times that,
  (c) the restatement of os2rt_ilqr_backward_mu, which it equals bit for bit with infinite bounds,
  (d) the coverage of the fixed inputs the GPU test runs (`box_case`): every clamp byte the rule can produce, a refused knot, an
      invalid mu, an infinite bound on one side.
Then the header against the table of gym_os2r_amd/box.py, the exports against the .map, every refusal of the C call through ctypes
without a device, those of the Python layer, what reaches C, and the resources of the eight kernels.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from gym_os2r_amd import abi

sys.path.insert(0, os.path.join(ROOT, "tests"))
from header_check import _agrees, _header, _is_pointer, _prototypes, checks_before_the_device, the_finite_and_symmetric_tests_make_no_hip_call  # noqa: E402
from test_gpu_ilqr_backward import gradients  # noqa: E402
from test_gpu_ilqr_backward import restate as restate_backward  # noqa: E402
from test_gpu_lqr_gains import R_COST, _bits, _dot, synthetic  # noqa: E402

NAMES = ["os2rb_abi_version", "os2rb_last_error", "os2rb_ilqr_backward_box"]
INF = float("inf")
EDGES = ((0, False), (0, True), (1, False), (1, True))       # e = 0..3: (component, at its upper bound)
# every clamp byte B4 can write: the interior, the four edges with the other component free, the four corners
UNPINNED, CORNERS = {1, 5, 2, 10}, {3, 7, 11, 15}
MEASURED_PG = {np.float64: 3.4e-15, np.float32: 4.2e-7}
MEASURED_VALUE = 2.1e-16
OUTPUTS = ("gains", "ff", "P", "p", "flags", "dv", "weights", "clamped")
SHAPE = (5, 70)                                              # K, M of the GPU test: three workgroups, the last with 6 lanes


# ---------------------------------------------------------------------------------------
# the restatement of include/os2r_box.h (needs no device)
# ---------------------------------------------------------------------------------------
def box_qp(dtype, T00, T01, T11, Qu0, Qu1, dlo0, dhi0, dlo1, dhi1, ok):
    """B2-B4 for arrays of knots, in `dtype`: -> dict of k0, k1 (the step), clamp (the byte), solved (flag 0), edge (the knot took an
    edge candidate), comp (the winner's clamped component) and pinned."""
    half, two, zero = dtype(0.5), dtype(2), np.zeros_like(T00)
    with np.errstate(all="ignore"):
        det = T00 * T11 - T01 * T01
        f0 = -((T11 * Qu0 - T01 * Qu1) / det)
        f1 = -((T00 * Qu1 - T01 * Qu0) / det)
        inside = (dlo0 <= f0) & (f0 <= dhi0) & (dlo1 <= f1) & (f1 <= dhi1)                  # false on a NaN
        have = np.zeros(T00.shape, bool)
        best, w0, w1 = zero.copy(), zero.copy(), zero.copy()
        byte, comp, pin = np.zeros(T00.shape, np.uint8), np.zeros(T00.shape, np.int8), np.zeros(T00.shape, bool)
        for c, upper in EDGES:
            b = ((dlo0, dhi0), (dlo1, dhi1))[c][upper] + zero
            Quj, Tjj, dloj, dhij = ((Qu1, T11, dlo1, dhi1), (Qu0, T00, dlo0, dhi0))[c]
            raw = -((Quj + T01 * b) / Tjj)
            below, above = raw < dloj, raw > dhij
            u = np.where(above, dhij, np.where(below, dloj, raw))                           # a NaN stays a NaN
            c0, c1 = (b, u) if c == 0 else (u, b)
            v = half * (((T00 * c0) * c0 + (T11 * c1) * c1) + two * ((T01 * c0) * c1)) + (Qu0 * c0 + Qu1 * c1)
            take = np.isfinite(b) & np.isfinite(v)
            take &= ~have | (v < best)
            bits = (1 << c) | ((below | above).astype(np.uint8) << (1 - c)) | ((4 << c) if upper else 0) | (above.astype(np.uint8) << (3 - c))
            best, w0, w1 = np.where(take, v, best), np.where(take, c0, w0), np.where(take, c1, w1)
            byte, comp, pin = np.where(take, bits, byte).astype(np.uint8), np.where(take, c, comp), np.where(take, below | above, pin)
            have |= take
        edge = ok & ~inside & have
        solved = ok & (inside | have)
        k0 = np.where(solved, np.where(inside, f0, w0), zero)
        k1 = np.where(solved, np.where(inside, f1, w1), zero)
    return dict(k0=k0, k1=k1, clamp=np.where(edge, byte, 0).astype(np.uint8), solved=solved, edge=edge, comp=comp, pinned=pin, inside=ok & inside)


def restate_box(A, B, Q, R, K, dtype, mu=0.0, lo=(-1.0, -1.0), hi=(1.0, 1.0), lx=None, lu=None, P_final=None, p_final=None,
                actions=None, obs=None, cols=None, alphas=None):
    """test_gpu_ilqr_backward.restate with B1-B5 in place of steps 4 and 6: the same kernel layouts, mu a number or [M] (an entry
    that is negative or not finite runs as 0 with every knot refused), lo and hi pairs, actions [L, 2] required
    -> its dict with clamped [K, M] uint8 added."""
    n, L = A.shape[0], A.shape[2]
    M = L // K
    A, B = A.astype(dtype), B.astype(dtype)
    Q, R = np.asarray(Q, np.float64).astype(dtype), np.asarray(R, np.float64).astype(dtype)     # rounded once
    lo, hi = np.asarray(lo, np.float64).astype(dtype), np.asarray(hi, np.float64).astype(dtype)
    mu = np.broadcast_to(np.asarray(mu, np.float64), (M,)).astype(dtype)
    with np.errstate(invalid="ignore"):
        mu_bad = ~np.isfinite(mu) | ((mu < 0) & (mu != 0))
    mu = np.where(mu_bad, dtype(0), mu)
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
    flags, clamped = np.zeros((K, M), np.uint8), np.zeros((K, M), np.uint8)
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
            T00, T11, T01 = np.where(reg, S00 + mu, S00), np.where(reg, S11 + mu, S11), S01
            # 2.
            det = T00 * T11 - T01 * T01
            ok = (T00 > 0) & (det > 0) & np.isfinite(det) & ~mu_bad
            # 3.
            PA = [[_dot([P[i][l] for l in range(n)], [a[l][j] for l in range(n)]) for j in range(n)] for i in range(n)]
            G = [[_dot([b[l][c] for l in range(n)], [PA[l][j] for l in range(n)]) for j in range(n)] for c in range(2)]
            # 5.
            Qx = [lx[j, s] + _dot([a[l][j] for l in range(n)], p) for j in range(n)]
            Qu = [lu[c, s] + _dot([b[l][c] for l in range(n)], p) for c in range(2)]
            # B1
            a0 = np.clip(actions[s].astype(dtype), dtype(-1), dtype(1))
            dlo0, dhi0, dlo1, dhi1 = lo[0] - a0[:, 0], hi[0] - a0[:, 0], lo[1] - a0[:, 1], hi[1] - a0[:, 1]
            # B2, B3
            qp = box_qp(dtype, T00, T01, T11, Qu[0], Qu[1], dlo0, dhi0, dlo1, dhi1, ok)
            k0, k1, solved, edge = qp["k0"], qp["k1"], qp["solved"], qp["edge"]
            # B4: the interior's K (step 4), or the winner's
            Kk = [[None] * n, [None] * n]
            for j in range(n):
                int0, int1 = (T11 * G[0][j] - T01 * G[1][j]) / det, (T00 * G[1][j] - T01 * G[0][j]) / det
                free0 = np.where((qp["comp"] == 1) & ~qp["pinned"], G[0][j] / T00, zero)
                free1 = np.where((qp["comp"] == 0) & ~qp["pinned"], G[1][j] / T11, zero)
                Kk[0][j] = np.where(solved, np.where(edge, free0, int0), zero)
                Kk[1][j] = np.where(solved, np.where(edge, free1, int1), zero)
            # 7.
            Pn = [[None] * n for _ in range(n)]
            for i in range(n):
                for j in range(i, n):
                    v = (Q[i, j] + _dot([a[l][i] for l in range(n)], [PA[l][j] for l in range(n)])) - \
                        (G[0][i] * Kk[0][j] + G[1][i] * Kk[1][j])
                    Pn[i][j] = Pn[j][i] = np.where(reg, v - mu * (Kk[0][i] * Kk[0][j] + Kk[1][i] * Kk[1][j]), v)
            # 8.
            pn = []
            for j in range(n):
                v = Qx[j] + (G[0][j] * k0 + G[1][j] * k1)
                pn.append(np.where(reg, v + mu * (Kk[0][j] * k0 + Kk[1][j] * k1), v))
            P, p = Pn, pn
            # 9.
            dv[k, 0] = k0 * Qu[0] + k1 * Qu[1]
            dv[k, 1] = half * (((S00 * k0) * k0 + (S11 * k1) * k1) + two * ((S01 * k0) * k1))
            for c in range(2):
                for j in range(n):
                    gains[k, c, j] = Kk[c][j]
            ff[k, 0], ff[k, 1] = k0, k1
            flags[k], clamped[k] = (~solved).astype(np.uint8), qp["clamp"]
            # 10.
            if weights is not None:
                o0 = obs[s].astype(dtype)
                raw = [d for d in range(D) if cols[d] >= 0]
                for j, kj in enumerate((k0, k1)):
                    w = {d: -Kk[j][cols[d]] for d in raw}
                    acc = _dot([w[d] for d in raw], [o0[:, d] for d in raw]) if raw else zero
                    for i in range(len(al)):
                        for d in raw:
                            weights[k, j, d, i * M:(i + 1) * M] = w[d]
                        weights[k, j, D, i * M:(i + 1) * M] = (a0[:, j] + al[i] * kj) - acc
    return dict(gains=gains, ff=ff, P=np.stack([np.stack(row) for row in P]), p=np.stack(p), flags=flags, dv=dv, weights=weights,
                clamped=clamped)


# the fixed inputs of the GPU test, and what they must reach ------------------------------------
M_REFUSED, M_BAD_MU = 29, 13
MU_VALUES = (0.0, 0.1, 3.0)
ONE_SIDED = dict(lo=(-INF, -0.5), hi=(0.25, INF))
COLS = {2: [0, 2, -1, 1, 3], 5: [0, 1, 5, -1, 2, 7, 3, 4, 9, 6]}     # an observation layout per chain length, one slot without a gain


def box_case(nq, K=SHAPE[0], M=SHAPE[1]):
    """The inputs of the issue's GPU comparison for a chain of nq dofs (kernel layouts, float64; the tests round them): the
    synthetic A, B, Q and gradients of test_gpu_ilqr_backward with lu scaled up until the steps leave the box, nominals in
    [-1.3, 1.3] (some beyond the limit: their box has a side at 0), a value Hessian of its own per trajectory, mu cycling through
    0, 0.1 and 3.  Trajectory M_REFUSED has a negative definite P_final: its 2 x 2 systems are refused; trajectory M_BAD_MU has
    mu = NaN."""
    n = 2 * nq
    A, B, Q = synthetic(n, K * M)
    lx, lu, pv = gradients(n, K * M, M)
    rng = np.random.default_rng(11)
    actions, obs = rng.uniform(-1.3, 1.3, (K * M, 2)), rng.uniform(-2.0, 2.0, (K * M, len(COLS[nq])))
    lu = lu * np.where(np.arange(K * M) % 3 == 0, 1.0, 12.0)
    P_final = Q[:, :, None] * (1.0 + 0.01 * np.arange(M))
    mu = np.array(MU_VALUES)[np.arange(M) % 3]
    if M > M_REFUSED:
        P_final[:, :, M_REFUSED] = -50.0 * np.eye(n)
    if M > M_BAD_MU:
        mu[M_BAD_MU] = np.nan
    return dict(A=A, B=B, Q=Q, K=K, mu=mu, cols=COLS[nq], alphas=(1.0, 0.5),
                kw=dict(lx=lx, lu=lu, P_final=P_final, p_final=pv, actions=actions, obs=obs))


def restate_case(c, dtype, **over):
    kw = dict(mu=c["mu"], cols=c["cols"], alphas=c["alphas"])
    kw.update(over)
    return restate_box(c["A"], c["B"], c["Q"], R_COST, c["K"], dtype, **kw, **c["kw"])


_WANT = {}


def wanted(nq, dtype, which="box"):
    """The restatement of box_case(nq) in `dtype`, computed once per session and shared (the GPU test takes it from here):
    "box" under (-1, 1), "one_sided" under ONE_SIDED, "scalar" two knots of the first 40 trajectories under the scalar mu 0.5."""
    key = (nq, dtype, which)
    if key not in _WANT:
        if which == "scalar":
            _WANT[key] = restate_case(box_case(nq, 2, 40), dtype, mu=0.5)
        else:
            _WANT[key] = restate_case(box_case(nq), dtype, **(ONE_SIDED if which == "one_sided" else {}))
        for v in _WANT[key].values():
            v.setflags(write=False)
    return _WANT[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nq", [2, 5])
def test_the_fixed_inputs_reach_every_clamp_byte_a_refused_knot_and_an_invalid_mu(nq, dtype):
    K, M = SHAPE
    want = wanted(nq, dtype)
    seen = set(np.unique(want["clamped"]).tolist())
    assert seen == {0} | UNPINNED | CORNERS, sorted(seen)
    flags, cl = want["flags"], want["clamped"]
    # the refused trajectory and the one with an invalid mu: every knot flagged, nothing clamped, K = 0, k = 0, all of it finite
    for m in (M_REFUSED, M_BAD_MU):
        assert flags[:, m].all() and not cl[:, m].any() and not want["gains"][..., m].any() and not want["ff"][..., m].any()
    others = np.ones(M, bool)
    others[[M_REFUSED, M_BAD_MU]] = False
    assert not flags[:, others].any()
    assert all(np.isfinite(want[o]).all() for o in OUTPUTS)
    # about a third of the knots and more are clamped, and every mu has clamped and free knots
    share = (cl != 0).mean()
    assert 0.3 < share < 0.9, share
    for v in range(3):
        ms = others & (np.arange(M) % 3 == v)
        assert (cl[:, ms] != 0).any() and (cl[:, ms] == 0).any(), v
    # a clamped component: its gain row is zero and the applied step sits on the bound; a free one of an edge knot has a gain row
    dt = dtype
    a0 = np.clip(box_case(nq)["kw"]["actions"].astype(dt), dt(-1), dt(1)).reshape(K, M, 2)
    for c in range(2):
        held = (cl >> c & 1) != 0
        assert not want["gains"][:, c][np.broadcast_to(held[:, None], want["gains"][:, c].shape)].any()
        bound = np.where((cl >> (2 + c) & 1) != 0, dt(1), dt(-1)) - a0[:, :, c]
        assert np.array_equal(want["ff"][:, c][held], bound[held])
        free = (cl != 0) & ~held
        assert free.any() and (np.abs(want["gains"][:, c]).max(1)[free] > 0).all()
    # inside the box everywhere
    step = a0 + np.moveaxis(want["ff"], 1, 2)
    assert (step >= -1).all() and (step <= 1).all()
    # one side infinite: the bytes that need the missing sides never occur, the others do
    one = wanted(nq, dtype, "one_sided")["clamped"]
    got = set(np.unique(one).tolist())
    assert got <= {0, 5, 2, 7} and {0, 5, 2} <= got, sorted(got)
    # the scalar case clamps too
    assert (wanted(nq, dtype, "scalar")["clamped"] != 0).any()


# ---------------------------------------------------------------------------------------
# (a) an independent solver
# ---------------------------------------------------------------------------------------
def _random_qps(count, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((count, 2, 2))
    T = g @ np.swapaxes(g, 1, 2) + 0.2 * np.eye(2)
    Qu = 3.0 * rng.standard_normal((count, 2))
    a0 = np.clip(rng.uniform(-1.3, 1.3, (count, 2)), -1, 1)
    return T[:, 0, 0].copy(), T[:, 0, 1].copy(), T[:, 1, 1].copy(), Qu[:, 0].copy(), Qu[:, 1].copy(), -1.0 - a0, 1.0 - a0


def _projected_gradient(T00, T01, T11, Qu0, Qu1, dlo, dhi, iters=20000):
    step = 1.0 / (T00 + T11)                               # the trace bounds the largest eigenvalue
    x0, x1 = np.zeros_like(T00), np.zeros_like(T00)
    for _ in range(iters):
        g0, g1 = T00 * x0 + T01 * x1 + Qu0, T01 * x0 + T11 * x1 + Qu1
        x0, x1 = np.clip(x0 - step * g0, dlo[:, 0], dhi[:, 0]), np.clip(x1 - step * g1, dlo[:, 1], dhi[:, 1])
    return x0, x1


@pytest.fixture(scope="module")
def qps():
    q = _random_qps(3000, 5)
    return q, _projected_gradient(*q)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_qp_of_the_restatement_equals_projected_gradient(qps, dtype):
    (T00, T01, T11, Qu0, Qu1, dlo, dhi), (x0, x1) = qps
    r = lambda x: x.astype(dtype)
    if dtype is np.float32:        # the problem the float32 restatement solves: its rounded inputs, solved again in float64
        T00, T01, T11, Qu0, Qu1, dlo, dhi = (r(x).astype(np.float64) for x in (T00, T01, T11, Qu0, Qu1, dlo, dhi))
        x0, x1 = _projected_gradient(T00, T01, T11, Qu0, Qu1, dlo, dhi)
    qp = box_qp(dtype, r(T00), r(T01), r(T11), r(Qu0), r(Qu1), r(dlo[:, 0]), r(dhi[:, 0]), r(dlo[:, 1]), r(dhi[:, 1]), np.ones(len(T00), bool))
    assert qp["solved"].all() and qp["k0"].dtype == dtype
    seen = set(np.unique(qp["clamp"]).tolist())
    assert seen == {0} | UNPINNED | CORNERS, sorted(seen)
    err = np.maximum(np.abs(qp["k0"] - x0), np.abs(qp["k1"] - x1)) / np.maximum(1.0, np.maximum(np.abs(x0), np.abs(x1)))
    print(f"box_qp against projected gradient, {dtype.__name__}: {err.max():.3e}")
    assert err.max() <= 8 * MEASURED_PG[dtype], err.max()


# ---------------------------------------------------------------------------------------
# (b) the general value update
# ---------------------------------------------------------------------------------------
def test_steps_7_and_8_are_the_general_value_update_on_the_clamped_gains():
    rng = np.random.default_rng(3)
    count, n, mu = 500, 6, 0.3
    g = rng.standard_normal((count, 2, 2))
    S = g @ np.swapaxes(g, 1, 2) + 0.1 * np.eye(2)
    T = S + mu * np.eye(2)
    h = rng.standard_normal((count, n, n))
    Qxx = h @ np.swapaxes(h, 1, 2)
    G, Qx, Qu = rng.standard_normal((count, 2, n)), rng.standard_normal((count, n)), 3.0 * rng.standard_normal((count, 2))
    a0 = np.clip(rng.uniform(-1.3, 1.3, (count, 2)), -1, 1)
    dlo, dhi = -1.0 - a0, 1.0 - a0
    qp = box_qp(np.float64, T[:, 0, 0], T[:, 0, 1], T[:, 1, 1], Qu[:, 0], Qu[:, 1], dlo[:, 0], dhi[:, 0], dlo[:, 1], dhi[:, 1], np.ones(count, bool))
    assert set(np.unique(qp["clamp"]).tolist()) == {0} | UNPINNED | CORNERS
    k = np.stack([qp["k0"], qp["k1"]], 1)
    Kint = np.linalg.solve(T, G)
    Kg = np.zeros((count, 2, n))
    for i in range(count):
        if not qp["edge"][i]:
            Kg[i] = Kint[i]
        elif not qp["pinned"][i]:
            j = 1 - qp["comp"][i]
            Kg[i, j] = G[i, j] / T[i, j, j]
    Kt = np.swapaxes(Kg, 1, 2)
    Gt = np.swapaxes(G, 1, 2)
    # steps 7 and 8 of os2r_control.h
    P78 = Qxx - Gt @ Kg - mu * (Kt @ Kg)
    p78 = Qx + (Gt @ k[:, :, None])[:, :, 0] + mu * (Kt @ k[:, :, None])[:, :, 0]
    # Tassa et al.: S unregularised
    Vxx = Qxx + Kt @ S @ Kg - Kt @ G - Gt @ Kg
    Vx = Qx + (Gt @ k[:, :, None])[:, :, 0] - (Kt @ Qu[:, :, None])[:, :, 0] - (Kt @ S @ k[:, :, None])[:, :, 0]
    err = max(np.abs(P78 - Vxx).max() / np.abs(Vxx).max(), np.abs(p78 - Vx).max() / np.abs(Vx).max())
    print(f"steps 7 and 8 against the general value update: {err:.3e}")
    assert err <= 8 * MEASURED_VALUE, err


# ---------------------------------------------------------------------------------------
# (c) without bounds it is the restatement of os2rt_ilqr_backward_mu
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nq", [2, 5])
def test_with_infinite_bounds_it_is_the_unconstrained_restatement_bit_for_bit(nq, dtype):
    c = box_case(nq, 3, 12)
    c["mu"] = np.array([0.0, 0.1, 3.0, -1.0])[np.arange(12) % 4]
    got = restate_case(c, dtype, lo=(-INF, -INF), hi=(INF, INF))
    assert not got["clamped"].any()
    lanes = dict(gains=1, ff=1, P=1, p=1, flags=1, dv=1, weights=len(c["alphas"]))
    for v, mu in enumerate((0.0, 0.1, 3.0, -1.0)):
        ms = np.arange(12) % 4 == v
        if mu >= 0:
            want = restate_backward(c["A"], c["B"], c["Q"], R_COST, c["K"], dtype, mu=mu, cols=c["cols"], alphas=c["alphas"], **c["kw"])
        else:           # as tests/test_gpu_ilqr_steer.py restates an invalid entry: B = 0 and R = 0 refuse every knot
            want = restate_backward(c["A"], np.zeros_like(c["B"]), c["Q"], np.zeros((2, 2)), c["K"], dtype, mu=0.0, cols=c["cols"],
                                    alphas=c["alphas"], **c["kw"])
            assert want["flags"].all()
        for o in lanes:
            sel = np.tile(ms, lanes[o])
            x, y = np.ascontiguousarray(got[o][..., sel]), np.ascontiguousarray(want[o][..., sel])
            bad = (_bits(x) != _bits(y)) & ~((x == 0) & (y == 0))
            assert not bad.any(), (mu, o, int(bad.sum()))
    # ... and a scalar mu is the array that holds it everywhere
    one, many = restate_case(c, dtype, mu=0.1), restate_case(c, dtype, mu=np.full(12, 0.1))
    assert all(np.array_equal(_bits(one[o]), _bits(many[o])) for o in OUTPUTS) and one["clamped"].any()


# ---------------------------------------------------------------------------------------
# header, table, exports
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import box, control
    protos = _prototypes("os2r_box.h", "os2rb")
    assert [p[0] for p in protos] == list(box.ENTRY_POINTS) == NAMES
    lib = box.load()
    for name, ret, args in protos:
        argtypes = box.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2rb_last_error" else C.c_int)
    # os2rt_ilqr_backward_mu with the scalar mu in front of mu_dev, the bounds behind it and clamp_dev behind dv_dev
    (_, _, theirs), = [p for p in _prototypes("os2r_steer.h", "os2rt") if p[0] == "os2rt_ilqr_backward_mu"]
    ours = protos[2][2]
    added = ["double mu", "const double* lo_host", "const double* hi_host", "uint8_t* clamp_dev"]
    assert [a for a in ours if a not in added] == theirs
    at = ours.index
    assert at("double mu") + 1 == at("const void* mu_dev") and at("const void* mu_dev") + 1 == at("const double* lo_host") == at("const double* hi_host") - 1
    assert at("void* dv_dev") + 1 == at("uint8_t* clamp_dev") and ours[-1] == "void* stream" and len(ours) == 28
    header = _header("os2r_box.h")
    assert re.search(r"#define OS2R_BOX_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert len(re.findall(r"#include", header)) == 1
    assert lib.os2rb_abi_version() == box.ABI_VERSION == 1
    assert box.Os2rControlLayout is control.Os2rControlLayout and box.layout is control.layout
    assert (box.CLAMPED_0, box.CLAMPED_1, box.UPPER_0, box.UPPER_1) == (1, 2, 4, 8) and box.DEFAULT_BOX == (-1.0, 1.0)
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", box.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "libos2r_box.map")) as f:
        assert re.search(r"global:\s*os2rb_\*;\s*local:\s*\*;", f.read())
    # no other header declares anything of this library
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "os2r_box.h":
            assert "os2rb_" not in _header(name) and "os2r_box" not in _header(name).lower(), name


def test_kernel_resources():
    """Exactly eight kernels ({float, double} x nq 2..5) are in the built library and none uses scratch: private_segment_fixed_size
    0, no VGPR spill and no AGPRs in the code-object metadata (spilled SGPRs ride in VGPR lanes, as in the sibling; both counts
    are printed).  The nominal actions wait in registers: the LDS of every
    kernel is that of ilqr_backward_mu_kernel for the same dtype and chain, not a byte more."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import box, steer
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(box.LIB_PATH)
    meta, parent = kernel_meta.kernel_meta(box.LIB_PATH), kernel_meta.kernel_meta(steer.LIB_PATH)
    assert len(meta) == 8, sorted(meta)
    for real in ("float", "double"):
        for nq in (2, 3, 4, 5):
            (name,) = [k for k in meta if f"ilqr_backward_box_kernel<{real}, {nq}>" in k]
            (theirs,) = [k for k in parent if f"ilqr_backward_mu_kernel<{real}, {nq}>" in k]
            m = meta[name]
            print(f"ilqr_backward_box_kernel<{real}, {nq}>: {m['vgpr_count']} VGPRs, {m['sgpr_spill_count']} SGPRs in lanes "
                  f"(the sibling: {parent[theirs]['vgpr_count']}, {parent[theirs]['sgpr_spill_count']})")
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
            assert m["vgpr_count"] <= 256, (name, m)             # the six waves of the widest workgroup on four SIMDs
            assert 0 < m["group_segment_fixed_size"] <= parent[theirs]["group_segment_fixed_size"], (name, m)


# ---------------------------------------------------------------------------------------
# refusals of the C call
# ---------------------------------------------------------------------------------------
NEW_TEXTS = ["null actions_dev (the bounds are relative to the nominal actions)", "null lo_host", "null hi_host", "a bound must not be NaN",
             "lo_host must be -infinity or finite, hi_host +infinity or finite", "a finite bound must lie in [-1, 1]",
             "lo must be < hi in both components", "mu_dev and a nonzero mu are both given", "ntraj exceeds what one launch covers"]


def test_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import box, control
    lib = box.load()
    nq, n = 3, 6
    buf = (C.c_double * 4096)()
    d = C.cast(buf, C.c_void_p)
    nan = float("nan")

    def Qm(i=None, j=None, v=0.0):
        m = np.eye(n)
        if i is not None:
            m[i, j] = v
        return (C.c_double * (n * n))(*m.reshape(-1))
    Rm = lambda *v: (C.c_double * 4)(*(v or (0.1, 0.0, 0.0, 0.1)))
    V = lambda *v: (C.c_double * len(v))(*v)

    def Lay(**kw):
        lay = control.layout(abi.F64, nq, 0, [0, 1, 3, -1])
        for k, v in kw.items():
            if k == "slot0":
                lay.slot_col[0] = v
            else:
                setattr(lay, k, v)
        return C.byref(lay)
    good = dict(lay=Lay(), K=2, M=4, a=d, b=d, lx=None, lu=None, q=Qm(), r=Rm(), mu=0.0, mu_dev=None, lo=V(-1.0, -1.0), hi=V(1.0, 1.0), pf=None,
                vf=None, gain=d, ff=None, po=None, vo=None, flag=None, dv=None, clamp=None, act=d, obs=None, al=None, nal=0, w=None)
    name = "os2rb_ilqr_backward_box"
    assert len(good) + 1 == len(box.ENTRY_POINTS[name])

    def call(**kw):
        a = dict(good, **kw)
        return getattr(lib, name)(*[a[k] for k in good], None)
    assert getattr(lib, name)(*[None if _is_pointer(t) else 0 for t in box.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rb_last_error() == b"os2rb_ilqr_backward_box: null layout"
    wts = dict(w=d, obs=d, al=V(1.0, 0.5), nal=2)
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(nq=1)), b"nq must be 2..5"),
             (dict(lay=Lay(nq=6)), b"nq must be 2..5"), (dict(K=0), b"nknots must be >= 1"), (dict(M=0), b"ntraj must be >= 1"),
             (dict(M=2 ** 62), b"ntraj exceeds what one launch covers"), (dict(a=None), b"null a_dev"), (dict(b=None), b"null b_dev"),
             (dict(q=None), b"null q_host"), (dict(r=None), b"null r_host"),
             (dict(act=None), b"null actions_dev"), (dict(lo=None), b"null lo_host"), (dict(hi=None), b"null hi_host"),
             (dict(q=Qm(1, 2, nan)), b"Q must be finite"), (dict(r=Rm(INF, 0.0, 0.0, 0.1)), b"R must be finite"),
             (dict(q=Qm(1, 2, 0.5)), b"Q must be exactly symmetric"), (dict(r=Rm(0.1, 0.01, 0.02, 0.1)), b"R must be exactly symmetric"),
             (dict(mu=nan), b"mu must be finite"), (dict(mu=INF), b"mu must be finite"), (dict(mu=-1e-9), b"mu must be >= 0"),
             (dict(mu=0.5, mu_dev=d), b"mu_dev and a nonzero mu are both given"),
             (dict(lo=V(nan, -1.0)), b"a bound must not be NaN"), (dict(hi=V(1.0, nan)), b"a bound must not be NaN"),
             (dict(hi=V(1.0, -nan)), b"a bound must not be NaN"),
             (dict(lo=V(INF, -1.0)), b"lo_host must be -infinity or finite"), (dict(hi=V(1.0, -INF)), b"lo_host must be -infinity or finite"),
             (dict(lo=V(-1.5, -1.0)), b"a finite bound must lie in [-1, 1]"), (dict(hi=V(1.0, 1.0000001)), b"a finite bound must lie in [-1, 1]"),
             (dict(lo=V(-1.0, 0.5), hi=V(1.0, 0.5)), b"lo must be < hi"), (dict(lo=V(0.25, -1.0), hi=V(0.0, 1.0)), b"lo must be < hi"),
             (dict(gain=None), b"all outputs are null"), (dict(gain=None, clamp=d, flag=d), b"all outputs are null"),
             (dict(wts, obs=None), b"weights need"), (dict(wts, al=None), b"weights need"),
             (dict(wts, nal=0), b"nalpha must be 1..16"), (dict(wts, nal=17), b"nalpha must be 1..16"),
             (dict(wts, al=V(1.0, nan)), b"alpha must be finite"), (dict(wts, lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"),
             (dict(wts, lay=Lay(obs_dim=13)), b"obs_dim must be 1..12"), (dict(wts, lay=Lay(slot0=n)), b"slot_col entries must be -1..n-1")]
    seen = set()
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.os2rb_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(b"os2rb_ilqr_backward_box: "), (kw.keys(), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases}) == 30                # each cause has a text of its own
    assert not any(buf)                                             # a refused call wrote nothing
    # the edges of the box are taken: the next refusal is about something else
    for kw in (dict(lo=V(-INF, -INF), hi=V(INF, INF)), dict(lo=V(-1.0, 0.999), hi=V(-0.999, 1.0)), dict(lo=V(-INF, 1.0), hi=V(-1.0, INF)),
               dict(mu=0.5), dict(mu=0.0, mu_dev=d), dict(mu=-0.0, mu_dev=d)):
        assert call(gain=None, **kw) == abi.ERR_INVALID and lib.os2rb_last_error().endswith(b"(gain, ff, pmat_out, pvec_out, dv, weights)"), kw
    # those of os2rc_ilqr_backward, and the new ones; every one before the device
    texts = checks_before_the_device("os2r_box_capi.hip", name, ("layout_refusal", "slots_refusal"))
    theirs = checks_before_the_device("os2r_control_capi.hip", "os2rc_ilqr_backward", ("layout_refusal", "slots_refusal"))
    assert set(theirs) <= set(texts) and set(texts) - set(theirs) <= set(NEW_TEXTS) and set(NEW_TEXTS) <= set(texts) and len(texts) == 30
    the_finite_and_symmetric_tests_make_no_hip_call()


# ---------------------------------------------------------------------------------------
# the Python layer, without a device
# ---------------------------------------------------------------------------------------
def test_the_bounds_of_the_python_layer():
    from gym_os2r_amd import box
    for given, lo, hi in ((True, (-1.0, -1.0), (1.0, 1.0)), ((-0.5, 0.5), (-0.5, -0.5), (0.5, 0.5)), (((-1, -0.25), 0.75), (-1.0, -0.25), (0.75, 0.75)),
                          ((-INF, (0.0, INF)), (-INF, -INF), (0.0, INF)), ((np.array([-1.0, 0.0]), [0.5, 1]), (-1.0, 0.0), (0.5, 1.0))):
        got = box.bounds(given)
        assert (tuple(got[0]), tuple(got[1])) == (lo, hi), given
    nan = float("nan")
    for bad in (False, None, 1.0, "ab", (1.0,), (-1.0, 0.0, 1.0), (nan, 1.0), (-1.0, (1.0, nan)), (INF, 1.0), (-1.0, -INF), (-2.0, 1.0), (-1.0, 1.5),
                (0.5, 0.5), (0.5, -0.5), ((-1.0, 0.5), (1.0, 0.25)), ("x", 1.0), ((-1.0, -1.0, -1.0), 1.0), (-1.0, [1.0])):
        with pytest.raises(ValueError, match="^ilqr_backward: "):
            box.bounds(bad)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return abi.OK
        return call


def test_python_argument_errors_and_what_reaches_c(monkeypatch):
    import torch
    from gym_os2r_amd import box, control, steer
    from gym_os2r_amd.sim import HipSim
    from test_ilqr_steer_host import _bare
    rec, reached = _Recorder(), []
    for name, module in (("box", box), ("control", control), ("steer", steer)):
        monkeypatch.setattr(module, "load", lambda name=name: (reached.append(name), rec)[1])
    s = _bare(torch.float64)
    s._control_layout = control.layout(abi.F64, 3, 0, [0, 1, 3, -1])
    s._stream = lambda: None
    assert "box" in HipSim.ilqr_backward.__kwdefaults__ and "clamp_out" in HipSim.ilqr_backward_into.__kwdefaults__
    n, D, K, M, f64 = 6, 4, 3, 4, torch.float64
    L = K * M
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    Q, R = torch.eye(n, dtype=f64), 0.1 * torch.eye(2, dtype=f64)
    A, B = z(L, n, n), z(L, n, 2)
    a, b = A.permute(1, 2, 0).contiguous(), B.permute(1, 2, 0).contiguous()
    act, gains, clamp = z(L, 2), z(K, 2, n, M), torch.zeros(K, M, dtype=torch.uint8)
    # refused before a library is reached
    for kw in (dict(box=True), dict(box=(-0.5, 0.5), actions=None), dict(box=(0.5, -0.5), actions=act), dict(box=(-2.0, 1.0), actions=act),
               dict(box="ab", actions=act), dict(box=True, actions=z(L + 1, 2))):
        with pytest.raises(ValueError, match="^ilqr_backward: "):
            s.ilqr_backward(A, B, Q, R, knots=K, **kw)
        with pytest.raises(ValueError, match="^ilqr_backward: "):
            s.ilqr_backward_into(a, b, Q, R, knots=K, gains_out=gains, **kw)
    for kw in (dict(clamp_out=clamp), dict(box=True, actions=act.float()), dict(box=True, actions=act, clamp_out=z(K, M)), dict(box=True, actions=act, clamp_out=clamp[:, :3]),
               dict(box=True, actions=act, mu=0.5, mu_dev=z(M))):
        with pytest.raises(ValueError, match="^ilqr_backward: "):
            s.ilqr_backward_into(a, b, Q, R, knots=K, gains_out=gains, **kw)
    assert reached == [] and rec.calls == []
    # what reaches C: the scalar mu and a null mu_dev, the bounds, the clamp bytes behind dv, the actions without a table
    s.ilqr_backward_into(a, b, Q, R, knots=K, mu=0.25, gains_out=gains, actions=act, obs=z(L, D), box=((-1.0, -0.5), 0.75), clamp_out=clamp)
    (name, args), = rec.calls
    assert name == "os2rb_ilqr_backward_box" and reached == ["box"] and len(args) == len(box.ENTRY_POINTS[name]) == 28
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x
    assert args[1:3] == (K, M) and ptr(args[3]) == a.data_ptr() and ptr(args[4]) == b.data_ptr()
    assert args[9] == 0.25 and args[10] is None and list(args[11]) == [-1.0, -0.5] and list(args[12]) == [0.75, 0.75]
    assert ptr(args[15]) == gains.data_ptr() and args[20] is None and ptr(args[21]) == clamp.data_ptr() and ptr(args[22]) == act.data_ptr()
    assert args[23] is None and args[24] is None and args[25] == 0 and args[26] is None        # no table: obs does not reach the library
    mu_dev = z(M)
    s.ilqr_backward_into(a, b, Q, R, knots=K, gains_out=gains, actions=act, box=True, mu_dev=mu_dev)
    name, args = rec.calls[-1]
    assert name == "os2rb_ilqr_backward_box" and args[9] == 0.0 and ptr(args[10]) == mu_dev.data_ptr() and args[21] is None
    assert list(args[11]) == [-1.0, -1.0] and list(args[12]) == [1.0, 1.0]
    # the allocating form: one more member, [K, M] uint8; without box the tuple and the library are as they were
    out = s.ilqr_backward(A, B, Q, R, knots=K, actions=act, box=True)
    assert len(out) == 8 and out[7].dtype == torch.uint8 and tuple(out[7].shape) == (K, M) and ptr(rec.calls[-1][1][21]) == out[7].data_ptr()
    assert ptr(rec.calls[-1][1][22]) == act.data_ptr()
    for off in (None, False):
        assert len(s.ilqr_backward(A, B, Q, R, knots=K, actions=act, box=off)) == 7 and rec.calls[-1][0] == "os2rc_ilqr_backward"
    assert len(s.ilqr_backward(A, B, Q, R, knots=K, mu_dev=mu_dev)) == 7 and rec.calls[-1][0] == "os2rt_ilqr_backward_mu"
    assert reached == ["box", "box", "box", "control", "control", "steer"]
