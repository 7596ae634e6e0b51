"""libos2r_ukf.so (include/os2r_ukf.h): the host side -- the numpy restatements of the two launches the GPU tests compare with
(`restate_ukf_points`, `restate_ukf_update`) on crafted inputs that reach every branch of them (`crafted_ukf`), their exact
properties, the restatements against the textbook in float64, the header against the one table of gym_os2r_amd/ukf.py, the
exports of the library, the other eight libraries as they were, the resources of the sixteen kernels in the built library, every
refusal of both entry points through ctypes without a device, weights(), the argument checks of the four HipSim methods that need
no device and what they pass to C.  No GPU needed."""
import ctypes as C
import math
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
from header_check import _agrees, _header, _is_pointer, _prototypes, checks_before_the_device  # noqa: E402
from test_ekf_host import D, GATE, M, MAX_OBS, NQ, ROBOTS, Recorder, _bare, _decode, _dot, n, restate_ekf, same_bits, slot_columns  # noqa: E402

NAMES = ["os2ru_abi_version", "os2ru_last_error", "os2ru_ukf_points", "os2ru_ukf_update"]
P_CLASSES = ("generic", "pivot 0 fails", "a middle pivot fails", "the last pivot fails", "NaN on the diagonal", "garbage below the diagonal")
U_CLASSES = ("generic", "a done lane", "a lane that is not finite", "lost, point 0 not finite", "one reading gated", "huge innovation",
             "one NaN reading", "p_in all NaN")
BRANCH_SHAPE = (70, 5, 10)               # M, nq, D: three workgroups with a tail


# ---------------------------------------------------------------------------------------
# the restatements of include/os2r_ukf.h (need no device)
# ---------------------------------------------------------------------------------------
def restate_ukf_points(x, p, gamma, *, dtype):
    """os2ru_ukf_points in numpy and in `dtype`, every robot at once: x [n, M], p [n, n, M] (upper triangle read).
    -> dict(points [n, S M], failed [M] int32, L [n, n, M]: the factor, meaningless where failed)."""
    x, P = np.array(x, dtype), np.array(p, dtype)
    nn, MM = x.shape
    S = 2 * nn + 1
    g = dtype(gamma)
    L = np.zeros((nn, nn, MM), dtype)
    failed = np.zeros(MM, np.int32)
    with np.errstate(all="ignore"):
        for j in range(nn):
            t = P[j, j].copy()
            if j:
                t = t - _dot(L[j, :j], L[j, :j], dtype)
            bad = ~(np.isfinite(t) & (t > 0))
            failed = np.where((failed == 0) & bad, j + 1, failed).astype(np.int32)
            d = np.sqrt(t)
            L[j, j] = d
            for i in range(j + 1, nn):
                u = P[j, i].copy()
                if j:
                    u = u - _dot(L[i, :j], L[j, :j], dtype)
                L[i, j] = u / d
            assert t.dtype == dtype and d.dtype == dtype
        ok = failed == 0
        pts = np.empty((nn, S, MM), dtype)
        pts[:, 0] = x
        for j in range(nn):
            gl = g * L[:, j]
            pts[:, 1 + j] = np.where(ok[None], x + gl, x)
            pts[:, 1 + nn + j] = np.where(ok[None], x - gl, x)
            assert gl.dtype == dtype
    return dict(points=pts.reshape(nn, S * MM), failed=failed, L=L)


def restate_ukf_update(q, qd, done, p_in, q_noise, scalars, meas, prec, slot_col, *, gate=0.0, dtype, want_points=True):
    """os2ru_ukf_update in numpy and in `dtype`, every robot at once: q, qd [nq, S M], done [S M] or None, p_in [n, n, M],
    q_noise [n, n], scalars (gamma, wm0, wc0, wi).  -> restate_ekf's dict (x, p, nis, used, refused, innov, p_minus) with lost [M]
    int32, x_minus [n, M] and, want_points, points [n, S M] and failed [M] int32."""
    q, qd = np.array(q, dtype), np.array(qd, dtype)
    nq = q.shape[0]
    nn = 2 * nq
    S = 2 * nn + 1
    MM = q.shape[1] // S
    gamma, wm0, wc0, wi = (dtype(v) for v in scalars)
    chi = np.concatenate([q.reshape(nq, S, MM), qd.reshape(nq, S, MM)])             # [n, S, M]
    lost = ~np.isfinite(chi).all(axis=(0, 1))
    if done is not None:
        lost |= (np.asarray(done).reshape(S, MM) != 0).any(axis=0)
    pin, Q = np.array(p_in, dtype), np.array(q_noise, dtype)
    with np.errstate(all="ignore"):
        acc = chi[:, 1].copy()
        for s in range(2, S):
            acc = acc + chi[:, s]
        xbar = wm0 * chi[:, 0] + wi * acc
        d = chi - xbar[:, None]
        Pm = np.empty((nn, nn, MM), dtype)
        for i in range(nn):
            for j in range(i, nn):
                fresh = Q[i, j] + (wc0 * (d[i, 0] * d[j, 0]) + wi * _dot(d[i, 1:], d[j, 1:], dtype))
                Pm[i, j] = Pm[j, i] = np.where(lost, pin[i, j], fresh)
        assert xbar.dtype == dtype and Pm.dtype == dtype and d.dtype == dtype
        x_minus = np.where(lost[None], chi[:, 0], xbar)
    out = restate_ekf(x_minus, Pm, meas, prec, slot_col, a=None, gate=gate, dtype=dtype)
    out.update(lost=lost.astype(np.int32), x_minus=x_minus)
    if want_points:
        pts = restate_ukf_points(out["x"], out["p"], gamma, dtype=dtype)
        out.update(points=pts["points"], failed=pts["failed"])
    return out


def crafted_ukf(MM, nq, DD, seed=0, dtype=np.float64, variant=0):
    """Inputs in float64 (the caller rounds) that reach every branch of both launches.
    For os2ru_ukf_points: x [n, M] and p [n, n, M], well conditioned (0.05 I plus a random Gram matrix of that size: condition
    number below 30), the robot classes m % 6 (P_CLASSES): 1 P[0][0] = -1; 2 P[n/2][n/2] = -0.3; 3 P[n-1][n-1] = 0, so the last
    pivot is negative; 4 P[1][1] = NaN; 5 NaN below the diagonal, which is never read.
    For os2ru_ukf_update: the float64 sigma points of the clean (x, P) pushed through chi -> F chi + b on the host, F = I + 0.05
    N(0, 1) per robot -- the unscented prediction of a linear map is F P F' + Q --, Q = 0.01 (I + a Gram matrix), prec in 50..200
    with the entry of slot 2 equal to 0 (variant 1: NaN), every reading 0.7 standard deviations of its innovation about the
    predicted mean, the last slot on the column of slot 0; scalars the defaults of weights() (variant 1: kappa = -1, a negative
    wm0).  The robot classes m % 8 (U_CLASSES), d0 slot 0: 1 a done lane, and p_in[1][1] = NaN (step 4 fails at column 1);
    2 a lane holds +inf, and p_in[c0][c0] = -1 (slot d0 is refused, step 4 fails); 3 point 0 holds a NaN; 4 the reading of d0
    lies 30 standard deviations away; 5 it is so far that z overflows; 6 it is NaN; 7 p_in is NaN everywhere, which a robot that
    is not lost never reads.  Below the diagonal p_in is NaN in every robot.
    -> dict(x, p, q [nq, S M], qd, done [S M] uint8, p_in, p_clean [n, n, M], F [M, n, n], b [n, M], q_noise [n, n], scalars, meas,
    prec, slot_col)"""
    from gym_os2r_amd import ukf
    rng = np.random.default_rng(1000 + seed)
    nn = 2 * nq
    S = 2 * nn + 1
    cols = slot_columns(nn, DD, seed)
    x = rng.uniform(-1.0, 1.0, (nn, MM))
    G = rng.normal(0.0, 1.0, (MM, nn, nn))
    P = 0.05 * np.eye(nn)[None] + 0.05 / nn * G @ G.transpose(0, 2, 1)
    P = 0.5 * (P + P.transpose(0, 2, 1))
    assert np.linalg.cond(P).max() < 1e4
    scalars = ukf.weights(nn, kappa=-1.0) if variant else ukf.weights(nn)
    gamma = scalars[0]
    p_clean = np.ascontiguousarray(P.transpose(1, 2, 0))
    m = np.arange(MM)
    # the points launch's own P
    p = p_clean.copy()
    pc = m % 6
    p[0, 0, pc == 1] = -1.0
    p[nn // 2, nn // 2, pc == 2] = -0.3
    p[nn - 1, nn - 1, pc == 3] = 0.0
    p[1, 1, pc == 4] = np.nan
    for i in range(nn):
        p[i, :i, pc == 5] = np.nan
    # the propagated points
    L = np.linalg.cholesky(P)                                                    # [M, n, n]
    chi = np.empty((MM, S, nn))
    chi[:, 0] = x.T
    for j in range(nn):
        chi[:, 1 + j] = x.T + gamma * L[:, :, j]
        chi[:, 1 + nn + j] = x.T - gamma * L[:, :, j]
    F = np.eye(nn)[None] + 0.05 * rng.normal(0.0, 1.0, (MM, nn, nn))
    b = rng.uniform(-0.2, 0.2, (nn, MM))
    chi = np.einsum("mij,msj->msi", F, chi) + b.T[:, None, :]
    Gq = rng.normal(0.0, 1.0, (nn, nn))
    Q = 0.01 * (np.eye(nn) + Gq @ Gq.T / nn)
    Q = 0.5 * (Q + Q.T)
    prec = rng.uniform(50.0, 200.0, DD)
    if DD >= 4:
        prec[2] = np.nan if variant else 0.0
    mean = np.einsum("mij,jm->im", F, x) + b
    Pm = F @ P @ F.transpose(0, 2, 1) + Q[None]
    meas = np.empty((MM, DD))
    for d, c in enumerate(cols):
        sd = np.sqrt(Pm[:, max(c, 0), max(c, 0)] + 1.0 / np.where(prec[d] > 0, prec[d], 1.0))
        meas[:, d] = mean[max(c, 0)] + 0.7 * sd * rng.normal(0.0, 1.0, MM)
    uc = m % 8
    c0 = cols[0]
    sd0 = np.sqrt(Pm[:, c0, c0] + 1.0 / prec[0])
    done = np.zeros((S, MM), np.uint8)
    done[(3 + m[uc == 1]) % S, m[uc == 1]] = 1 + m[uc == 1] % 3                  # any flag that is not 0
    chi[uc == 2, 2 * nn, nn - 1] = np.inf
    chi[uc == 3, 0, 1] = np.nan
    meas[uc == 4, 0] = mean[c0, uc == 4] + 30.0 * sd0[uc == 4]
    meas[uc == 5, 0] = 1e200 if dtype == np.float64 else 1e30
    meas[uc == 6, 0] = np.nan
    p_in = p_clean.copy()
    p_in[1, 1, uc == 1] = np.nan
    p_in[c0, c0, uc == 2] = -1.0
    p_in[:, :, uc == 7] = np.nan
    for i in range(nn):
        p_in[i, :i] = np.nan
    lanes = np.ascontiguousarray(chi.transpose(2, 1, 0)).reshape(nn, S * MM)      # [n][s M + m]
    return dict(x=x, p=p, q=lanes[:nq].copy(), qd=lanes[nq:].copy(), done=done.reshape(-1), p_in=p_in, p_clean=p_clean, F=F, b=b, q_noise=Q,
                scalars=scalars, meas=meas, prec=prec, slot_col=cols)


def restated_update(c, dtype, gate=GATE, done=True, want_points=True):
    return restate_ukf_update(c["q"], c["qd"], c["done"] if done else None, c["p_in"], c["q_noise"], c["scalars"], c["meas"], c["prec"],
                              c["slot_col"], gate=gate, dtype=dtype, want_points=want_points)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatements_on_crafted_inputs_that_reach_every_branch(dtype, variant):
    MM, nq, DD = BRANCH_SHAPE
    nn = 2 * nq
    S = 2 * nn + 1
    c = crafted_ukf(MM, nq, DD, dtype=dtype, variant=variant)
    cols = c["slot_col"]
    assert MM > 2 * ROBOTS and MM % ROBOTS and cols.count(-1) == 2 and cols[DD - 1] == cols[0]
    assert (np.isnan(c["prec"][2]) if variant else c["prec"][2] == 0) and (c["scalars"][1] < 0 if variant else c["scalars"][1] == 0)
    # the points
    pts = restate_ukf_points(c["x"], c["p"], c["scalars"][0], dtype=dtype)
    pc = np.arange(MM) % 6
    want_failed = np.select([pc == 1, pc == 2, pc == 3, pc == 4], [1, nn // 2 + 1, nn, 2], 0)
    assert np.array_equal(pts["failed"], want_failed) and pts["failed"].dtype == np.int32
    cube = pts["points"].reshape(nn, S, MM)
    x = c["x"].astype(dtype)
    assert pts["points"].dtype == dtype and np.isfinite(pts["points"]).all()
    assert same_bits(cube[:, :, want_failed != 0], np.broadcast_to(x[:, None], cube.shape)[:, :, want_failed != 0])   # failed: all points are x
    ok = want_failed == 0
    for j in range(nn):
        assert same_bits(cube[:j, 1 + j], x[:j]) and same_bits(cube[:j, 1 + nn + j], x[:j])     # chi_{1+j}[i] = x_i exactly for i < j
        assert (cube[j, 1 + j, ok] > x[j, ok]).all() and (cube[j, 1 + nn + j, ok] < x[j, ok]).all()
    assert same_bits(cube[:, 0], x)
    clean = restate_ukf_points(c["x"], np.where(np.isnan(c["p"]) & (pc == 5)[None, None], 0.0, c["p"]), c["scalars"][0], dtype=dtype)
    assert np.isnan(c["p"][:, :, pc == 5]).any() and same_bits(clean["points"], pts["points"])  # below the diagonal: never read
    # the update
    uc = np.arange(MM) % 8
    live = [d for d in range(DD) if cols[d] >= 0 and d != 2]
    all_bits = int(sum(1 << d for d in live))
    out, free = restated_update(c, dtype), restated_update(c, dtype, gate=0.0)
    assert np.array_equal(out["lost"], np.isin(uc, (1, 2, 3)).astype(np.int32))
    assert np.array_equal(restated_update(c, dtype, done=False)["lost"], np.isin(uc, (2, 3)).astype(np.int32))
    used, refused = out["used"], out["refused"]
    assert not (used & ~all_bits).any() and not (refused & ~all_bits).any()          # a dropped slot sets neither bit
    for k in (0, 7):
        assert (refused[uc == k] == 0).all() and (free["used"][uc == k] == all_bits).all()
    # lost: x before the slots is point 0 and P- the P it came with, no Q added
    chi0 = np.concatenate([c["q"][:, :MM], c["qd"][:, :MM]]).astype(dtype)
    for k in (1, 2, 3):
        assert same_bits(out["x_minus"][:, uc == k], chi0[:, uc == k])
        sel = np.triu(np.ones((nn, nn), bool))
        assert same_bits(out["p_minus"][:, :, uc == k][sel], c["p_in"].astype(dtype)[:, :, uc == k][sel])
    on1 = int(sum(1 << d for d in live if cols[d] == 1))                                          # p_in[1][1] = NaN: its slots refuse, step 4 fails
    assert (free["refused"][uc == 1] == on1).all() and (free["used"][uc == 1] == all_bits & ~on1).all() and (out["failed"][uc == 1] == 2).all()
    assert (refused[uc == 2] & 1 == 1).all() and (out["failed"][uc == 2] != 0).all()              # p_in[c0][c0] = -1
    assert np.isnan(out["x"][1, uc == 3]).all() and (used[uc == 3] & on1 == 0).all()              # point 0 not finite
    bit1 = [d for d in live if cols[d] == 1]
    if bit1:
        assert (refused[uc == 3] >> bit1[0] & 1 == 1).all()                                       # its slot refuses itself (z is NaN)
    assert (used[uc == 4] & 1 == 0).all() and (refused[uc == 4] & 1 == 0).all() and (free["used"][uc == 4] & 1 == 1).all()
    assert (refused[uc == 5] & 1 == 1).all() and (used[uc == 5] != 0).all()
    assert (free["used"][uc == 6] == all_bits & ~1).all() and (refused[uc == 6] == 0).all()
    good = np.isin(uc, (0, 4, 5, 6, 7))
    assert (out["failed"][good] == 0).all() and np.isfinite(out["p"][:, :, good]).all() and np.isfinite(out["points"][:, np.tile(good, S)]).all()
    for k in ("x", "p", "nis", "innov", "points"):
        assert out[k].dtype == dtype, k


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exact_properties_on_every_robot(dtype):
    """p_out is bitwise symmetric; step 2 fed with the restated x and P- is restate_ekf without a time update, bit for bit; step 4
    is restate_ukf_points of the update's own outputs; a robot that is not lost never reads p_in."""
    MM, nq, DD = BRANCH_SHAPE
    for variant, gate in ((0, GATE), (1, 0.0)):
        c = crafted_ukf(MM, nq, DD, dtype=dtype, variant=variant)
        out = restated_update(c, dtype, gate)
        assert same_bits(out["p"], out["p"].transpose(1, 0, 2)) and same_bits(out["p_minus"], out["p_minus"].transpose(1, 0, 2))
        again = restate_ekf(out["x_minus"], out["p_minus"], c["meas"], c["prec"], c["slot_col"], a=None, gate=gate, dtype=dtype)
        for k in ("x", "p", "nis", "innov"):
            assert same_bits(again[k], out[k]), k
        assert np.array_equal(again["used"], out["used"]) and np.array_equal(again["refused"], out["refused"])
        pts = restate_ukf_points(out["x"], out["p"], c["scalars"][0], dtype=dtype)
        assert same_bits(pts["points"], out["points"]) and np.array_equal(pts["failed"], out["failed"])
        assert (out["used"] & out["refused"] == 0).all()
        other = dict(c, p_in=np.where((out["lost"] == 0)[None, None], 7.0, c["p_in"]))
        assert all(np.array_equal(restated_update(other, dtype, gate)[k], out[k], equal_nan=True) for k in out)


# 100 x the worst distances measured for these very inputs on the CPU: float64 4.44e-16 (points), 1.1e-15 (P), 6.66e-16 (x),
# 4.19e-15 (nis); float32 1.8e-7, 3.24e-7, 2.16e-7, 2.78e-6
TEXTBOOK_BOUNDS = {np.float64: (4.44e-14, 1.1e-13, 6.66e-14, 4.19e-13), np.float32: (1.8e-5, 3.24e-5, 2.16e-5, 2.78e-4)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_against_the_textbook_in_float64(dtype):
    """The robots that reach no special branch, gate 0, both sets of weights: the points of the restatement in `dtype` against
    x +- gamma np.linalg.cholesky(P) in float64; then those points pushed through chi -> F chi + b on the host in float64 and
    rounded, and the restated update against the textbook from the same (rounded) x and P -- the prediction F P F' + Q about F x + b,
    K = P- H'(H P- H' + R)^-1, x + K (y - H x), (I - K H) P- and nu' S^-1 nu.  The distances in the points and in x are absolute
    (the states are of order 1), the one in P relative to the largest entry of the robot's P, the one in nis relative to nis."""
    worst = np.zeros(4)
    for nq, DD, seed, variant in ((2, 3, 1, 0), (3, 6, 2, 1), (4, 8, 3, 0), (5, 10, 4, 1), (5, 12, 5, 0)):
        MM, nn = 48, 2 * nq
        S = 2 * nn + 1
        c = crafted_ukf(MM, nq, DD, seed=seed, dtype=dtype, variant=variant)
        gamma = c["scalars"][0]
        r64 = lambda v: np.asarray(v).astype(dtype).astype(np.float64)
        x, P = r64(c["x"]), r64(c["p_clean"])
        pts = restate_ukf_points(x, P, gamma, dtype=dtype)
        assert (pts["failed"] == 0).all()
        L = np.linalg.cholesky(P.transpose(2, 0, 1))
        cube = pts["points"].reshape(nn, S, MM).astype(np.float64)
        for j in range(nn):
            worst[0] = max(worst[0], np.abs(cube[:, 1 + j] - (x + gamma * L[:, :, j].T)).max(), np.abs(cube[:, 1 + nn + j] - (x - gamma * L[:, :, j].T)).max())
        F, b = c["F"], c["b"]
        moved = (np.einsum("mij,jsm->ism", F, cube) + b[:, None, :]).reshape(nn, S * MM)
        out = restate_ukf_update(moved[:nq], moved[nq:], None, c["p_in"], c["q_noise"], c["scalars"], c["meas"], c["prec"], c["slot_col"],
                                 gate=0.0, dtype=dtype, want_points=False)
        live = [d for d in range(DD) if c["slot_col"][d] >= 0 and r64(c["prec"])[d] > 0]
        H = np.zeros((len(live), nn))
        H[np.arange(len(live)), [c["slot_col"][d] for d in live]] = 1.0
        R = np.diag(1.0 / r64(c["prec"])[live])
        for m in [m for m in range(MM) if m % 8 in (0, 7)]:
            Pm = F[m] @ P[:, :, m] @ F[m].T + r64(c["q_noise"])
            xm = F[m] @ x[:, m] + b[:, m]
            nu = r64(c["meas"])[m, live] - H @ xm
            Sm = H @ Pm @ H.T + R
            K = np.linalg.solve(Sm, H @ Pm).T
            xp, Pp, nis = xm + K @ nu, (np.eye(nn) - K @ H) @ Pm, nu @ np.linalg.solve(Sm, nu)
            assert out["used"][m] == sum(1 << d for d in live) and out["refused"][m] == 0 and out["lost"][m] == 0
            dist = (np.abs(out["p"][:, :, m] - Pp).max() / np.abs(Pp).max(), np.abs(out["x"][:, m] - xp).max(), abs(out["nis"][m] - nis) / nis)
            worst[1:] = np.maximum(worst[1:], dist)
    print(f"ukf against the textbook, {dtype.__name__}: worst distance in the points {worst[0]:.3g}, in P {worst[1]:.3g}, in x {worst[2]:.3g}, "
          f"in nis {worst[3]:.3g}")
    assert (worst <= TEXTBOOK_BOUNDS[dtype]).all(), worst


# ---------------------------------------------------------------------------------------
# header, table, exports
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import control, ukf
    protos = _prototypes("os2r_ukf.h", "os2ru")
    assert [p[0] for p in protos] == list(ukf.ENTRY_POINTS) == NAMES
    lib = ukf.load()
    for name, ret, args in protos:
        argtypes = ukf.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2ru_last_error" else C.c_int)
    args = protos[2][2]
    assert args[0] == "const Os2rControlLayout* layout" and args[1] == "int64_t nrobots" and args[4] == "double gamma"
    assert args[6] == "int32_t* failed_dev" and args[-1] == "void* stream" and len(args) == 8
    args = protos[3][2]
    assert args[0] == "const Os2rControlLayout* layout" and args[1] == "int64_t nrobots" and args[4] == "const uint8_t* done_dev"
    assert args[6] == "const double* q_host" and args[7:11] == ["double gamma", "double wm0", "double wc0", "double wi"] and args[13] == "double gate"
    assert args[20:23] == ["int32_t* lost_dev", "void* points_out_dev", "int32_t* failed_dev"] and args[-1] == "void* stream" and len(args) == 24
    table = ukf.ENTRY_POINTS["os2ru_ukf_update"]
    assert all(table[i] is C.c_double for i in (7, 8, 9, 10, 13)) and table[1] is C.c_int64 and table[6] is C.POINTER(C.c_double)
    header = _header("os2r_ukf.h")
    assert re.search(r"#define OS2R_UKF_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    for word in ("periodic wrap", "not raw", "augmented state", "square-root form", "weights per robot", "several filter steps per launch"):
        assert word in header, word                                       # the out-of-scope list
    assert lib.os2ru_abi_version() == ukf.ABI_VERSION == 1
    assert ukf.Os2rControlLayout is control.Os2rControlLayout and ukf.layout is control.layout and ukf.MAX_OBS == MAX_OBS
    assert issubclass(ukf.Os2rUkfLibraryMissing, ImportError) and [ukf.npoints(k) for k in (2, 5)] == [9, 21]
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", ukf.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)


def test_the_other_libraries_are_as_they_were():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib, control, ekf, mppi, pf, search, steer, ukf
    tables = {_lib.LIB_PATH: _lib.ENTRY_POINTS, _lib.RECORD_LIB_PATH: _lib.RECORD_ENTRY_POINTS, control.LIB_PATH: control.ENTRY_POINTS,
              search.LIB_PATH: search.ENTRY_POINTS, steer.LIB_PATH: steer.ENTRY_POINTS, mppi.LIB_PATH: mppi.ENTRY_POINTS,
              pf.LIB_PATH: pf.ENTRY_POINTS, ekf.LIB_PATH: ekf.ENTRY_POINTS}
    others = set().union(*tables.values())
    assert len(tables) == 8 and not set(ukf.ENTRY_POINTS) & others and not any(name.startswith("os2ru_") for name in others)
    for name in ("os2r.h", "os2r_control.h", "os2r_record.h", "os2r_search.h", "os2r_steer.h", "os2r_mppi.h", "os2r_pf.h", "os2r_ekf.h"):
        assert "os2ru_" not in _header(name) and "os2r_ukf" not in _header(name).lower(), name
    assert len(_lib.ENTRY_POINTS) == 35 and len(_lib.RECORD_ENTRY_POINTS) == 3
    assert list(ekf.ENTRY_POINTS) == ["os2re_abi_version", "os2re_last_error", "os2re_ekf_update"]
    for path, table in tables.items():
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(table), path
        kernels = kernel_meta.kernel_meta(path)
        assert kernels and not any("ukf" in k.lower() for k in kernels), path
    # ... and the new library holds none of theirs
    forbidden = ("ekf", "pf_update", "mppi", "steer", "_mu_kernel", "line_search", "record", "ilqr_backward_kernel", "lqr_gains_kernel<")
    mine = kernel_meta.kernel_meta(ukf.LIB_PATH)
    assert len(mine) == 16 and not any(word in k for k in mine for word in forbidden)


def lds_bounds(nn, size):
    """The bounds the header comment of csrc/os2r_ukf.hpp states -> (ukf_points_kernel, ukf_update_kernel)."""
    return (nn * nn + nn) * ROBOTS * size, ((max(nn * nn, 9 * nn) + 2 * nn + MAX_OBS) * ROBOTS + nn * nn + MAX_OBS) * size + (ROBOTS * nn + MAX_OBS) * 4


def test_kernel_resources():
    """Exactly sixteen kernels, the two families in float and double for chains of 2..5 dofs, are in the built library and none
    uses scratch: private_segment_fixed_size 0, no VGPR or SGPR spill and no AGPRs in the code-object metadata.  The static LDS is
    within the bounds the header comment states, every kernel leaves room for four waves on a SIMD (at most 128 registers), and
    there is no dynamic LDS: the launches pass 0."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import ukf
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(ukf.LIB_PATH)
    meta = kernel_meta.kernel_meta(ukf.LIB_PATH)
    assert len(meta) == 16, sorted(meta)
    src = open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "os2r_ukf.hpp")).read()
    assert "ukf_points_kernel: (n n + n) 32 sizeof(T) bytes -- 28160 for double and nq = 5" in src
    assert "ukf_update_kernel: ((max(n n, 9 n) + 2 n + 12) 32 + n n + 12) sizeof(T) + (32 n + 12) * 4 bytes -- 36016 for double and nq = 5" in src
    assert lds_bounds(10, 8) == (28160, 36016) and 4 * 36016 <= 160 * 1024
    assert re.search(r"constexpr int kUkfRobots = (\d+);", src).group(1) == str(ROBOTS) and "#pragma clang fp contract(off)" in src
    for real, size in (("float", 4), ("double", 8)):
        for nq in (2, 3, 4, 5):
            for family, bound in zip(("ukf_points_kernel", "ukf_update_kernel"), lds_bounds(2 * nq, size)):
                (name,) = [k for k in meta if f"{family}<{real}, {nq}>" in k]
                m = meta[name]
                assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
                assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 128, (name, m)
                assert 0 < m["group_segment_fixed_size"] <= bound, (name, m, bound)
    inst = open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "os2r_ukf_inst.hip")).read()
    assert "hipLaunchKernelGGL((ukf_points_kernel<T, NQ>), grid, block, 0, s, p)" in inst      # no dynamic LDS
    assert "hipLaunchKernelGGL((ukf_update_kernel<T, NQ>), grid, block, 0, s, p)" in inst and inst.count("by_chain_length(nq,") == 2


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def test_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import control, ukf
    lib = ukf.load()
    MM, nq = 4, 3
    nn = 2 * nq
    S = 2 * nn + 1
    buf = (C.c_double * 8192)()
    base = C.addressof(buf)
    at = lambda i: C.c_void_p(base + 8 * i)
    top = lambda back: C.c_void_p(2 ** 64 - back)
    nan, inf = float("nan"), float("inf")
    eye = [1.0 if i == j else 0.0 for i in range(nn) for j in range(nn)]
    dbl = lambda values: (C.c_double * len(values))(*values)

    def Lay(dtype=abi.F64, cols=(0, 1, 3, -1), **kw):
        lay = control.layout(dtype, nq, 0, list(cols))
        for k, v in kw.items():
            setattr(lay, k, v)
        return C.byref(lay)

    def q_with(i, j, value):
        q = list(eye)
        q[i * nn + j] = value
        return dbl(q)
    X, PM, NS = nn * MM, nn * nn * MM, nn * S * MM
    HALF = NS // 2
    layout_cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"layout->dtype must be OS2R_F32 or OS2R_F64"),
                    (dict(lay=Lay(nq=1)), b"layout->nq must be 2..5"), (dict(lay=Lay(nq=6)), b"layout->nq must be 2..5")]
    count_cases = [(dict(M=0), b"nrobots must be >= 1"), (dict(M=-1), b"nrobots must be >= 1"), (dict(M=2 ** 62), b"n * S * nrobots exceeds 2^31 - 1"),
                   (dict(M=(2 ** 31 - 1) // (nn * S) + 1), b"n * S * nrobots exceeds 2^31 - 1")]

    def run(name, good, cases, edges, last_kw, last, helpers, total, at_the_limit):
        fn, prefix = getattr(lib, name), name.encode() + b": "
        assert len(good) + 1 == len(ukf.ENTRY_POINTS[name])

        def call(**kw):
            a = dict(good, **kw)
            return fn(*[a[k] for k in good], None)
        assert fn(*[None if _is_pointer(t) else 0 for t in ukf.ENTRY_POINTS[name]]) == abi.ERR_INVALID
        assert lib.os2ru_last_error() == prefix + b"null layout"
        seen = set()
        for kw, msg in cases:
            rc = call(**kw)
            err = lib.os2ru_last_error()
            assert rc == abi.ERR_INVALID and err == prefix + msg, (name, kw.keys(), msg, rc, err)
            seen.add(err)
        assert len(seen) == len({m for _, m in cases}) == total           # each cause has a text of its own
        assert not any(buf)                                               # a refused call wrote nothing
        # the edges are taken: the next refusal is about something else (no call here is let through to a device)
        for kw in edges:
            assert call(**dict(kw, **last_kw)) == abi.ERR_INVALID and lib.os2ru_last_error() == prefix + last, (name, kw)
        # nrobots at the int32 limit (every array then covers the whole buffer: the next refusal is a scalar's)
        kw, msg = at_the_limit
        assert call(M=(2 ** 31 - 1) // (nn * S), **kw) == abi.ERR_INVALID and lib.os2ru_last_error() == prefix + msg
        assert not any(buf)
        texts = checks_before_the_device("os2r_ukf_capi.hip", name, helpers)
        assert len(texts) == total and {prefix + t.encode() for t in texts} == seen

    # os2ru_ukf_points
    good = dict(lay=Lay(), M=MM, x=at(0), p=at(1024), gamma=2.0, points=at(4096), failed=None)
    cases = layout_cases + count_cases + [
        (dict(x=None), b"null x_dev"), (dict(p=None), b"null p_dev"), (dict(points=None), b"null points_dev"),
        (dict(gamma=nan), b"gamma must be finite"), (dict(gamma=inf), b"gamma must be finite"), (dict(gamma=0.0), b"gamma must be > 0"),
        (dict(gamma=-1.0), b"gamma must be > 0"), (dict(gamma=-0.0), b"gamma must be > 0"),
        (dict(points=at(0)), b"points_dev overlaps x_dev"), (dict(points=at(X - 1)), b"points_dev overlaps x_dev"),
        (dict(x=at(4096 + NS - 1)), b"points_dev overlaps x_dev"), (dict(points=at(1024 + PM - 1)), b"points_dev overlaps p_dev"),
        (dict(points=at(1024 - NS + 1)), b"points_dev overlaps p_dev"),
        # (arrays whose ends wrap round at the top of the address space: the check is on the distance)
        (dict(M=2 ** 18, x=top(65), points=top(33)), b"points_dev overlaps x_dev"),
        (dict(M=2 ** 18, p=top(65), points=top(33)), b"points_dev overlaps p_dev")]
    edges = [dict(gamma=5e-324), dict(gamma=1.7e308), dict(x=at(4096 - X)), dict(lay=Lay(obs_dim=0)),
             dict(lay=Lay(cols=(99, 0, 0, 0))), dict(failed=at(0))]
    run("os2ru_ukf_points", good, cases, edges, dict(p=at(4096 + NS - 1)), b"points_dev overlaps p_dev", ("layout_refusal",), 12,
        (dict(gamma=nan), b"gamma must be finite"))

    # os2ru_ukf_update
    good = dict(lay=Lay(), M=MM, q=at(2048), qd=at(2048 + HALF), done=None, pin=at(1024), Q=dbl(eye), gamma=2.0, wm0=0.0, wc0=2.0, wi=0.1,
                meas=at(512), prec=at(600), gate=9.0, xo=at(64), po=at(1024 + PM), nis=None, used=None, refused=None, innov=None, lost=None,
                points=at(4096), failed=at(7000))
    cases = layout_cases + [
        (dict(lay=Lay(obs_dim=0)), b"layout->obs_dim must be 1..12"), (dict(lay=Lay(obs_dim=13)), b"layout->obs_dim must be 1..12"),
        (dict(lay=Lay(cols=(0, nn, 1, 2))), b"layout->slot_col entries must be -1..n-1"),
        (dict(lay=Lay(cols=(0, 1, -2, 2))), b"layout->slot_col entries must be -1..n-1")] + count_cases + [
        (dict(q=None), b"null q_dev"), (dict(qd=None), b"null qd_dev"), (dict(pin=None), b"null p_in_dev"), (dict(Q=None), b"null q_host"),
        (dict(meas=None), b"null meas_dev"), (dict(prec=None), b"null prec_dev"), (dict(xo=None), b"null x_out_dev"), (dict(po=None), b"null p_out_dev"),
        (dict(points=None), b"failed_dev needs points_out_dev"),
        (dict(Q=q_with(1, 1, nan)), b"Q must be finite"), (dict(Q=q_with(0, 2, inf)), b"Q must be finite"),
        (dict(Q=q_with(0, 2, 0.5)), b"Q must be exactly symmetric"),
        (dict(gamma=nan), b"gamma must be finite"), (dict(gamma=-inf), b"gamma must be finite"), (dict(wm0=nan), b"wm0 must be finite"),
        (dict(wm0=inf), b"wm0 must be finite"), (dict(wc0=nan), b"wc0 must be finite"), (dict(wc0=-inf), b"wc0 must be finite"),
        (dict(wi=nan), b"wi must be finite"), (dict(wi=inf), b"wi must be finite"),
        (dict(gamma=0.0), b"gamma must be > 0"), (dict(gamma=-2.0), b"gamma must be > 0"), (dict(wi=0.0), b"wi must be > 0"), (dict(wi=-0.1), b"wi must be > 0"),
        (dict(gate=nan), b"gate must be finite"), (dict(gate=inf), b"gate must be finite"), (dict(gate=-0.5), b"gate must be >= 0"),
        (dict(gate=-5e-324), b"gate must be >= 0"),
        (dict(po=at(1024 + 1)), b"p_out_dev overlaps p_in_dev without being it"), (dict(po=at(1024 + PM - 1)), b"p_out_dev overlaps p_in_dev without being it"),
        (dict(po=at(1024 - PM + 1)), b"p_out_dev overlaps p_in_dev without being it"),
        (dict(points=at(2048)), b"points_out_dev overlaps q_dev"), (dict(points=at(2048 + HALF - 1)), b"points_out_dev overlaps q_dev"),
        (dict(points=at(2048 - NS + 1), qd=at(6000)), b"points_out_dev overlaps q_dev"),
        (dict(points=at(2048 + HALF)), b"points_out_dev overlaps qd_dev"), (dict(q=at(6000), points=at(2048 + HALF - NS + 1)), b"points_out_dev overlaps qd_dev"),
        (dict(M=2 ** 18, pin=top(65), po=top(33)), b"p_out_dev overlaps p_in_dev without being it"),
        (dict(M=2 ** 18, po=at(1024), q=top(65), points=top(33)), b"points_out_dev overlaps q_dev"),
        (dict(M=2 ** 18, po=at(1024), qd=top(65), points=top(33)), b"points_out_dev overlaps qd_dev")]
    edges = [dict(gate=0.0), dict(gate=-0.0), dict(gate=1.7e308), dict(wm0=-1e6, wc0=-1e6), dict(gamma=5e-324, wi=5e-324),
             dict(done=at(0)), dict(po=at(1024)), dict(lay=Lay(obs_dim=1)),
             dict(lay=Lay(cols=(-1,) * 12, obs_dim=12))]
    # (the last check refuses: a points_out_dev that ends one element into qd_dev; where the edge leaves out the points, its own
    # p_out_dev one element into p_in_dev is what refuses, which the loop below tells apart)
    fn = lib.os2ru_ukf_update
    no_points = dict(points=None, failed=None, po=at(1024 + 1))
    a = dict(good, **no_points)
    assert fn(*[a[k] for k in good], None) == abi.ERR_INVALID
    assert lib.os2ru_last_error() == b"os2ru_ukf_update: p_out_dev overlaps p_in_dev without being it"
    a = dict(good, lay=Lay(abi.F32), gate=1e300, points=at(2048 + HALF))      # (in fp32 the arrays are half as long)
    assert fn(*[a[k] for k in good], None) == abi.ERR_INVALID and lib.os2ru_last_error() == b"os2ru_ukf_update: points_out_dev overlaps qd_dev"
    run("os2ru_ukf_update", good, cases, edges, dict(points=at(2048 + HALF - NS + 1), q=at(6000)), b"points_out_dev overlaps qd_dev",
        ("layout_refusal", "slots_refusal"), 29, (dict(gate=nan), b"gate must be finite"))


def test_weights():
    from gym_os2r_amd import ukf
    for nn in (4, 6, 8, 10):
        assert ukf.weights(nn) == (math.sqrt(nn), 0.0, 2.0, 1.0 / (2 * nn))
    # (n + lambda = (1e-5 - 10) + 10 carries the rounding of 10, 2e-15 on 1e-5: 1e-10 relative on its root of 3e-3)
    g, wm0, wc0, wi = ukf.weights(10, alpha=1e-3, beta=2.0, kappa=0.0)
    assert wm0 < -9e5 and abs(wm0 + 20 * wi - 1.0) < 1e-9 and abs(g - 1e-3 * math.sqrt(10)) < 1e-12 and abs(wc0 - (wm0 + 3.0 - 1e-6)) < 1e-9
    g, wm0, wc0, wi = ukf.weights(6, kappa=-1.0)
    assert (g, wm0, wi) == (math.sqrt(5.0), -0.2, 0.1) and abs(wm0 + 12 * wi - 1.0) < 1e-15
    for kw in (dict(kappa=-10.0), dict(kappa=-11.0), dict(alpha=0.0), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(beta=float("nan")),
               dict(beta=float("inf")), dict(kappa=float("nan")), dict(kappa=float("inf")), dict(alpha="x"), dict(beta=None), dict(alpha=1e200),
               dict(alpha=1e-200)):
        with pytest.raises(ValueError, match="^ukf weights: "):
            ukf.weights(10, **kw)
    for nn in (0, -1, "x", None):
        with pytest.raises(ValueError, match="^ukf weights: "):
            ukf.weights(nn)
    assert "fp32" in ukf.weights.__doc__ and "1e-3" in ukf.weights.__doc__


# ---------------------------------------------------------------------------------------
# the Python layer, without a device
# ---------------------------------------------------------------------------------------
S = 2 * n + 1
LANES = S * M


def test_python_argument_errors_need_no_device(monkeypatch):
    import torch
    from gym_os2r_amd import ukf
    from gym_os2r_amd.sim import HipSim
    assert all(callable(getattr(HipSim, k)) for k in ("ukf_points", "ukf_points_into", "ukf_update", "ukf_update_into"))
    reached = []
    monkeypatch.setattr(ukf, "load", lambda: reached.append("ukf"))
    f64 = torch.float64
    s = _bare(f64)
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64)

    def refuses(method, what, *args, **kw):
        with pytest.raises(ValueError, match=f"^{what}: "):
            getattr(s, method)(*args, **kw)
    bad_weights = (dict(alpha=0.0), dict(kappa=-float(n)), dict(alpha=float("nan")), dict(beta=float("inf")), dict(kappa="x"))
    # ukf_points_into
    x, P, pts = z(n, M), z(n, n, M), z(n, LANES)
    good = (x, P, pts)
    for i in range(3):
        refuses("ukf_points_into", "ukf_points", *[None if j == i else t for j, t in enumerate(good)])
    for args in ((z(n + 1, M), P, pts), (z(n), P, pts), (z(n, 0), P, pts), (x.numpy(), P, pts), (x.float(), P, pts), (x, z(n, n, M + 1), pts),
                 (x, z(M, n, n).permute(1, 2, 0), pts), (x, P.float(), pts), (x, P, z(n, LANES + 1)), (x, P, z(n, LANES).float()),
                 (x, P, z(LANES, n).t()), (x, P, z(n, 2 * n * M))):
        refuses("ukf_points_into", "ukf_points", *args)
    for kw in (dict(failed=z(M)), dict(failed=i32(M + 1)), dict(failed=i64(M))) + bad_weights:
        refuses("ukf_points_into", "ukf_points", *good, **kw)
    # ukf_points
    Pv = z(n, n, M).permute(2, 0, 1)
    for args in ((None, Pv), (x, None), (z(n + 1, M), Pv), (z(n), Pv), (x, z(M + 1, n, n)), (x, P), (x.float(), Pv), (x, "x")):
        refuses("ukf_points", "ukf_points", *args)
    for kw in bad_weights:
        refuses("ukf_points", "ukf_points", x, Pv, **kw)
    # ukf_update_into
    q, qd, meas, prec, xo, Po = z(NQ, LANES), z(NQ, LANES), z(M, D), z(D), z(n, M), z(n, n, M)
    Q = torch.eye(n, dtype=f64)
    skew = Q.clone()
    skew[0, 1] = 0.5
    good = ((q, qd), P, meas, prec, xo, Po)
    for i in range(6):
        refuses("ukf_update_into", "ukf_update", *[None if j == i else t for j, t in enumerate(good)], Q=Q)
    for args in (((q,), P, meas, prec, xo, Po), (q, P, meas, prec, xo, Po), ((q, qd.numpy()), P, meas, prec, xo, Po), ((q, z(NQ, LANES + 1)), P, meas, prec, xo, Po),
                 ((z(NQ, LANES + 1), qd), P, meas, prec, xo, Po), ((z(NQ, S * (M + 1)), z(NQ, S * (M + 1))), P, meas, prec, xo, Po),
                 ((z(NQ, n * M), z(NQ, n * M)), P, meas, prec, xo, Po), ((z(NQ + 1, LANES), qd), P, meas, prec, xo, Po), ((q.float(), qd), P, meas, prec, xo, Po),
                 ((z(LANES, NQ).t(), qd), P, meas, prec, xo, Po), ((q, qd), z(n, n, M + 1), meas, prec, xo, Po), ((q, qd), P.float(), meas, prec, xo, Po),
                 ((q, qd), P, z(M, D + 1), prec, xo, Po), ((q, qd), P, z(D, M).t(), prec, xo, Po), ((q, qd), P, meas.float(), prec, xo, Po),
                 ((q, qd), P, z(M), prec, xo, Po), ((q, qd), P, meas, z(D + 1), xo, Po), ((q, qd), P, meas, prec.float(), xo, Po),
                 ((q, qd), P, meas, prec, z(n, M + 1), Po), ((q, qd), P, meas, prec, xo.float(), Po), ((q, qd), P, meas, prec, xo, z(n, n + 1, M)),
                 ((q, qd), P, meas, prec, xo, z(M, n, n).permute(1, 2, 0))):
        refuses("ukf_update_into", "ukf_update", *args, Q=Q)
    with pytest.raises(ValueError, match=f"^ukf_update: the {LANES + S} lanes of state .* are no multiple of points = {S}"):
        s.ukf_update_into((z(NQ, LANES + S), z(NQ, LANES + S)), P, meas, prec, xo, Po, Q=Q)
    for kw in (dict(Q=None), dict(Q=skew), dict(Q=skew.tolist()), dict(Q=Q * float("nan")), dict(Q=torch.eye(n + 1)), dict(Q="x"),
               dict(Q=Q, gate=-1.0), dict(Q=Q, gate=float("nan")), dict(Q=Q, gate=float("inf")), dict(Q=Q, gate="x"), dict(Q=Q, gate=True),
               dict(Q=Q, gate=None), dict(Q=Q, done=z(LANES)), dict(Q=Q, done=torch.zeros(LANES + 1, dtype=torch.uint8)),
               dict(Q=Q, done=torch.zeros(LANES, dtype=torch.bool)), dict(Q=Q, nis=z(M + 1)), dict(Q=Q, nis=z(M).float()), dict(Q=Q, used=z(M)),
               dict(Q=Q, used=i32(M + 1)), dict(Q=Q, used=i64(M)), dict(Q=Q, refused=z(M)), dict(Q=Q, refused=i64(M)), dict(Q=Q, innov=z(M, D + 1)),
               dict(Q=Q, innov=z(D, M).t()), dict(Q=Q, innov=z(M, D).float()), dict(Q=Q, lost=z(M)), dict(Q=Q, lost=i32(M + 1)), dict(Q=Q, lost=i64(M)),
               dict(Q=Q, points_out=z(n, LANES + 1)), dict(Q=Q, points_out=z(n, LANES).float()), dict(Q=Q, points_out=z(LANES, n).t()),
               dict(Q=Q, failed=i32(M)), dict(Q=Q, points_out=pts, failed=z(M)), dict(Q=Q, points_out=pts, failed=i32(M + 1))) \
            + tuple(dict(Q=Q, **kw) for kw in bad_weights):
        refuses("ukf_update_into", "ukf_update", *good, **kw)
    # ukf_update
    for args in ((None, Pv, meas, prec), ((q, qd), None, meas, prec), ((q, qd), Pv, None, prec), ((q, qd), Pv, meas, None), ((q, qd), z(M + 1, n, n), meas, prec),
                 ((q, qd), P, meas, prec), ((q, qd), Pv, z(M + 1, D), prec), ((q, qd), Pv, meas.float(), prec), ((q, qd), Pv, meas, z(D - 1)),
                 ((q, qd[:, :-1]), Pv, meas, prec), ((q.float(), qd.float()), Pv, meas, prec), (q, Pv, meas, prec)):
        refuses("ukf_update", "ukf_update", *args, Q=Q)
    for kw in (dict(Q=None), dict(Q=skew), dict(Q=Q * float("inf")), dict(Q=Q, gate=-1.0), dict(Q=Q, gate="x"), dict(Q=Q, gate=False),
               dict(Q=Q, done=z(LANES))) + tuple(dict(Q=Q, **kw) for kw in bad_weights):
        refuses("ukf_update", "ukf_update", (q, qd), Pv, meas, prec, **kw)
    assert reached == []                                                   # no check needed the library


POINTS_ORDER = ["layout", "M", "x", "P", "gamma", "points_out", "failed", "stream"]
UPDATE_ORDER = ["layout", "M", "q", "qd", "done", "P_in", "Q", "gamma", "wm0", "wc0", "wi", "meas", "prec", "gate", "x_out", "P_out", "nis", "used",
                "refused", "innov", "lost", "points_out", "failed", "stream"]


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_what_reaches_c_position_by_position(dt, monkeypatch):
    import torch
    from gym_os2r_amd import control, ukf
    dt = getattr(torch, dt)
    rec, stream = Recorder(), C.c_void_p(0)
    s = _bare(dt)
    s._control_layout = control.layout(abi.F64 if dt == torch.float64 else abi.F32, NQ, 0, [0, 1, 2, 3])
    s._stream = lambda: stream
    reached = []
    monkeypatch.setattr(ukf, "load", lambda: (reached.append("ukf"), rec)[1])
    z = lambda *shape, dtype=dt: torch.zeros(*shape, dtype=dtype)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    QV = torch.arange(float(n * n), dtype=torch.float64).reshape(n, n)
    QV = QV + QV.T + 40.0 * torch.eye(n, dtype=torch.float64)
    default, other = ukf.weights(n), ukf.weights(n, alpha=0.5, beta=1.5, kappa=1.0)

    def held(entry, order, kw, **special):
        name, args = rec.calls[-1]
        assert name == entry and len(args) == len(ukf.ENTRY_POINTS[name]) == len(order)
        for i, (what, got) in enumerate(zip(order, args)):
            where = f"{entry}, argument {i} ({what})"
            if what == "stream":
                assert got is stream, where
            elif what == "layout":
                assert _decode(got) is s._control_layout, where
            elif what in special:
                assert _decode(got) == special[what] and type(_decode(got)) is type(special[what]), where
            else:
                assert _decode(got) == (None if kw.get(what) is None else kw[what].data_ptr()), where

    def scalars(w, gate=None):
        out = dict(gamma=w[0], wm0=w[1], wc0=w[2], wi=w[3])
        return out if gate is None else dict(out, gate=gate)
    # the points
    kw = dict(x=z(n, M), P=z(n, n, M), points_out=z(n, LANES), failed=i32(M))
    s.ukf_points_into(**kw, alpha=0.5, beta=1.5, kappa=1.0)
    held("os2ru_ukf_points", POINTS_ORDER, kw, M=M, gamma=other[0])
    bare = dict(kw, failed=None)
    s.ukf_points_into(**bare)
    held("os2ru_ukf_points", POINTS_ORDER, bare, M=M, gamma=default[0])
    # the update
    q, qd = z(NQ, LANES), z(NQ, LANES)
    kw = dict(P_in=z(n, n, M), meas=z(M, D), prec=z(D), x_out=z(n, M), P_out=z(n, n, M), done=torch.zeros(LANES, dtype=torch.uint8), nis=z(M),
              used=i32(M), refused=i32(M), innov=z(M, D), lost=i32(M), points_out=z(n, LANES), failed=i32(M))
    ptrs = [v.data_ptr() for v in list(kw.values()) + [q, qd]]
    assert len(set(ptrs)) == len(ptrs)
    s.ukf_update_into((q, qd), **kw, Q=QV, gate=9.5, alpha=0.5, beta=1.5, kappa=1.0)
    held("os2ru_ukf_update", UPDATE_ORDER, dict(kw, q=q, qd=qd), M=M, Q=QV.reshape(-1).tolist(), **scalars(other, 9.5))
    bare = dict(P_in=kw["P_in"], meas=kw["meas"], prec=kw["prec"], x_out=kw["x_out"], P_out=kw["P_in"])
    s.ukf_update_into((q, qd), **bare, Q=QV)
    held("os2ru_ukf_update", UPDATE_ORDER, dict(bare, q=q, qd=qd), M=M, Q=QV.reshape(-1).tolist(), **scalars(default, 0.0))
    assert reached == ["ukf"] * 4

    # the allocating forms: the state pair and the P an earlier call returned go on without a copy, the two P buffers alternate
    seen, real = [], type(s).ukf_update_into

    def spy(self, *args, **kwargs):
        names = ("state", "P_in", "meas", "prec", "x_out", "P_out")
        seen.append(dict(zip(names, args), **kwargs))
        return real(self, *args, **kwargs)
    monkeypatch.setattr(type(s), "ukf_update_into", spy)
    same = lambda a, b: a.data_ptr() == b.data_ptr()
    P0 = torch.eye(n, dtype=dt).repeat(M, 1, 1)                             # no view of the kernel's layout: converted and copied
    meas, prec, done = z(M, D), z(D), torch.zeros(LANES, dtype=torch.uint8)
    x1, P1, nis, used, refused, innov, lost, points, failed = s.ukf_update((q, qd), P0, meas, prec, Q=QV, done=done, gate=9.5, want_innov=True)
    first = seen[0]
    assert first["state"][0] is q and first["state"][1] is qd and first["meas"] is meas and first["prec"] is prec and first["done"] is done
    assert not same(first["P_in"], P0) and torch.equal(first["P_in"], P0.permute(1, 2, 0)) and first["P_in"].is_contiguous()
    for name, shape in (("P_in", (n, n, M)), ("x_out", (n, M)), ("P_out", (n, n, M)), ("nis", (M,)), ("innov", (M, D)), ("points_out", (n, LANES))):
        assert tuple(first[name].shape) == shape and first[name].is_contiguous() and first[name].dtype == dt, name
    for name in ("used", "refused", "lost", "failed"):
        assert first[name].dtype == torch.int32 and tuple(first[name].shape) == (M,), name
    held("os2ru_ukf_update", UPDATE_ORDER, dict(first, q=q, qd=qd), M=M, Q=QV.reshape(-1).tolist(), **scalars(default, 9.5))
    assert tuple(x1.shape) == (n, M) and tuple(P1.shape) == (M, n, n) and same(P1, first["P_out"]) and x1 is first["x_out"]
    assert points is first["points_out"] and failed is first["failed"] and lost is first["lost"] and innov is first["innov"]
    assert all(tuple(t.shape) == (M,) for t in (nis, used, refused, lost, failed))
    x2, P2, *_ = s.ukf_update((q, qd), P1, meas, prec, Q=QV)
    *_, no_innov, _, no_points, no_failed = s.ukf_update((q, qd), P2, meas, prec, Q=QV, want_points=False, kappa=1.0)
    P3 = seen[2]["P_out"].permute(2, 0, 1)
    assert same(seen[1]["P_in"], P1) and same(seen[2]["P_in"], P2) and not same(P1, P2) and same(P3, P1)
    assert no_innov is None and no_points is None and no_failed is None and seen[2]["points_out"] is None and seen[2]["failed"] is None
    assert seen[1]["done"] is None and seen[1]["gate"] == 0.0 and seen[1]["innov"] is None and seen[1]["points_out"] is not None
    held("os2ru_ukf_update", UPDATE_ORDER, dict(seen[2], q=q, qd=qd), M=M, Q=QV.reshape(-1).tolist(), **scalars(ukf.weights(n, kappa=1.0), 0.0))
    # ukf_points: the P ukf_update returned goes on without a copy, x as it is; anything else is copied once
    seen_p, real_p = [], type(s).ukf_points_into

    def spy_p(self, *args, **kwargs):
        seen_p.append(dict(zip(("x", "P", "points_out"), args), **kwargs))
        return real_p(self, *args, **kwargs)
    monkeypatch.setattr(type(s), "ukf_points_into", spy_p)
    pts, fl = s.ukf_points(x1, P1, alpha=0.5, beta=1.5, kappa=1.0)
    assert seen_p[0]["x"] is x1 and same(seen_p[0]["P"], P1) and tuple(seen_p[0]["P"].shape) == (n, n, M) and seen_p[0]["P"].is_contiguous()
    assert pts is seen_p[0]["points_out"] and tuple(pts.shape) == (n, LANES) and fl.dtype == torch.int32 and tuple(fl.shape) == (M,)
    held("os2ru_ukf_points", POINTS_ORDER, seen_p[0], M=M, gamma=other[0])
    pts, fl = s.ukf_points(x1, P0, want_failed=False)
    assert fl is None and not same(seen_p[1]["P"], P0) and torch.equal(seen_p[1]["P"], P0.permute(1, 2, 0))
    assert tuple(pts[:NQ].shape) == tuple(pts[NQ:].shape) == (NQ, LANES) and pts[:NQ].is_contiguous() and pts[NQ:].is_contiguous()
