"""libos2r_ekf.so (include/os2r_ekf.h): the host side -- the numpy restatement of the update the GPU tests compare with
(`restate_ekf`) on crafted inputs that reach every branch of it (`crafted_ekf`), the restatement against the textbook joint
update, its exact properties, the header against the one table of gym_os2r_amd/ekf.py, the exports of the library, the other
seven libraries as they were, the resources of the eight kernels in the built library, every refusal of os2re_ekf_update through
ctypes without a device, the argument checks of HipSim.ekf_update that need no device and what the two methods pass to C.
No GPU needed."""
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
from header_check import _agrees, _header, _is_pointer, _prototypes, checks_before_the_device  # noqa: E402

NAMES = ["os2re_abi_version", "os2re_last_error", "os2re_ekf_update"]
MAX_OBS = 12
ROBOTS = 32                              # robots of one workgroup (kEkfRobots)
GATE = 9.0
CLASSES = ("generic", "one NaN reading", "every reading NaN", "one reading gated", "negative variance", "infinite variance",
           "garbage below the diagonal", "huge innovation")
BRANCH_SHAPE = (67, 5, 10)               # M, nq, D: three workgroups with a tail


# ---------------------------------------------------------------------------------------
# the restatement of include/os2r_ekf.h (needs no device)
# ---------------------------------------------------------------------------------------
def _dot(x, y, dtype):
    """sum_l x[l] y[l] as ((x0 y0 + x1 y1) + x2 y2) + ..., every product and sum rounded on its own; x, y [n, ...]."""
    acc = x[0] * y[0]
    for l in range(1, len(x)):
        acc = acc + x[l] * y[l]
    assert acc.dtype == dtype
    return acc


def restate_ekf(x_pred, p_in, meas, prec, slot_col, *, a=None, q=None, gate=0.0, dtype, trace=None):
    """include/os2r_ekf.h, steps 1-3, in numpy and in `dtype`, every robot at once: x_pred [n, M], p_in [n, n, M], a [n, n, M] or
    None, q [n, n] or None, meas [M, D], prec [D].  trace: a list that is given (d, applied [M], diagonal before [n, M], diagonal
    after [n, M]) per slot that was looked at.  -> dict(x [n, M], p [n, n, M], nis [M], used [M] int32, refused [M] int32,
    innov [M, D], p_minus [n, n, M])."""
    x = np.array(x_pred, dtype)
    n, M = x.shape
    pin = np.array(p_in, dtype)
    y_all = np.array(meas, dtype)
    D = y_all.shape[1]
    pr_all = np.array(prec, dtype)
    gate = dtype(gate)
    P = np.empty((n, n, M), dtype)
    for i in range(n):
        for j in range(i, n):
            P[i, j] = P[j, i] = pin[i, j]
    with np.errstate(all="ignore"):
        if a is not None:
            A, Q = np.array(a, dtype), np.array(q, dtype)
            AP = np.empty_like(P)
            for i in range(n):
                for j in range(n):
                    AP[i, j] = _dot(A[i], P[:, j], dtype)
            for i in range(n):
                for j in range(i, n):
                    P[i, j] = P[j, i] = Q[i, j] + _dot(AP[i], A[j], dtype)
        p_minus = P.copy()
        nis = np.zeros(M, dtype)
        used, refused = np.zeros(M, np.int32), np.zeros(M, np.int32)
        innov = np.zeros((M, D), dtype)
        for d in range(D):
            c = int(slot_col[d])
            pr = pr_all[d]
            if c < 0 or not (np.isfinite(pr) and pr > 0):
                continue
            y = y_all[:, d]
            look = np.isfinite(y)
            r = dtype(1) / pr
            s = P[c, c] + r
            s_ok = np.isfinite(s) & (s > 0)
            v = y - x[c]
            z = (v * v) / s
            z_ok = np.isfinite(z)
            refuse = look & ~(s_ok & z_ok)
            gated = (z > gate) if gate > 0 else np.zeros(M, bool)
            apply = look & s_ok & z_ok & ~gated
            k = P[:, c] / s[None]
            row = P[c].copy()
            before = np.array([P[i, i] for i in range(n)])
            x = np.where(apply[None], x + k * v[None], x)
            for i in range(n):
                for j in range(i, n):
                    P[i, j] = P[j, i] = np.where(apply, P[i, j] - k[i] * row[j], P[i, j])
            nis = np.where(apply, nis + z, nis)
            used |= np.where(apply, 1 << d, 0).astype(np.int32)
            refused |= np.where(refuse, 1 << d, 0).astype(np.int32)
            innov[:, d] = np.where(apply, v, 0)
            assert all(t.dtype == dtype for t in (r, s, v, z, k, x, P, nis))
            if trace is not None:
                trace.append((d, apply, before, np.array([P[i, i] for i in range(n)])))
    return dict(x=x, p=P, nis=nis, used=used, refused=refused, innov=innov, p_minus=p_minus)


def slot_columns(n, D, seed=0):
    """The state column of every slot: a permutation of the columns, repeated where D > n; slot 1 carries none (-1) where D >= 3,
    slot D - 2 none where D >= 6, and the last slot shows the column of slot 0 again where D >= 2."""
    rng = np.random.default_rng(100 + seed)
    cols = [int(v) for v in np.concatenate([rng.permutation(n) for _ in range(-(-D // n))])[:D]]
    if D >= 3:
        cols[1] = -1
    if D >= 6:
        cols[D - 2] = -1
    if D >= 2:
        cols[D - 1] = cols[0]
    return cols


def crafted_ekf(M, nq, D, seed=0, dtype=np.float64, variant=0):
    """Inputs in float64 (the caller rounds) whose robot classes m % 8 (CLASSES) reach every branch.  P is well conditioned
    (0.05 I plus a random Gram matrix of that size), A is I + 0.05 N(0, 1), Q = 0.01 (I + a Gram matrix), prec in 50..200 with the
    entry of slot 2 equal to 0 where D >= 4 (variant 1: NaN), every reading lies 0.7 standard deviations of its innovation about
    the predicted state, and d0 is slot 0, c0 its column:
      0  generic
      1  the reading of d0 is NaN
      2  every reading is NaN: x_out is x_pred and p_out is P-
      3  the reading of d0 lies 30 standard deviations away: gated at GATE, applied at gate 0
      4  P[c0][c0] = -5: d0 is refused, the slots after it are applied
      5  P[c0][c0] = +inf: s is not finite
      6  NaN below the diagonal of p_in, which is never read
      7  the reading of d0 is so far that z overflows: refused
    -> dict(x_pred [n, M], p_in [n, n, M], a [n, n, M], q [n, n], meas [M, D], prec [D], slot_col [D])"""
    rng = np.random.default_rng(seed)
    n = 2 * nq
    cols = slot_columns(n, D, seed)
    x_pred = rng.uniform(-1.0, 1.0, (n, M))
    G = rng.normal(0.0, 1.0, (M, n, n))
    P = 0.05 * np.eye(n)[None] + 0.05 / n * G @ G.transpose(0, 2, 1)
    P = 0.5 * (P + P.transpose(0, 2, 1))
    A = np.eye(n)[None] + 0.05 * rng.normal(0.0, 1.0, (M, n, n))
    Gq = rng.normal(0.0, 1.0, (n, n))
    Q = 0.01 * (np.eye(n) + Gq @ Gq.T / n)
    Q = 0.5 * (Q + Q.T)
    prec = rng.uniform(50.0, 200.0, D)
    if D >= 4:
        prec[2] = np.nan if variant else 0.0
    meas = np.empty((M, D))
    for d, c in enumerate(cols):
        sd = np.sqrt(P[:, max(c, 0), max(c, 0)] + 1.0 / np.where(prec[d] > 0, prec[d], 1.0))
        meas[:, d] = x_pred[max(c, 0)] + 0.7 * sd * rng.normal(0.0, 1.0, M)
    m = np.arange(M)
    cls = m % 8
    c0 = cols[0]
    sd0 = np.sqrt(P[:, c0, c0] + 1.0 / prec[0])
    meas[cls == 1, 0] = np.nan
    meas[cls == 2] = np.nan
    meas[cls == 3, 0] = x_pred[c0, cls == 3] + 30.0 * sd0[cls == 3]
    P[cls == 4, c0, c0] = -5.0
    P[cls == 5, c0, c0] = np.inf
    meas[cls == 7, 0] = 1e200 if dtype == np.float64 else 1e30
    p_in = np.ascontiguousarray(P.transpose(1, 2, 0))
    for i in range(n):
        p_in[i, :i, cls == 6] = np.nan
    return dict(x_pred=x_pred, p_in=p_in, a=np.ascontiguousarray(A.transpose(1, 2, 0)), q=Q, meas=meas, prec=prec, slot_col=cols)


def _restated(c, dtype, gate=GATE, predict=True, trace=None):
    return restate_ekf(c["x_pred"], c["p_in"], c["meas"], c["prec"], c["slot_col"], a=c["a"] if predict else None,
                       q=c["q"] if predict else None, gate=gate, dtype=dtype, trace=trace)


def same_bits(got, want):
    """Two float arrays are the same bit for bit, +0 and -0 as one and a NaN as a NaN (neither the sign of a zero nor the sign
    and payload of a NaN are part of the contract)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    bits = np.uint64 if got.dtype == np.float64 else np.uint32
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    g, w = np.where((got == 0) | nan, 0, got).astype(got.dtype), np.where((want == 0) | nan, 0, want).astype(want.dtype)
    return np.array_equal(g.view(bits), w.view(bits))


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_on_crafted_inputs_that_reach_every_branch(dtype, variant):
    M, nq, D = BRANCH_SHAPE
    n = 2 * nq
    c = crafted_ekf(M, nq, D, dtype=dtype, variant=variant)
    cols = c["slot_col"]
    assert M > 2 * ROBOTS and M % ROBOTS and cols.count(-1) == 2 and cols[D - 1] == cols[0] and D >= 4
    assert (np.isnan(c["prec"][2]) if variant else c["prec"][2] == 0) and MAX_OBS == abi.MAX_OBS
    cls = np.arange(M) % 8
    live = np.array([d for d in range(D) if cols[d] >= 0 and d != 2])                  # the slots that are looked at
    all_bits = int(sum(1 << d for d in live))
    for predict in (True, False):
        out, free = _restated(c, dtype, GATE, predict), _restated(c, dtype, 0.0, predict)
        used, refused = out["used"], out["refused"]
        assert not (used & ~all_bits).any() and not (refused & ~all_bits).any()         # a dropped slot sets neither bit
        # generic: nothing refused, and without a gate every live slot applied
        assert (refused[cls == 0] == 0).all() and (free["used"][cls == 0] == all_bits).all()
        # one NaN reading: that slot alone is missing
        assert (free["used"][cls == 1] == all_bits & ~1).all() and (refused[cls == 1] == 0).all()
        # every reading NaN: x_out is x_pred and p_out is P-, bit for bit
        lost = cls == 2
        assert (used[lost] == 0).all() and (refused[lost] == 0).all() and (out["nis"][lost] == 0).all()
        assert np.array_equal(out["x"][:, lost], c["x_pred"].astype(dtype)[:, lost])
        assert np.array_equal(out["p"][:, :, lost], out["p_minus"][:, :, lost])
        # gated at GATE, applied without a gate; neither bit where gated
        far = cls == 3
        assert (used[far] & 1 == 0).all() and (refused[far] & 1 == 0).all() and (free["used"][far] & 1 == 1).all()
        assert (free["nis"][far] > GATE).all() and (out["innov"][far, 0] == 0).all() and (free["innov"][far, 0] != 0).all()
        # a negative variance: the slot is refused, the slots after it are applied
        neg = cls == 4
        assert (refused[neg] & 1 == 1).all() and (used[neg] & 1 == 0).all() and (used[neg] != 0).all()
        assert (free["used"][neg] | free["refused"][neg] == all_bits).all()
        # an infinite variance: s is not finite
        inf = cls == 5
        assert (refused[inf] & 1 == 1).all() and (used[inf] & 1 == 0).all()
        # z overflows: refused
        huge = cls == 7
        assert (refused[huge] & 1 == 1).all() and (used[huge] & 1 == 0).all() and (used[huge] != 0).all()
        # what lies below the diagonal of p_in is never read
        clean = dict(c, p_in=np.where(np.isnan(c["p_in"]), 0.0, c["p_in"]))
        again = _restated(clean, dtype, GATE, predict)
        assert np.isnan(c["p_in"][:, :, cls == 6]).any() and all(np.array_equal(again[k], out[k], equal_nan=True) for k in out)
        assert np.isfinite(out["p"][:, :, cls != 5]).all() and np.isfinite(out["x"]).all()
        assert out["x"].dtype == dtype and out["p"].dtype == dtype and out["nis"].dtype == dtype and out["innov"].dtype == dtype


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exact_properties_on_every_robot(dtype):
    """p_out is bitwise symmetric, no diagonal entry of P rises across an applied slot, no slot is both used and refused, and
    innov is 0 outside used."""
    M, nq, D = BRANCH_SHAPE
    n = 2 * nq
    for variant, gate, predict in ((0, GATE, True), (1, 0.0, True), (0, GATE, False), (1, 0.0, False)):
        c = crafted_ekf(M, nq, D, dtype=dtype, variant=variant)
        trace = []
        out = _restated(c, dtype, gate, predict, trace)
        assert same_bits(out["p"], out["p"].transpose(1, 0, 2))
        assert trace and any(apply.any() for _, apply, _, _ in trace)
        for d, apply, before, after in trace:
            assert not (after > before)[:, apply].any(), d
            assert same_bits(after[:, ~apply], before[:, ~apply]), d
        assert (out["used"] & out["refused"] == 0).all()
        off = (out["used"][:, None] >> np.arange(D)[None]) & 1 == 0
        assert (out["innov"][off] == 0).all() and (out["innov"][~off] != 0).any()


# 100 x the worst distances measured for these very inputs on the CPU: float64 4.3e-16 (P), 6.7e-16 (x), 2.5e-15 (nis);
# float32 4.5e-7, 1.6e-7, 9.1e-7
TEXTBOOK_BOUNDS = {np.float64: (4.3e-14, 6.7e-14, 2.5e-13), np.float32: (4.5e-5, 1.6e-5, 9.1e-5)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_sequence_of_scalar_updates_is_the_joint_update_of_the_textbook(dtype):
    """The generic robots, gate 0: the restatement in `dtype` against K = P- H'(H P- H' + R)^-1, x + K (y - H x), (I - K H) P- and
    nu' S^-1 nu in float64 from the same (rounded) inputs.  The distance in P is relative to the largest entry of the robot's P,
    the one in nis relative to nis, the one in x absolute (the states are of order 1)."""
    worst = np.zeros(3)
    for nq, D, seed in ((2, 3, 1), (3, 6, 2), (4, 8, 3), (5, 10, 4), (5, 12, 5)):
        M, n = 64, 2 * nq
        c = crafted_ekf(M, nq, D, seed=seed, dtype=dtype)
        out = _restated(c, dtype, 0.0, True)
        r64 = lambda k: np.asarray(c[k]).astype(dtype).astype(np.float64)
        live = [d for d in range(D) if c["slot_col"][d] >= 0 and r64("prec")[d] > 0]
        H = np.zeros((len(live), n))
        H[np.arange(len(live)), [c["slot_col"][d] for d in live]] = 1.0
        R = np.diag(1.0 / r64("prec")[live])
        for m in range(0, M, 8):                                                      # the generic robots
            A, P = r64("a")[:, :, m], np.triu(r64("p_in")[:, :, m])
            P = P + np.triu(P, 1).T
            Pm = A @ P @ A.T + r64("q")
            nu = r64("meas")[m, live] - H @ r64("x_pred")[:, m]
            S = H @ Pm @ H.T + R
            K = np.linalg.solve(S, H @ Pm).T
            x, Pp, nis = r64("x_pred")[:, m] + K @ nu, (np.eye(n) - K @ H) @ Pm, nu @ np.linalg.solve(S, nu)
            assert out["used"][m] == sum(1 << d for d in live) and out["refused"][m] == 0
            dist = (np.abs(out["p"][:, :, m] - Pp).max() / np.abs(Pp).max(), np.abs(out["x"][:, m] - x).max(), abs(out["nis"][m] - nis) / nis)
            worst = np.maximum(worst, dist)
    print(f"ekf against the textbook, {dtype.__name__}: worst relative distance in P {worst[0]:.3g}, in x {worst[1]:.3g}, in nis {worst[2]:.3g}")
    assert (worst <= TEXTBOOK_BOUNDS[dtype]).all(), worst


# ---------------------------------------------------------------------------------------
# header, table, exports
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import control, ekf
    protos = _prototypes("os2r_ekf.h", "os2re")
    assert [p[0] for p in protos] == list(ekf.ENTRY_POINTS) == NAMES
    lib = ekf.load()
    for name, ret, args in protos:
        argtypes = ekf.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2re_last_error" else C.c_int)
    args = protos[2][2]
    assert args[0] == "const Os2rControlLayout* layout" and args[1] == "int64_t nrobots" and args[5] == "const double* q_host"
    assert args[8] == "double gate" and args[12] == "int32_t* used_dev" and args[13] == "int32_t* refused_dev"
    assert args[-1] == "void* stream" and len(args) == 16
    table = ekf.ENTRY_POINTS["os2re_ekf_update"]
    assert table[8] is C.c_double and table[1] is C.c_int64 and table[5] is C.POINTER(C.c_double)
    header = _header("os2r_ekf.h")
    assert re.search(r"#define OS2R_EKF_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert lib.os2re_abi_version() == ekf.ABI_VERSION == 1
    assert ekf.Os2rControlLayout is control.Os2rControlLayout and ekf.layout is control.layout and ekf.MAX_OBS == MAX_OBS
    assert issubclass(ekf.Os2rEkfLibraryMissing, ImportError)
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", ekf.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)


def test_the_other_libraries_are_as_they_were():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib, control, ekf, mppi, pf, search, steer
    tables = {_lib.LIB_PATH: _lib.ENTRY_POINTS, _lib.RECORD_LIB_PATH: _lib.RECORD_ENTRY_POINTS, control.LIB_PATH: control.ENTRY_POINTS,
              search.LIB_PATH: search.ENTRY_POINTS, steer.LIB_PATH: steer.ENTRY_POINTS, mppi.LIB_PATH: mppi.ENTRY_POINTS,
              pf.LIB_PATH: pf.ENTRY_POINTS}
    others = set().union(*tables.values())
    assert len(tables) == 7 and not set(ekf.ENTRY_POINTS) & others and not any(name.startswith("os2re_") for name in others)
    for name in ("os2r.h", "os2r_control.h", "os2r_record.h", "os2r_search.h", "os2r_steer.h", "os2r_mppi.h", "os2r_pf.h"):
        assert "os2re_" not in _header(name) and "os2r_ekf" not in _header(name).lower(), name
    assert len(_lib.ENTRY_POINTS) == 35 and len(_lib.RECORD_ENTRY_POINTS) == 3
    assert list(control.ENTRY_POINTS) == ["os2rc_abi_version", "os2rc_last_error", "os2rc_ilqr_backward"]
    assert list(search.ENTRY_POINTS) == ["os2rs_abi_version", "os2rs_last_error", "os2rs_ilqr_line_search"]
    assert list(steer.ENTRY_POINTS) == ["os2rt_abi_version", "os2rt_last_error", "os2rt_ilqr_backward_mu", "os2rt_ilqr_steer"]
    assert list(mppi.ENTRY_POINTS) == ["os2rm_abi_version", "os2rm_last_error", "os2rm_mppi_update"]
    assert list(pf.ENTRY_POINTS) == ["os2rp_abi_version", "os2rp_last_error", "os2rp_pf_update"]
    for path, table in tables.items():
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(table), path
        kernels = kernel_meta.kernel_meta(path)
        assert kernels and not any("ekf" in k.lower() for k in kernels), path
    # ... and the new library holds none of theirs
    forbidden = ("pf_update", "mppi", "steer", "_mu_kernel", "line_search", "record", "ilqr_backward_kernel", "lqr_gains_kernel<")
    assert not any(word in k for k in kernel_meta.kernel_meta(ekf.LIB_PATH) for word in forbidden)


def lds_bound(n, size):
    """The bound the header comment of csrc/os2r_ekf.hpp states: one n x n matrix, x, k, the measurements of 32 robots, r, Q and
    the twelve drop flags."""
    return ((n * n + 2 * n + MAX_OBS) * ROBOTS + n * n + MAX_OBS) * size + MAX_OBS * 4


def test_kernel_resources():
    """Exactly eight kernels, float and double for chains of 2..5 dofs, are in the built library and none uses scratch:
    private_segment_fixed_size 0, no VGPR or SGPR spill and no AGPRs in the code-object metadata.  The static LDS is within the
    bound the header comment states -- 34736 bytes for double and nq = 5, of which four fit the 160 KiB of a CU --, every kernel
    leaves room for four waves on a SIMD (at most 128 registers), and there is no dynamic LDS: the launch passes 0."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import ekf
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(ekf.LIB_PATH)
    meta = kernel_meta.kernel_meta(ekf.LIB_PATH)
    assert len(meta) == 8, sorted(meta)
    src = open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "os2r_ekf.hpp")).read()
    assert "((n n + 2 n + 12) 32 + n n + 12) sizeof(T) + 12 * 4 bytes -- 34736 for double and nq = 5" in src
    assert lds_bound(10, 8) == 34736 and 4 * lds_bound(10, 8) <= 160 * 1024
    assert re.search(r"constexpr int kEkfRobots = (\d+);", src).group(1) == str(ROBOTS)
    for real, size in (("float", 4), ("double", 8)):
        for nq in (2, 3, 4, 5):
            (name,) = [k for k in meta if f"ekf_update_kernel<{real}, {nq}>" in k]
            m = meta[name]
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
            assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 128, (name, m)
            assert 0 < m["group_segment_fixed_size"] <= lds_bound(2 * nq, size), (name, m)
    inst = open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "os2r_ekf_inst.hip")).read()
    assert "hipLaunchKernelGGL((ekf_update_kernel<T, NQ>), grid, block, 0, s, p)" in inst      # no dynamic LDS
    assert "by_chain_length(nq," in inst


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def test_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import control, ekf
    lib = ekf.load()
    M, nq = 4, 3
    n = 2 * nq
    buf = (C.c_double * 4096)()
    base = C.addressof(buf)
    at = lambda i: C.c_void_p(base + 8 * i)
    nan, inf = float("nan"), float("inf")
    eye = [1.0 if i == j else 0.0 for i in range(n) for j in range(n)]
    dbl = lambda values: (C.c_double * len(values))(*values)

    def Lay(dtype=abi.F64, cols=(0, 1, 3, -1), **kw):
        lay = control.layout(dtype, nq, 0, list(cols))
        for k, v in kw.items():
            setattr(lay, k, v)
        return C.byref(lay)

    def q_with(i, j, value):
        q = list(eye)
        q[i * n + j] = value
        return dbl(q)
    X, PM = n * M, n * n * M
    good = dict(lay=Lay(), M=M, xp=at(0), pin=at(1024), a=at(2048), q=dbl(eye), meas=at(512), prec=at(600), gate=9.0, xo=at(64),
                po=at(1024 + PM), nis=None, used=None, refused=None, innov=None)
    name = "os2re_ekf_update"
    assert len(good) + 1 == len(ekf.ENTRY_POINTS[name]) == 16

    def call(**kw):
        a = dict(good, **kw)
        return lib.os2re_ekf_update(*[a[k] for k in good], None)
    assert lib.os2re_ekf_update(*[None if _is_pointer(t) else 0 for t in ekf.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2re_last_error() == b"os2re_ekf_update: null layout"
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"layout->dtype must be OS2R_F32 or OS2R_F64"),
             (dict(lay=Lay(nq=1)), b"layout->nq must be 2..5"), (dict(lay=Lay(nq=6)), b"layout->nq must be 2..5"),
             (dict(lay=Lay(obs_dim=0)), b"layout->obs_dim must be 1..12"), (dict(lay=Lay(obs_dim=13)), b"layout->obs_dim must be 1..12"),
             (dict(lay=Lay(cols=(0, n, 1, 2))), b"layout->slot_col entries must be -1..n-1"),
             (dict(lay=Lay(cols=(0, 1, -2, 2))), b"layout->slot_col entries must be -1..n-1"),
             (dict(M=0), b"nrobots must be >= 1"), (dict(M=-1), b"nrobots must be >= 1"),
             (dict(M=2 ** 62), b"n * n * nrobots exceeds 2^31 - 1"), (dict(M=(2 ** 31 - 1) // (n * n) + 1), b"n * n * nrobots exceeds 2^31 - 1"),
             (dict(xp=None), b"null x_pred_dev"), (dict(pin=None), b"null p_in_dev"), (dict(meas=None), b"null meas_dev"),
             (dict(prec=None), b"null prec_dev"), (dict(xo=None), b"null x_out_dev"), (dict(po=None), b"null p_out_dev"),
             (dict(q=None), b"a_dev needs q_host"),
             (dict(q=q_with(1, 1, nan)), b"Q must be finite"), (dict(q=q_with(0, 2, inf)), b"Q must be finite"),
             (dict(q=q_with(0, 2, 0.5)), b"Q must be exactly symmetric"),
             (dict(gate=nan), b"gate must be finite"), (dict(gate=inf), b"gate must be finite"), (dict(gate=-inf), b"gate must be finite"),
             (dict(gate=-0.5), b"gate must be >= 0"), (dict(gate=-5e-324), b"gate must be >= 0"),
             (dict(xo=at(1)), b"x_out_dev overlaps x_pred_dev without being it"),
             (dict(xo=at(X - 1)), b"x_out_dev overlaps x_pred_dev without being it"),
             (dict(xp=at(X - 1), xo=at(0)), b"x_out_dev overlaps x_pred_dev without being it"),
             (dict(po=at(1024 + 1)), b"p_out_dev overlaps p_in_dev without being it"),
             (dict(po=at(1024 + PM - 1)), b"p_out_dev overlaps p_in_dev without being it"),
             (dict(po=at(1024 - PM + 1)), b"p_out_dev overlaps p_in_dev without being it"),
             # (arrays whose ends wrap round at the top of the address space: the check is on the distance)
             (dict(M=2 ** 20, xp=C.c_void_p(2 ** 64 - 65), xo=C.c_void_p(2 ** 64 - 33)), b"x_out_dev overlaps x_pred_dev without being it"),
             (dict(M=2 ** 20, xo=at(0), pin=C.c_void_p(2 ** 64 - 65), po=C.c_void_p(2 ** 64 - 33)), b"p_out_dev overlaps p_in_dev without being it")]
    seen = set()
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.os2re_last_error()
        assert rc == abi.ERR_INVALID and err == b"os2re_ekf_update: " + msg, (kw.keys(), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases}) == 20                  # each cause has a text of its own
    assert not any(buf)                                                   # a refused call wrote nothing
    # the edges are taken: the next refusal is about something else (no call here is let through to a device).  The last check
    # refuses: a p_out_dev one element into p_in_dev
    last = b"os2re_ekf_update: p_out_dev overlaps p_in_dev without being it"
    edges = [dict(gate=0.0), dict(gate=-0.0), dict(gate=1.7e308), dict(dtype=abi.F32, gate=1e300), dict(a=None, q=None), dict(a=None),
             dict(xo=at(0)), dict(xo=at(X)), dict(xp=at(X), xo=at(0)), dict(lay=Lay(obs_dim=1)), dict(lay=Lay(cols=(-1,) * 12, obs_dim=12)),
             dict(lay=Lay(cols=(n - 1, 0, 0, -1))), dict(M=(2 ** 31 - 1) // (n * n), xo=at(0))]
    for kw in edges:
        if "dtype" in kw:
            kw = dict(kw, lay=Lay(kw.pop("dtype")))
        assert call(**dict(kw, po=at(1024 + 1))) == abi.ERR_INVALID and lib.os2re_last_error() == last, kw
    # nrobots at the int32 limit: nq = 2 and n n nrobots = 2^31 - 16; and equal pointers for P
    big = dict(lay=Lay(nq=2, cols=(0, 1, 3, -1)), M=(2 ** 31 - 1) // 16, a=None, q=None, xo=at(0), po=at(1024))
    assert call(**dict(big, gate=nan)) == abi.ERR_INVALID and lib.os2re_last_error() == b"os2re_ekf_update: gate must be finite"
    assert call(po=at(1024), xo=at(0), gate=-1.0) == abi.ERR_INVALID and lib.os2re_last_error() == b"os2re_ekf_update: gate must be >= 0"
    assert call(po=at(1024 - PM), gate=-1.0) == abi.ERR_INVALID and lib.os2re_last_error() == b"os2re_ekf_update: gate must be >= 0"
    assert not any(buf)
    texts = checks_before_the_device("os2r_ekf_capi.hip", name, ("layout_refusal", "slots_refusal"))
    assert len(texts) == 20 and {("os2re_ekf_update: " + t).encode() for t in texts} == seen


# ---------------------------------------------------------------------------------------
# the Python layer, without a device
# ---------------------------------------------------------------------------------------
NQ, D, M = 3, 4, 5
n = 2 * NQ


def _bare(dtype):
    """A HipSim that never met a device: enough of it for the checks that run before the library is called."""
    import torch
    from gym_os2r_amd.sim import HipSim
    s = HipSim.__new__(HipSim)
    s.N, s.nq, s.D, s.dtype, s.device = 8, NQ, D, dtype, torch.device("cpu")
    s._h = None
    s._lib = None      # (and it has no cfg: filling the layout would raise AttributeError, not ValueError)
    return s


def test_python_argument_errors_need_no_device():
    import torch
    from gym_os2r_amd.sim import HipSim
    assert callable(HipSim.ekf_update) and callable(HipSim.ekf_update_into)
    f64 = torch.float64
    s = _bare(f64)
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    x, P, A, meas, prec, xo, Po = z(n, M), z(n, n, M), z(n, n, M), z(M, D), z(D), z(n, M), z(n, n, M)
    Q = torch.eye(n, dtype=f64)
    skew = Q.clone()
    skew[0, 1] = 0.5

    def into(*args, **kw):
        with pytest.raises(ValueError, match="^ekf_update: "):
            s.ekf_update_into(*args, **kw)

    def whole(*args, **kw):
        with pytest.raises(ValueError, match="^ekf_update: "):
            s.ekf_update(*args, **kw)
    good = (x, P, meas, prec, xo, Po)
    for i in range(6):                                                     # each required tensor None
        into(*[None if j == i else t for j, t in enumerate(good)])
    for args in ((z(n + 1, M), P, meas, prec, xo, Po), (z(n), P, meas, prec, xo, Po), (z(n, 0), P, meas, prec, xo, Po),
                 (x.numpy(), P, meas, prec, xo, Po), (x, z(n, n, M + 1), meas, prec, xo, Po), (x, z(M, n, n).permute(1, 2, 0), meas, prec, xo, Po),
                 (x, P.float(), meas, prec, xo, Po), (x, P, z(M, D + 1), prec, xo, Po), (x, P, z(D, M).t(), prec, xo, Po),
                 (x, P, meas.float(), prec, xo, Po), (x, P, meas, z(D + 1), xo, Po), (x, P, meas, prec.float(), xo, Po),
                 (x, P, meas, prec, z(n, M + 1), Po), (x, P, meas, prec, xo.float(), Po), (x, P, meas, prec, xo, z(n, n + 1, M)),
                 (x, P, meas, prec, xo, z(M, n, n).permute(1, 2, 0)), (x.float(), P, meas, prec, xo, Po)):
        into(*args)
    for kw in (dict(A=A), dict(A=A, Q=None), dict(A=A, Q=skew), dict(A=A, Q=skew.tolist()), dict(A=A, Q=Q * float("nan")),
               dict(A=A, Q=torch.eye(n + 1)), dict(A=A, Q="x"), dict(A=z(n, n, M + 1), Q=Q), dict(A=A.float(), Q=Q),
               dict(A=z(M, n, n).permute(1, 2, 0), Q=Q), dict(gate=-1.0), dict(gate=float("nan")), dict(gate=float("inf")), dict(gate="x"),
               dict(gate=True), dict(gate=None), dict(nis=z(M + 1)), dict(nis=z(M).float()), dict(used=z(M)), dict(used=i32(M + 1)),
               dict(used=torch.zeros(M, dtype=torch.int64)), dict(refused=z(M)), dict(refused=torch.zeros(M, dtype=torch.int64)),
               dict(innov=z(M, D + 1)), dict(innov=z(D, M).t()), dict(innov=z(M, D).float())):
        into(*good, **kw)
    Pv, Av = z(n, n, M).permute(2, 0, 1), z(n, n, M).permute(2, 0, 1)
    for args in ((None, Pv, meas, prec), (x, None, meas, prec), (x, Pv, None, prec), (x, Pv, meas, None), (z(n + 1, M), Pv, meas, prec),
                 (z(n), Pv, meas, prec), (x, z(M + 1, n, n), meas, prec), (x, P, meas, prec), (x, Pv, z(M + 1, D), prec), (x, Pv, meas.float(), prec),
                 (x, Pv, meas, z(D - 1)), ((x[:NQ], x[NQ:n - 1]), Pv, meas, prec), (x.float(), Pv, meas, prec)):
        whole(*args)
    for kw in (dict(A=Av), dict(A=Av, Q=skew), dict(A=Av, Q=Q * float("inf")), dict(A=z(M, n, n + 1), Q=Q), dict(A=z(n, n, M), Q=Q),
               dict(gate=-1.0), dict(gate=float("nan")), dict(gate="x"), dict(gate=False)):
        whole(x, Pv, meas, prec, **kw)


class Recorder:
    """Stands where the library would be: every attribute is a function that keeps its positional arguments and returns OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return abi.OK
        return call


def _decode(a):
    if isinstance(a, C.c_void_p):
        return a.value
    if isinstance(a, C.Array):
        return list(a)
    return getattr(a, "_obj", a)


ORDER = ["layout", "M", "x_pred", "P_in", "A", "q", "meas", "prec", "gate", "x_out", "P_out", "nis", "used", "refused", "innov", "stream"]


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_what_reaches_c_position_by_position(dt, monkeypatch):
    import torch
    from gym_os2r_amd import control, ekf
    dt = getattr(torch, dt)
    rec, stream = Recorder(), C.c_void_p(0)
    s = _bare(dt)
    s._control_layout = control.layout(abi.F64 if dt == torch.float64 else abi.F32, NQ, 0, [0, 1, 2, 3])
    s._stream = lambda: stream
    reached = []
    monkeypatch.setattr(ekf, "load", lambda: (reached.append("ekf"), rec)[1])
    z = lambda *shape, dtype=dt: torch.zeros(*shape, dtype=dtype)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    QV = torch.arange(float(n * n), dtype=torch.float64).reshape(n, n)
    QV = QV + QV.T + 40.0 * torch.eye(n, dtype=torch.float64)

    def held(kw, **special):
        name, args = rec.calls[-1]
        assert name == "os2re_ekf_update" and len(args) == len(ekf.ENTRY_POINTS[name]) == len(ORDER) == 16
        for i, (what, got) in enumerate(zip(ORDER, args)):
            where = f"argument {i} ({what})"
            if what == "stream":
                assert got is stream, where
            elif what == "layout":
                assert _decode(got) is s._control_layout, where
            elif what in special:
                assert _decode(got) == special[what] and type(_decode(got)) is type(special[what]), where
            else:
                assert _decode(got) == (None if kw[what] is None else kw[what].data_ptr()), where
    kw = dict(x_pred=z(n, M), P_in=z(n, n, M), meas=z(M, D), prec=z(D), x_out=z(n, M), P_out=z(n, n, M), A=z(n, n, M), Q=QV, gate=9.5,
              nis=z(M), used=i32(M), refused=i32(M), innov=z(M, D))
    ptrs = [v.data_ptr() for k, v in kw.items() if isinstance(v, torch.Tensor) and k != "Q"]
    assert len(set(ptrs)) == len(ptrs)
    s.ekf_update_into(**kw)
    held(kw, M=M, q=QV.reshape(-1).tolist(), gate=9.5)
    # without A the process noise does not reach the library; the optional outputs are null, the gate 0; equal pointers go on
    bare = dict(kw, A=None, nis=None, used=None, refused=None, innov=None, x_out=kw["x_pred"], P_out=kw["P_in"])
    del bare["gate"]
    s.ekf_update_into(**bare)
    held(bare, M=M, q=None, gate=0.0)
    assert reached == ["ekf", "ekf"]

    # the allocating form: linearize()'s A, its pair of halves and the P an earlier call returned go on without a copy
    seen, real = [], type(s).ekf_update_into

    def spy(self, *args, **kwargs):
        names = ("x_pred", "P_in", "meas", "prec", "x_out", "P_out")
        seen.append(dict(zip(names, args), **kwargs))
        return real(self, *args, **kwargs)
    monkeypatch.setattr(type(s), "ekf_update_into", spy)
    same = lambda a, b: a.data_ptr() == b.data_ptr()
    nxt = z(n, M)
    A = z(n, n, M).permute(2, 0, 1)
    P0 = torch.eye(n, dtype=dt).repeat(M, 1, 1)                             # no view of the kernel's layout: converted and copied
    meas, prec = z(M, D), z(D)
    x1, P1, nis, used, refused, innov = s.ekf_update((nxt[:NQ], nxt[NQ:]), P0, meas, prec, A=A, Q=QV, gate=9.5, want_innov=True)
    first = seen[0]
    for name, shape in (("x_pred", (n, M)), ("P_in", (n, n, M)), ("A", (n, n, M)), ("x_out", (n, M)), ("P_out", (n, n, M)), ("nis", (M,)),
                        ("innov", (M, D)), ("meas", (M, D)), ("prec", (D,))):
        assert tuple(first[name].shape) == shape and first[name].is_contiguous() and first[name].dtype == dt, name
    assert first["used"].dtype == first["refused"].dtype == torch.int32 and tuple(first["used"].shape) == tuple(first["refused"].shape) == (M,)
    assert same(first["x_pred"], nxt) and same(first["A"], A) and not same(first["P_in"], P0) and first["meas"] is meas and first["prec"] is prec
    assert torch.equal(first["P_in"], P0.permute(1, 2, 0))
    held(first, M=M, q=QV.reshape(-1).tolist(), gate=9.5)
    assert tuple(x1.shape) == (n, M) and tuple(P1.shape) == (M, n, n) and tuple(innov.shape) == (M, D) and same(P1, first["P_out"])
    assert all(tuple(t.shape) == (M,) for t in (nis, used, refused)) and x1 is first["x_out"]
    # the returned P fed back: no copy, and the two kept buffers alternate
    x2, P2 = s.ekf_update(nxt, P1, meas, prec)[:2]
    x3, P3, *_, none = s.ekf_update(nxt, P2, meas, prec, A=A, Q=QV)
    assert same(seen[1]["P_in"], P1) and same(seen[2]["P_in"], P2) and not same(P1, P2) and same(P3, P1) and none is None
    assert seen[1]["A"] is None and seen[1]["innov"] is None and seen[1]["gate"] == 0.0 and seen[1]["x_pred"] is nxt
    held(seen[2], M=M, q=QV.reshape(-1).tolist(), gate=0.0)
    # a pair that is not the two halves of one tensor is joined
    s.ekf_update((z(NQ, M), z(NQ, M)), P1, meas, prec)
    assert tuple(seen[3]["x_pred"].shape) == (n, M) and len(rec.calls) == 6
