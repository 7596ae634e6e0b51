"""libos2r_cem.so (include/os2r_cem.h): the host side -- the numpy restatement of the update the GPU tests compare with
(`restate_cem`) against the textbook statement in float64 on crafted inputs that reach every branch of it (`crafted_cem`), the
header against the one table of gym_os2r_amd/cem.py, the exports of the library, the other libraries as they were, the resources
of the four kernels in the built library, every refusal of os2rx_cem_update through ctypes without a device, and the argument
checks of HipSim.cem_update that need no device.  No GPU needed."""
import ctypes as C
import itertools
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

NAMES = ["os2rx_abi_version", "os2rx_last_error", "os2rx_cem_update"]
CHUNKS = 8
BRANCH_SHAPE = (7, 70, 11, 4)           # K, M, S, E: two workgroups with a tail, S no multiple of 8, ties across the boundary
# ... E = 1, E = S, S = 3: empty partials, S = 1
HOST_SHAPES = [BRANCH_SHAPE, (7, 70, 11, 1), (7, 70, 11, 11), (7, 70, 3, 2), (7, 70, 1, 1)]
NONE_VALID = 5                          # the robot without a valid lane
SIGMA_MIN, SIGMA_MAX = 0.05, 0.5        # reached from below by the robots whose samples agree, from above by those of +-1.5
# The largest distance of the restatement from the textbook statement in float64 over HOST_SHAPES x gains (1, 0.5) x sigma gains
# (1, 0.5), measured on the CPU this test was written on (test_the_restatement_is_the_textbook_update prints them): the bound is
# 100 x that, the margin of the ekf and ukf host tests.
MEASURED = {np.float64: dict(mean=2.776e-16, var=4.441e-16, sigma=1.110e-16), np.float32: dict(mean=5.960e-8, var=8.825e-8, sigma=3.994e-8)}
MARGIN = 100


# ---------------------------------------------------------------------------------------
# the restatement of include/os2r_cem.h (needs no device)
# ---------------------------------------------------------------------------------------
def chunked_over(x, elite, dtype):
    """Step 3: the sum of x [S, K, M, 2] over the elite samples (elite [S, M] bool) in eight partials, partial c adding its elite
    samples s = c, c + 8, ... in ascending order onto 0, lanes that are not elite skipped."""
    p = []
    for c in range(CHUNKS):
        acc = np.zeros(x.shape[1:], dtype)
        for s in range(c, x.shape[0], CHUNKS):
            acc = np.where(elite[s][None, :, None], acc + x[s], acc)
        p.append(acc)
    return ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))


def elite_set(returns, S, E, dtype):
    """Steps 1 and 2 -> (elite [S, M] bool, count [M] int32, e [M], threshold [M] in `dtype`).  Literally: lane s is an elite iff it
    is valid and fewer than e valid lanes come before it, a lane coming before another if its return is higher, or equal (-0 and
    +0 are) and its sample index lower."""
    r = np.asarray(returns).astype(dtype).reshape(S, -1)
    valid = np.isfinite(r)
    count = valid.sum(0).astype(np.int32)
    e = np.minimum(E, count)
    with np.errstate(all="ignore"):
        higher = r[:, None, :] > r[None, :, :]                                           # [s', s, m]: s' is ahead of s by its return
        tied = (r[:, None, :] == r[None, :, :]) & (np.arange(S)[:, None, None] < np.arange(S)[None, :, None])
    before = ((higher | tied) & valid[:, None, :]).sum(0)                                # [s, m]
    elite = valid & (before < e[None, :])
    with np.errstate(all="ignore"):
        threshold = np.where(elite, r, np.inf).min(0)
    threshold = (np.where(count > 0, threshold, 0) + 0.0).astype(dtype)                  # (+ 0.0: the threshold -0 reads +0)
    return elite, count, e, threshold


def restate_cem(returns, actions, nominal_in, sigma_in, *, S, E, gain=1.0, sigma_gain=1.0, sigma_min=0.0, sigma_max=1.0, shift=1,
                tail_zero=False, dtype):
    """include/os2r_cem.h, steps 1-11, in numpy and in `dtype`.  sigma_in [2, M].  -> dict(nominal_out [K, M, 2], var [K, M, 2],
    sigma_out [2, M], applied [M, 2], bias [K, 2, N]: the bias entries of the table, lane_sigma [2, N], elite [S, M] int32,
    threshold [M], count [M] int32, mean [K, M, 2], sd [2, M])."""
    K, N, _ = actions.shape
    M = N // S
    g, sg, lo, hi = (np.float64(v).astype(dtype) for v in (gain, sigma_gain, sigma_min, sigma_max))      # rounded once
    elite, count, e, threshold = elite_set(returns, S, E, dtype)
    a = np.asarray(actions).astype(dtype).reshape(K, S, M, 2).transpose(1, 0, 2, 3)                       # [S, K, M, 2]
    nom = np.asarray(nominal_in).astype(dtype)
    sig_in = np.asarray(sigma_in).astype(dtype)
    some = count > 0
    with np.errstate(all="ignore"):
        te = e.astype(dtype)[None, :, None]
        A = chunked_over(a, elite, dtype)
        mu = A / te
        d = a - mu[None]
        V = chunked_over((d * d).astype(dtype), elite, dtype)
        var = np.where(some[None, :, None], V / te, 0).astype(dtype)
        moved = mu if g == 1 else nom + g * (mu - nom)
        mean = np.where(some[None, :, None], np.clip(moved, -1, 1), nom).astype(dtype)
        acc = np.zeros((M, 2), dtype)
        for k in range(K):
            acc = acc + var[k]
        sd = np.sqrt(acc / dtype(K)).T                                                                     # [2, M]
        sig = sd if sg == 1 else sig_in + sg * (sd - sig_in)
        sigma_out = np.where(some[None, :], np.minimum(np.maximum(sig, lo), hi), sig_in).astype(dtype)
    out = np.stack([mean[min(k + shift, K - 1)] for k in range(K)])
    if tail_zero:
        out[[k for k in range(K) if k + shift >= K]] = 0
    bias = np.tile(out.transpose(0, 2, 1), (1, 1, S))                                                      # [K, 2, S M], lane s M + m
    lane_sigma = np.tile(sigma_out, (1, S))
    assert all(x.dtype == dtype for x in (A, mu, V, var, mean, sd, sigma_out, out, bias, lane_sigma, threshold))
    return dict(nominal_out=out, var=var, sigma_out=sigma_out, applied=mean[0].copy(), bias=bias, lane_sigma=lane_sigma,
                elite=elite.astype(np.int32), threshold=threshold, count=count, mean=mean, sd=sd)


def textbook_cem(returns, actions, nominal_in, sigma_in, *, S, E, gain, sigma_gain, sigma_min, sigma_max):
    """The same update as a textbook states it, in float64 and robot by robot: a stable argsort of -returns over the valid lanes,
    np.mean and np.var of the elites' actions, sqrt of the mean variance."""
    K, N, _ = actions.shape
    M = N // S
    r = np.asarray(returns, np.float64).reshape(S, M)
    a = np.asarray(actions, np.float64).reshape(K, S, M, 2)
    nom, sig_in = np.asarray(nominal_in, np.float64), np.asarray(sigma_in, np.float64)
    mean, var, sigma = nom.copy(), np.zeros((K, M, 2)), sig_in.copy()
    elite, count, threshold = np.zeros((S, M), np.int32), np.zeros(M, np.int32), np.zeros(M)
    for m in range(M):
        lanes = np.flatnonzero(np.isfinite(r[:, m]))
        count[m] = len(lanes)
        if not len(lanes):
            continue
        best = lanes[np.argsort(-(r[lanes, m] + 0.0), kind="stable")][:E]
        elite[best, m] = 1
        threshold[m] = r[best[-1], m] + 0.0
        mu = np.mean(a[:, best, m], axis=1)
        var[:, m] = np.var(a[:, best, m], axis=1)
        mean[:, m] = np.clip(nom[:, m] + gain * (mu - nom[:, m]), -1, 1)
        sd = np.sqrt(np.mean(var[:, m], axis=0))
        sigma[:, m] = np.clip(sig_in[:, m] + sigma_gain * (sd - sig_in[:, m]), sigma_min, sigma_max)
    return dict(mean=mean, var=var, sigma_out=sigma, elite=elite, count=count, threshold=threshold)


def crafted_cem(K, M, S, seed=0):
    """Inputs in float64 (the caller rounds): returns in 0..10, actions and nominal in -1..1, sigma in 0.1..0.4 and, by robot (where M
    reaches it),
      m % 9 == 1   NaN returns on the samples s % 3 == 0 (every one of them with S = 1)
      m % 9 == 2   +inf on sample 0 and -inf on the last sample
      m = 5        no valid lane at all
      m % 9 == 3   returns quantised to the three values 1, 2, 3: ties on both sides of the elite boundary
      m % 9 == 4   returns +0 and -0 in turn: every lane tied
      m % 9 == 6   actions of +-1.5: the mean is clamped, the elites agree
      m % 9 == 7   one valid lane, the last: 0 < count < E wherever E > 1
      m % 9 == 8   actions of +1.5 on even samples and -1.5 on odd ones: a width above sigma_max
    -> dict(returns [N], actions [K, N, 2], nominal [K, M, 2], sigma [2, M])"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.0, 10.0, (S, M))
    a = rng.uniform(-1.0, 1.0, (K, S, M, 2))
    nominal = rng.uniform(-1.0, 1.0, (K, M, 2))
    sigma = rng.uniform(0.1, 0.4, (2, M))
    m, s = np.arange(M), np.arange(S)
    r[np.ix_(s % 3 == 0, m % 9 == 1)] = np.nan
    r[0, m % 9 == 2] = np.inf
    r[S - 1, m % 9 == 2] = -np.inf
    r[:, m == NONE_VALID] = np.nan
    r[:, m % 9 == 3] = np.floor(r[:, m % 9 == 3] / 3.4) + 1.0
    r[:, m % 9 == 4] = np.where(s % 2 == 0, 0.0, -0.0)[:, None]
    r[:S - 1, m % 9 == 7] = np.nan
    a[:, :, m % 9 == 6, 0], a[:, :, m % 9 == 6, 1] = 1.5, -1.5
    a[:, :, m % 9 == 8, :] = np.where(s % 2 == 0, 1.5, -1.5)[None, :, None, None]
    return dict(returns=r.reshape(-1), actions=a.reshape(K, S * M, 2), nominal=nominal, sigma=sigma)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_is_the_textbook_update(dtype):
    """elite, count and threshold agree exactly; mean, var and sigma within MARGIN x the distance measured when this was written."""
    worst = dict(mean=0.0, var=0.0, sigma=0.0)
    for (K, M, S, E), gain, sigma_gain in itertools.product(HOST_SHAPES, (1.0, 0.5), (1.0, 0.5)):
        c = crafted_cem(K, M, S)
        kw = dict(S=S, E=E, gain=gain, sigma_gain=sigma_gain, sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX)
        got = restate_cem(c["returns"], c["actions"], c["nominal"], c["sigma"], shift=0, dtype=dtype, **kw)
        rounded = [np.asarray(c[k]).astype(dtype).astype(np.float64) for k in ("returns", "actions", "nominal", "sigma")]
        lo, hi = float(dtype(SIGMA_MIN)), float(dtype(SIGMA_MAX))
        want = textbook_cem(*rounded, **dict(kw, sigma_min=lo, sigma_max=hi))
        for name in ("elite", "count", "threshold"):
            assert np.array_equal(got[name], want[name]), (name, K, M, S, E)
        assert np.isfinite(got["mean"]).all() and np.isfinite(got["var"]).all() and np.isfinite(got["sigma_out"]).all()
        for name, key in (("mean", "mean"), ("var", "var"), ("sigma", "sigma_out")):
            worst[name] = max(worst[name], float(np.abs(got[key].astype(np.float64) - want[key]).max()))
    print(f"restate_cem against the textbook, {dtype.__name__}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for name, value in worst.items():
        assert value <= MARGIN * MEASURED[dtype][name], (name, value)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_on_crafted_inputs_that_reach_every_branch(dtype):
    from gym_os2r_amd import cem
    assert CHUNKS == cem.CHUNKS == int(re.search(r"#define OS2RX_CHUNKS (\d+)", _header("os2r_cem.h")).group(1))
    K, M, S, E = BRANCH_SHAPE
    c = crafted_cem(K, M, S)
    m = np.arange(M)
    kw = dict(S=S, E=E, sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX, dtype=dtype)
    args = (c["returns"], c["actions"], c["nominal"], c["sigma"])
    out = restate_cem(*args, shift=1, **kw)
    nominal, sigma = c["nominal"].astype(dtype), c["sigma"].astype(dtype)
    r = c["returns"].astype(dtype).reshape(S, M)
    a = c["actions"].astype(dtype).reshape(K, S, M, 2)
    elite, count, mean, thr = out["elite"], out["count"], out["mean"], out["threshold"]
    # invalid lanes: NaN, +inf and -inf, never elite, counted out; e = min(E, count) elites
    assert (count[m % 9 == 1] == S - len(range(0, S, 3))).all() and (count[m % 9 == 2] == S - 2).all() and (count[m % 9 == 7] == 1).all()
    assert np.isnan(r).any() and (r == np.inf).any() and (r == -np.inf).any() and (elite[~np.isfinite(r)] == 0).all()
    assert np.array_equal(elite.sum(0), np.minimum(E, count)) and 0 < count[7] < E
    # no valid lane: the robot keeps its nominal and its sigma, unclamped; var 0, threshold 0
    assert count[NONE_VALID] == 0 and (count == 0).sum() == 1 and thr[NONE_VALID] == 0 and (out["var"][:, NONE_VALID] == 0).all()
    assert np.array_equal(mean[:, NONE_VALID], nominal[:, NONE_VALID]) and np.array_equal(out["sigma_out"][:, NONE_VALID], sigma[:, NONE_VALID])
    # one valid lane: its actions are the mean, the variance is 0, the width is sigma_min
    assert np.array_equal(mean[:, 7], a[:, S - 1, 7]) and (out["var"][:, 7] == 0).all() and (out["sigma_out"][:, 7] == dtype(SIGMA_MIN)).all()
    # three values: ties straddle the boundary, cut by the sample index
    q = 3
    tied = r[:, q] == thr[q]
    assert tied.sum() > elite[tied, q].sum() > 0 and (elite[r[:, q] > thr[q], q] == 1).all() and (elite[r[:, q] < thr[q], q] == 0).all()
    first = np.flatnonzero(tied)[:elite[tied, q].sum()]
    assert (elite[first, q] == 1).all() and elite[np.flatnonzero(tied)[-1], q] == 0
    # +0 and -0 are tied: the first E samples are the elites
    assert np.signbit(r[1, 4]) and not np.signbit(r[0, 4]) and (elite[:E, 4] == 1).all() and (elite[E:, 4] == 0).all() and thr[4] == 0
    # the clamp of the mean, from both sides; the width at both bounds and between them
    assert (mean[:, m % 9 == 6, 0] == 1).all() and (mean[:, m % 9 == 6, 1] == -1).all() and (np.abs(mean) <= 1).all()
    assert (out["sigma_out"][:, m % 9 == 6] == dtype(SIGMA_MIN)).all()
    wide = out["sd"] > SIGMA_MAX                      # (of the robots m % 9 == 8 those whose elites hold samples of both signs)
    assert wide[:, m % 9 == 8].sum() > (m % 9 == 8).sum() and (out["sigma_out"][wide] == dtype(SIGMA_MAX)).all()
    between = (out["sigma_out"] > dtype(SIGMA_MIN)) & (out["sigma_out"] < dtype(SIGMA_MAX)) & (count > 0)[None]
    assert between.any() and np.array_equal(out["sigma_out"][between], out["sd"][between])
    # the gains: half way, each on its own
    half = restate_cem(*args, shift=1, gain=0.5, sigma_gain=0.5, **kw)
    assert np.array_equal(half["elite"], elite) and not np.array_equal(half["mean"], mean) and not np.array_equal(half["sigma_out"], out["sigma_out"])
    assert np.array_equal(restate_cem(*args, shift=1, gain=0.5, **kw)["sigma_out"], out["sigma_out"])
    assert np.array_equal(restate_cem(*args, shift=1, sigma_gain=0.5, **kw)["mean"], mean)
    plain = m % 9 == 0
    mu = restate_cem(*args, shift=1, **dict(kw, sigma_max=10.0))
    by_hand = nominal[:, plain] + dtype(0.5) * (mu["mean"][:, plain] - nominal[:, plain])
    assert np.array_equal(half["mean"][:, plain], by_hand)
    # every partial holds something (S = 11 > 8), partials 3..7 one term, partials 0..2 two
    assert S > CHUNKS and S % CHUNKS
    # the shift and both tails
    assert np.array_equal(out["applied"], mean[0]) and np.array_equal(out["nominal_out"][:-1], mean[1:])
    assert np.array_equal(out["nominal_out"][-1], mean[-1])
    zero = restate_cem(*args, shift=1, tail_zero=True, **kw)
    assert np.array_equal(zero["nominal_out"][:-1], mean[1:]) and (zero["nominal_out"][-1] == 0).all() and np.array_equal(zero["applied"], mean[0])
    for tail_zero in (False, True):
        same = restate_cem(*args, shift=0, tail_zero=tail_zero, **kw)
        assert np.array_equal(same["nominal_out"], mean)
        far = restate_cem(*args, shift=K, tail_zero=tail_zero, **kw)
        assert np.array_equal(far["nominal_out"], np.zeros_like(mean) if tail_zero else np.tile(mean[-1], (K, 1, 1)))
        assert np.array_equal(far["applied"], mean[0]) and np.array_equal(far["sigma_out"], out["sigma_out"])
    # the bias entries and the lane sigma: lane s M + m holds its robot's
    lane = np.arange(S * M)
    assert np.array_equal(out["bias"], out["nominal_out"].transpose(0, 2, 1)[:, :, lane % M]) and out["bias"].shape == (K, 2, S * M)
    assert np.array_equal(out["lane_sigma"], out["sigma_out"][:, lane % M]) and out["lane_sigma"].shape == (2, S * M)
    # E = 1: the best lane's actions, no variance; E = S: every valid lane; fewer samples than partials; one sample
    for K3, M3, S3, E3 in HOST_SHAPES[1:]:
        c3 = crafted_cem(K3, M3, S3)
        o3 = restate_cem(c3["returns"], c3["actions"], c3["nominal"], c3["sigma"], shift=1, **dict(kw, S=S3, E=E3))
        a3 = c3["actions"].astype(dtype).reshape(K3, S3, M3, 2)
        r3 = c3["returns"].astype(dtype).reshape(S3, M3)
        plain = np.flatnonzero(np.arange(M3) % 9 == 0)
        assert np.isfinite(o3["mean"]).all() and (o3["count"] == 0).any() and (o3["count"] == S3).any()
        if E3 == 1:
            best = np.argmax(r3[:, plain], axis=0)
            assert np.array_equal(o3["mean"][:, plain], a3[:, best, plain]) and (o3["var"] == 0).all()
            assert (o3["sigma_out"][:, o3["count"] > 0] == dtype(SIGMA_MIN)).all()
        if E3 == S3:
            assert np.array_equal(o3["elite"], np.isfinite(r3).astype(np.int32))
        if S3 == 3:
            e2 = o3["elite"][:, plain].astype(bool)
            by_hand = np.where(e2[0], a3[:, 0, plain, 0], 0) + np.where(e2[1], a3[:, 1, plain, 0], 0)      # partials 0 and 1 ...
            by_hand = (by_hand + np.where(e2[2], a3[:, 2, plain, 0], 0)) / dtype(2)                      # ... and partial 2
            assert S3 < CHUNKS and np.array_equal(np.clip(by_hand, -1, 1), o3["mean"][:, plain, 0])


# ---------------------------------------------------------------------------------------
# header, table, exports
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import cem, control
    protos = _prototypes("os2r_cem.h", "os2rx")
    assert [p[0] for p in protos] == list(cem.ENTRY_POINTS) == NAMES
    lib = cem.load()
    for name, ret, args in protos:
        argtypes = cem.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2rx_last_error" else C.c_int)
    args = protos[2][2]
    assert args[0] == "const Os2rControlLayout* layout" and args[4] == "int32_t nelite" and args[-1] == "void* stream" and len(args) == 25
    assert args[9:13] == ["double gain", "double sigma_gain", "double sigma_min", "double sigma_max"]
    assert cem.ENTRY_POINTS["os2rx_cem_update"][2] is C.c_int64 and all(t is C.c_double for t in cem.ENTRY_POINTS["os2rx_cem_update"][9:13])
    header = _header("os2r_cem.h")
    assert re.search(r"#define OS2R_CEM_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert lib.os2rx_abi_version() == cem.ABI_VERSION == 1
    assert cem.TAIL_ZERO == int(re.search(r"#define OS2RX_TAIL_ZERO (\d)u", header).group(1)) == 1 and cem.TAILS == dict(hold=0, zero=1)
    assert cem.Os2rControlLayout is control.Os2rControlLayout and cem.layout is control.layout
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", cem.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)


def test_the_other_libraries_are_as_they_were():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib, cem, control, ekf, mppi, pf, search, steer, ukf
    loaders = (control, search, steer, mppi, pf, ekf, ukf)
    others = set(_lib.ENTRY_POINTS) | set(_lib.RECORD_ENTRY_POINTS) | set().union(*(set(mod.ENTRY_POINTS) for mod in loaders))
    assert not set(cem.ENTRY_POINTS) & others and not any(name.startswith("os2rx_") for name in others)
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "os2r_cem.h":
            assert "os2rx_" not in _header(name) and "os2r_cem" not in _header(name).lower(), name
    assert len(_lib.ENTRY_POINTS) == 35 and len(_lib.RECORD_ENTRY_POINTS) == 3
    assert list(control.ENTRY_POINTS) == ["os2rc_abi_version", "os2rc_last_error", "os2rc_ilqr_backward"]
    assert list(search.ENTRY_POINTS) == ["os2rs_abi_version", "os2rs_last_error", "os2rs_ilqr_line_search"]
    assert list(steer.ENTRY_POINTS) == ["os2rt_abi_version", "os2rt_last_error", "os2rt_ilqr_backward_mu", "os2rt_ilqr_steer"]
    assert list(mppi.ENTRY_POINTS) == ["os2rm_abi_version", "os2rm_last_error", "os2rm_mppi_update"]
    assert list(pf.ENTRY_POINTS) == ["os2rp_abi_version", "os2rp_last_error", "os2rp_pf_update"]
    assert list(ekf.ENTRY_POINTS) == ["os2re_abi_version", "os2re_last_error", "os2re_ekf_update"]
    assert list(ukf.ENTRY_POINTS) == ["os2ru_abi_version", "os2ru_last_error", "os2ru_ukf_points", "os2ru_ukf_update"]
    exports = {_lib.LIB_PATH: set(_lib.ENTRY_POINTS), _lib.RECORD_LIB_PATH: set(_lib.RECORD_ENTRY_POINTS)}
    exports.update({mod.LIB_PATH: set(mod.ENTRY_POINTS) for mod in loaders})
    assert len(exports) == 9
    for path, table in exports.items():
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == table, path
        kernels = kernel_meta.kernel_meta(path)
        assert kernels and not any("cem" in k for k in kernels), path


def test_kernel_resources():
    """Exactly four kernels, the update and the pooling in float and double, are in the built library and none uses scratch:
    private_segment_fixed_size 0, no VGPR or SGPR spill and no AGPRs in the code-object metadata.  With at most 64 registers the 8
    waves of a workgroup leave room for three more workgroups on a CU, whose LDS holds four of the widest kernel's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import cem
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(cem.LIB_PATH)
    meta = kernel_meta.kernel_meta(cem.LIB_PATH)
    assert len(meta) == 4, sorted(meta)
    for kernel in ("cem_update_kernel", "cem_pool_kernel"):
        for real in ("float", "double"):
            (name,) = [k for k in meta if f"{kernel}<{real}>" in k]
            m = meta[name]
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
            assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 64, (name, m)
            assert 0 < 4 * m["group_segment_fixed_size"] <= 160 * 1024, (name, m)


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def test_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import cem, control
    lib = cem.load()
    K, M, S, E = 3, 4, 2, 1
    buf = (C.c_double * 4096)()
    base = (C.addressof(buf) + 15) & ~15                  # a pair of doubles is 16 bytes
    at = lambda i: C.c_void_p(base + 8 * i)
    nan, inf = float("nan"), float("inf")
    F32 = abi.F32

    def Lay(dtype=abi.F64, **kw):
        lay = control.layout(dtype, 3, 0, [0, 1, 3, -1])
        for k, v in kw.items():
            setattr(lay, k, v)
        return C.byref(lay)
    P = 2 * K * M                                         # the elements of a nominal, and of var_out
    # returns at 0 (8), actions at 64 (48), nominal_in at 1024, sigma_in at 1200 (8), then the outputs
    good = dict(lay=Lay(), K=K, M=M, S=S, E=E, ret=at(0), act=at(64), nin=at(1024), sin=at(1200), gain=1.0, sgain=1.0, lo=0.0, hi=1.0,
                shift=1, flags=0, nout=at(1024 + P), var=at(1024 + 2 * P), sout=at(1200), app=None, table=None, lane=None, elite=None,
                thr=None, count=None)
    name = "os2rx_cem_update"
    assert len(good) + 1 == len(cem.ENTRY_POINTS[name])

    def call(**kw):
        a = dict(good, **kw)
        return lib.os2rx_cem_update(*[a[k] for k in good], None)
    assert lib.os2rx_cem_update(*[None if _is_pointer(t) else 0 for t in cem.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rx_last_error() == b"os2rx_cem_update: null layout"
    tab = dict(table=at(2048))
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(nq=1)), b"nq must be 2..5"),
             (dict(K=0), b"nknots must be >= 1"), (dict(K=-3), b"nknots must be >= 1"), (dict(K=65536, shift=0), b"nknots must be <= 65535"),
             (dict(M=0), b"nrobots must be >= 1"), (dict(M=-1), b"nrobots must be >= 1"), (dict(S=0), b"nsamples must be >= 1"),
             (dict(E=0), b"nelite must be >= 1"), (dict(E=-2), b"nelite must be >= 1"), (dict(E=S + 1), b"nelite must be <= nsamples"),
             (dict(M=2 ** 62), b"nsamples * nrobots exceeds 2^31 - 1"), (dict(M=2 ** 30, S=2), b"nsamples * nrobots exceeds 2^31 - 1"),
             (dict(shift=-1), b"shift must be 0..nknots"), (dict(shift=K + 1), b"shift must be 0..nknots"),
             (dict(flags=2), b"unknown flag bits"), (dict(flags=0x80000001), b"unknown flag bits")]
    for key, word in (("gain", b"gain"), ("sgain", b"sigma_gain")):
        cases += [(dict({key: v}), b": " + word + b" must be finite") for v in (nan, inf, -inf)]
        cases += [(dict({key: v}), b": " + word + b" must be in (0, 1]") for v in (0.0, -0.5, 1.0000001, 5e-324 * -1)]
        cases += [(dict({key: 1e-50}, lay=Lay(F32)), b": " + word + b" is outside the normal range of fp32")]
    for key, word in (("lo", b"sigma_min"), ("hi", b"sigma_max")):
        cases += [(dict({key: v}), b": " + word + b" must be finite") for v in (nan, inf, -inf)]
        cases += [(dict({key: -1e-300}), b": " + word + b" must be >= 0")]
        cases += [(dict({key: 1e-50}, lay=Lay(F32)), b": " + word + b" is outside the normal range of fp32")]
    cases += [(dict(hi=1e39, lay=Lay(F32)), b": sigma_max is outside the normal range of fp32"),
              (dict(lo=0.5, hi=0.25), b"sigma_min must be <= sigma_max"),
              (dict(ret=None), b"null returns_dev"), (dict(act=None), b"null actions_dev"), (dict(nin=None), b"null nominal_in_dev"),
              (dict(sin=None), b"null sigma_in_dev"), (dict(nout=None), b"null nominal_out_dev"), (dict(var=None), b"null var_out_dev"),
              (dict(sout=None), b"null sigma_out_dev"), (dict(act=at(65)), b"actions_dev must be aligned to a pair"),
              (dict(nout=at(1024)), b"nominal_out_dev overlaps nominal_in_dev"),
              (dict(nout=at(1024 + P - 1)), b"nominal_out_dev overlaps nominal_in_dev"),
              (dict(nout=at(1024 - P + 1), var=at(3000)), b"nominal_out_dev overlaps nominal_in_dev"),
              (dict(var=at(S * M - 1)), b"var_out_dev overlaps returns_dev"), (dict(var=at(64 + 2 * K * S * M - 1)), b"var_out_dev overlaps actions_dev"),
              (dict(var=at(64 - P + 1)), b"var_out_dev overlaps actions_dev"), (dict(var=at(1024 + P - 1), nout=at(3000)), b"var_out_dev overlaps nominal_in_dev"),
              (dict(var=at(1200 + 2 * M - 1)), b"var_out_dev overlaps sigma_in_dev"), (dict(var=at(1200 - P + 1)), b"var_out_dev overlaps sigma_in_dev"),
              (dict(tab, lay=Lay(obs_dim=0)), b"obs_dim must be 1..12 when table_dev is given"),
              (dict(tab, lay=Lay(obs_dim=13)), b"obs_dim must be 1..12 when table_dev is given")]
    seen = set()
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.os2rx_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(b"os2rx_cem_update: "), (kw.keys(), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases}) == 39                  # each cause has a text of its own
    assert not any(buf)                                                   # a refused call wrote nothing
    # the edges are taken: the next refusal is about something else (no call here is let through to a device)
    edges = [dict(shift=0), dict(shift=K), dict(flags=1), dict(E=S), dict(gain=5e-324), dict(sgain=5e-324), dict(lo=5e-324), dict(hi=1.7e308),
             dict(lo=1.0, hi=1.0), dict(lo=0.0, hi=0.0), dict(K=65535, nout=at(2 ** 27), var=at(2 ** 28)),
             dict(dtype=F32, gain=1.2e-38), dict(dtype=F32, lo=0.0, hi=3.4e38), dict(dtype=F32, act=at(65)),
             dict(nout=at(1024 - P), var=at(3000)), dict(var=at(S * M)), dict(var=at(1200 + 2 * M)), dict(sout=at(1200)), dict(sout=at(1300))]
    for kw in edges:
        kw = dict(kw, table=at(3500), lay=Lay(kw.pop("dtype", abi.F64), obs_dim=0))           # the last check refuses
        assert call(**kw) == abi.ERR_INVALID and lib.os2rx_last_error().endswith(b"when table_dev is given"), kw
    assert not any(buf)
    texts = checks_before_the_device("os2r_cem_capi.hip", name, ("layout_refusal",))
    assert len(texts) == 39 and all(any(t.encode() in e for e in seen) for t in texts)


# ---------------------------------------------------------------------------------------
# the Python layer, without a device
# ---------------------------------------------------------------------------------------
def _bare(dtype, n=8, nq=3, D=4):
    """A HipSim that never met a device: enough of it for the checks that run before the library is called."""
    import torch
    from gym_os2r_amd.sim import HipSim
    s = HipSim.__new__(HipSim)
    s.N, s.nq, s.D, s.dtype, s.device = n, nq, D, dtype, torch.device("cpu")
    s._h = None
    s._lib = None      # (and it has no cfg: filling the layout would raise AttributeError, not ValueError)
    return s


def test_python_argument_errors_need_no_device():
    import torch
    from gym_os2r_amd.sim import HipSim
    assert callable(HipSim.cem_update) and callable(HipSim.cem_update_into)
    f64 = torch.float64
    s = _bare(f64)
    K, M, S, D = 3, 4, 2, 4
    N = S * M
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    ret, act, nom, sig, out, var, sout = z(N), z(K, N, 2), z(K, M, 2), z(2, M), z(K, M, 2), z(K, M, 2), z(2, M)
    ok = dict(samples=S, elites=1)

    def into(*args, **kw):
        with pytest.raises(ValueError, match="^cem_update: "):
            s.cem_update_into(*args, **dict(ok, **kw))

    def whole(*args, **kw):
        with pytest.raises(ValueError, match="^cem_update: "):
            s.cem_update(*args, **dict(ok, **kw))
    full = (ret, act, nom, sig, out, var, sout)
    surface = (ret, act, nom, z(M, 2))
    for bad in (0, -1, 3, 2.0, True, None, "2"):
        into(*full, samples=bad)
        whole(*surface, samples=bad)
    for bad in (0, -1, S + 1, 1.0, True, None, "1"):
        into(*full, elites=bad)
        whole(*surface, elites=bad)
    for name in ("gain", "sigma_gain"):
        for bad in (0.0, -1.0, 1.5, float("nan"), float("inf"), "x", None):
            into(*full, **{name: bad})
            whole(*surface, **{name: bad})
    for kw in (dict(sigma_min=-0.1), dict(sigma_min=float("nan")), dict(sigma_max=float("inf")), dict(sigma_min=0.5, sigma_max=0.25),
               dict(sigma_max=-1.0), dict(sigma_min="x"), dict(sigma_max=None)):
        into(*full, **kw)
        whole(*surface, **kw)
    for bad in (-1, K + 1, 1.0, True, None):
        into(*full, shift=bad)
        whole(*surface, shift=bad)
    for bad in ("keep", 0, None):
        into(*full, tail=bad)
        whole(*surface, tail=bad)
    for i in range(len(full)):
        into(*[None if j == i else t for j, t in enumerate(full)])
    for args in ((z(N + 1), act, nom, sig, out, var, sout), (ret.float(), act, nom, sig, out, var, sout), (ret, z(K, N, 3), nom, sig, out, var, sout),
                 (ret, z(K, N), nom, sig, out, var, sout), (ret, act.numpy(), nom, sig, out, var, sout), (ret, act, z(K, M + 1, 2), sig, out, var, sout),
                 (ret, act, nom, z(M, 2), out, var, sout), (ret, act, nom, z(M, 2).t(), out, var, sout), (ret, act, nom, sig, z(K, M, 2).float(), var, sout),
                 (ret, act, nom, sig, out, z(M, K, 2).permute(1, 0, 2), sout), (ret, act, nom, sig, out, var, z(M, 2)),
                 (ret, z(2, K, N).permute(1, 2, 0), nom, sig, out, var, sout), (ret, act, nom, sig, nom, var, sout), (ret, act, nom, sig, out, nom, sout)):
        into(*args)
    for kw in (dict(applied=z(M)), dict(applied=z(M, 2).float()), dict(table=z(N, K, 2, D + 1)), dict(table=z(K, 2, D, N)),
               dict(lane_sigma=z(N, 2)), dict(lane_sigma=z(2, N).float()), dict(elite=z(S, M)), dict(elite=torch.zeros(M, S, dtype=torch.int32)),
               dict(threshold=z(M, 1)), dict(count=z(M)), dict(count=torch.zeros(M, dtype=torch.int64))):
        into(*full, **kw)
    for args in ((ret, None, nom, z(M, 2)), (ret, act, None, z(M, 2)), (ret, act, nom, None), (ret, act, z(K, M + 1, 2), z(M, 2)),
                 (ret, act, nom.float(), z(M, 2)), (ret, act, nom, z(2, M)), (ret, act, nom, z(M + 1, 2)), (ret, act, nom, "wide"),
                 (None, act, nom, z(M, 2)), (z(N - 1), act, nom, z(M, 2))):
        whole(*args)
    for bad in (z(K, 2, D + 1, N), z(N, K, 2, D + 1), z(K, 2, D + 1, N).permute(3, 0, 1, 2).float(), z(K, 2, D, N).permute(3, 0, 1, 2), "yes", 1):
        whole(*surface, table=bad)
