"""libos2r_pf.so (include/os2r_pf.h): the host side -- the numpy restatement of the update the GPU tests compare with (`restate_pf`)
on crafted inputs that reach every branch of it (`crafted_pf`) and on weights for which every operation is exact, the header
against the one table of gym_os2r_amd/pf.py, the exports of the library, the other six libraries as they were, the resources of
the two kernels in the built library, every refusal of os2rp_pf_update through ctypes without a device, and the argument checks
of HipSim.pf_update that need no device.  No GPU needed."""
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

NAMES = ["os2rp_abi_version", "os2rp_last_error", "os2rp_pf_update"]
CHUNKS = 8
MAX_OBS = 12
BRANCH_SHAPE = (130, 19, 10)            # M, S, D: three workgroups with a tail, S no multiple of 8
RATIO = 0.5
CLASSES = ("generic", "none valid", "one valid", "special logw", "equal", "dominant", "u = 0", "u next below 1")
FAR = 1e3                               # the offset whose squared distance underflows exp to 0


# ---------------------------------------------------------------------------------------
# the restatement of include/os2r_pf.h (needs no device)
# ---------------------------------------------------------------------------------------
def chunked(x, dtype):
    """Step 6: the sum of x [S, ...] over s in eight partials, partial c adding s = c, c + 8, ... in ascending order onto 0."""
    p = []
    for c in range(CHUNKS):
        acc = np.zeros(x.shape[1:], dtype)
        for s in range(c, x.shape[0], CHUNKS):
            acc = acc + x[s]
        p.append(acc)
    return ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))


def exp_argument(obs, meas, prec, logw_in, S, dtype):
    """Steps 1-5 up to the exp: -> (valid [S, M], count [M] int32, the argument l_s - lmax [S, M] in `dtype`, bit for bit; 0 where
    the particle is not valid)."""
    y = np.asarray(meas).astype(dtype)
    M, D = y.shape
    o = np.asarray(obs).astype(dtype).reshape(S, M, D)
    p = np.asarray(prec).astype(dtype)
    with np.errstate(all="ignore"):
        d2 = np.zeros((S, M), dtype)
        for i in range(D):
            diff = o[:, :, i] - y[None, :, i]
            d2 = d2 + (diff * diff) * p[i]
        lw = np.zeros((S, M), dtype) if logw_in is None else np.asarray(logw_in).astype(dtype).reshape(S, M)
        l = lw - dtype(0.5) * d2
        valid = np.isfinite(l)
        count = valid.sum(0).astype(np.int32)
        lmax = np.where(valid, l, -np.inf).max(0)
        lmax = np.where(count > 0, lmax, 0).astype(dtype)
        arg = (np.where(valid, l, lmax[None]) - lmax[None]).astype(dtype)
    assert arg.dtype == dtype and d2.dtype == dtype
    return valid, count, arg


def ancestors(w, u, dtype):
    """Step 11 for one robot: w [S] its weights, u its offset as given -> a [S], the ancestor of every slot."""
    S = len(w)
    w = np.asarray(w).astype(dtype)
    u = dtype(u)
    with np.errstate(all="ignore"):
        u = u if np.isfinite(u) and dtype(0) <= u < dtype(1) else dtype(0.5)
    c = np.empty(S, dtype)
    c[0] = w[0]
    for s in range(1, S):
        c[s] = c[s - 1] + w[s]
    step = c[S - 1] / dtype(S)
    last = int(np.nonzero(w > 0)[0][-1])
    a = np.empty(S, np.int64)
    for n in range(S):
        t = (dtype(n) + u) * step
        over = np.nonzero(c > t)[0]
        a[n] = over[0] if len(over) else last
    assert step.dtype == dtype and t.dtype == dtype
    return a


def restate_pf(obs, meas, prec, logw_in=None, u=None, *, S, ratio, dtype, weights=None):
    """include/os2r_pf.h, steps 1-11, in numpy and in `dtype`.  weights [S, M]: the device's own (its exp is within a few ulp of
    numpy's, not the same bits); None: numpy's exp.  -> dict(logw_out [S, M], index [S M] int32, est [M, D], weights [S, M],
    ess [M], count [M] int32, resampled [M] int32, wsum [M], Q [M])."""
    valid, count, arg = exp_argument(obs, meas, prec, logw_in, S, dtype)
    y = np.asarray(meas).astype(dtype)
    M, D = y.shape
    o = np.asarray(obs).astype(dtype).reshape(S, M, D)
    with np.errstate(all="ignore"):
        if weights is None:
            weights = np.where(valid, np.exp(arg), 0).astype(dtype)
        w = np.asarray(weights).astype(dtype).reshape(S, M)
        wsum = chunked(w, dtype)
        Q = chunked((w * w).astype(dtype), dtype)
        E = chunked(np.where(valid[:, :, None], w[:, :, None] * o, 0).astype(dtype), dtype)
        some = count > 0
        ess = np.where(some, (wsum * wsum) / Q, 0).astype(dtype)
        est = np.where(some[:, None], E / wsum[:, None], y).astype(dtype)
        below = ess < dtype(ratio) * dtype(S)
    resampled = (some & (below | (count < S))).astype(np.int32)
    minus_inf = dtype(-np.inf)
    logw_out = np.where(valid, arg, minus_inf).astype(dtype)
    logw_out[:, ~some] = 0
    logw_out[:, resampled == 1] = 0
    index = np.full((S, M), -1, np.int32)
    offsets = np.full(M, 0.5) if u is None else np.asarray(u)
    for m in np.nonzero(resampled)[0]:
        index[:, m] = ancestors(w[:, m], offsets[m], dtype) * M + m
    assert all(x.dtype == dtype for x in (wsum, Q, E, ess, est, logw_out))
    return dict(logw_out=logw_out, index=index.reshape(-1), est=est, weights=w, ess=ess, count=count, resampled=resampled, wsum=wsum, Q=Q)


def crafted_pf(M, S, D, seed=0, dtype=np.float64):
    """Inputs in float64 (the caller rounds; u is made in `dtype`, so that the value next below 1 stays below 1) that reach every
    branch.  meas in -1..1, prec in 0.5..2 with the last entry 0 where D > 1, logw in -1..0 and, by robot class m % 8 (CLASSES):
      0  generic: the particles lie about the measurement, tightly for m % 16 == 0 (no resampling at RATIO) and widely for
         m % 16 == 8 (resampling), where u is also outside [0, 1) or NaN: taken as 0.5
      1  every particle invalid (a NaN in its observation): the robot is lost
      2  exactly one valid particle, s = m % S
      3  a logw of +inf, -inf and NaN in turn on the particles s % 3 == 0 (every one of them with S = 1)
      4  equal observations and equal logw: equal weights, ess = S
      5  one particle, s = (m // 8) % S, at the measurement and all the others FAR away: their weights underflow to 0
      6  as 0 wide, u = 0
      7  as 0 wide, u the number next below 1
    -> dict(obs [N, D], meas [M, D], prec [D], logw [S, M], u [M])"""
    rng = np.random.default_rng(seed)
    meas = rng.uniform(-1.0, 1.0, (M, D))
    prec = rng.uniform(0.5, 2.0, D)
    if D > 1:
        prec[D - 1] = 0.0
    m = np.arange(M)
    cls = m % 8
    tight = (m % 16 == 0)
    scale = np.where(tight, 0.1, 2.0)
    obs = meas[None] + rng.normal(0.0, 1.0, (S, M, D)) * scale[None, :, None]
    logw = rng.uniform(-1.0, 0.0, (S, M))
    u = rng.uniform(0.0, 1.0, M).astype(dtype)
    u[m % 32 == 8] = 1.5
    u[m % 32 == 24] = np.nan
    obs[:, cls == 1, 0] = np.nan
    for r in m[cls == 2]:
        obs[np.arange(S) != r % S, r, D - 1] = np.nan
    for k, bad in enumerate((np.inf, -np.inf, np.nan)):
        logw[np.ix_(np.arange(S) % 9 == 3 * k, cls == 3)] = bad
    obs[:, cls == 4] = obs[0, cls == 4][None]
    logw[:, cls == 4] = -0.25
    for r in m[cls == 5]:
        obs[:, r] = meas[r]
        obs[np.arange(S) != (r // 8) % S, r, 0] += FAR
    u[cls == 6] = 0.0
    u[cls == 7] = np.nextafter(dtype(1), dtype(0))
    return dict(obs=obs.reshape(S * M, D), meas=meas, prec=prec, logw=logw, u=u)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_on_crafted_inputs_that_reach_every_branch(dtype):
    from gym_os2r_amd import pf
    header = _header("os2r_pf.h")
    assert CHUNKS == pf.CHUNKS == int(re.search(r"#define OS2RP_CHUNKS (\d+)", header).group(1))
    assert MAX_OBS == pf.MAX_OBS == abi.MAX_OBS
    M, S, D = BRANCH_SHAPE
    c = crafted_pf(M, S, D, dtype=dtype)
    out = restate_pf(c["obs"], c["meas"], c["prec"], c["logw"], c["u"], S=S, ratio=RATIO, dtype=dtype)
    m = np.arange(M)
    cls = m % 8
    w, count, res, index = out["weights"], out["count"], out["resampled"], out["index"].reshape(S, M)
    valid, _, arg = exp_argument(c["obs"], c["meas"], c["prec"], c["logw"], S, dtype)
    meas = c["meas"].astype(dtype)
    assert S > CHUNKS and S % CHUNKS and M > 2 * 64 and M % 64               # every partial holds something; a tail workgroup
    # invalid particles: weight exactly 0, counted out, -inf in logw_out where the robot keeps its particles; the maximum has weight 1
    assert (w[~valid] == 0).all() and (w.max(0)[count > 0] == 1).all() and np.array_equal(count, valid.sum(0))
    keep = (res == 0) & (count > 0)
    assert keep.any() and np.array_equal(out["logw_out"][:, keep], np.where(valid, arg, -np.inf)[:, keep])
    assert (index[:, res == 0] == -1).all() and (out["logw_out"][:, res == 1] == 0).all() and (out["logw_out"].max(0) == 0).all()
    # an invalid particle is never an ancestor, and every ancestor is a particle of the same robot
    anc = index[:, res == 1]
    assert (anc >= 0).all() and np.array_equal(anc % M, np.broadcast_to(m[res == 1], anc.shape))
    assert valid[anc // M, anc % M].all() and (w[anc // M, anc % M] > 0).all() and (np.diff(anc, axis=0) >= 0).all()
    # the lost robots: nothing valid, index -1, est = meas, ess 0, logw_out 0
    lost = cls == 1
    assert (count[lost] == 0).all() and (res[lost] == 0).all() and (index[:, lost] == -1).all() and (out["ess"][lost] == 0).all()
    assert np.array_equal(out["est"][lost], meas[lost]) and (out["logw_out"][:, lost] == 0).all() and ((count == 0) == lost).all()
    # one valid particle: every slot picks it
    one = cls == 2
    assert (count[one] == 1).all() and (res[one] == 1).all() and np.array_equal(index[:, one] // M, np.tile(m[one] % S, (S, 1)))
    assert np.array_equal(out["est"][one], c["obs"].astype(dtype).reshape(S, M, D)[m[one] % S, m[one]]) and (out["ess"][one] == 1).all()
    # special logw: +inf, -inf and NaN are all invalid, the robot resamples for that reason
    sp = cls == 3
    lw = c["logw"][:, sp]
    assert np.isposinf(lw).any() and np.isneginf(lw).any() and np.isnan(lw).any() and (count[sp] == np.isfinite(lw).sum(0)).all()
    assert (res[sp] == 1).all() and (0 < count[sp]).all() and (count[sp] < S).all()
    # equal weights: ess = S exactly, no resampling at any ratio <= 1
    eq = cls == 4
    assert (w[:, eq] == 1).all() and (out["ess"][eq] == S).all() and (res[eq] == 0).all() and (out["wsum"][eq] == S).all()
    # (the mean of S equal values: at most six rounded adds on a path of the tree and one division, each within eps / 2)
    assert np.allclose(out["est"][eq], c["obs"].astype(dtype).reshape(S, M, D)[0, eq], rtol=4 * np.finfo(dtype).eps, atol=0)
    # one dominant particle: valid lanes with weight exactly 0, every slot picks the dominant one
    dom = cls == 5
    assert (count[dom] == S).all() and (w[:, dom].sum(0) == 1).all() and (res[dom] == 1).all() and (out["ess"][dom] == 1).all()
    assert np.array_equal(index[:, dom] // M, np.tile((m[dom] // 8) % S, (S, 1)))
    # generic: tight robots keep, wide robots resample; u outside [0, 1) or NaN is 0.5
    assert (res[m % 16 == 0] == 0).all() and (res[(cls == 0) & (m % 16 == 8)] == 1).all() and (count[cls == 0] == S).all()
    half = restate_pf(c["obs"], c["meas"], c["prec"], c["logw"], np.where(np.isin(m % 32, (8, 24)), 0.5, c["u"]), S=S, ratio=RATIO, dtype=dtype)
    assert np.array_equal(half["index"], out["index"]) and np.isnan(c["u"]).any() and (c["u"] > 1).any()
    # u = 0 and u next below 1 are taken as they are: slot 0 of u = 0 is the first particle with a positive weight
    assert (c["u"][cls == 6] == 0).all() and (c["u"][cls == 7] < 1).all() and (c["u"][cls == 7] + np.finfo(dtype).epsneg == 1).all()
    assert (res[cls == 6] == 1).all() and (res[cls == 7] == 1).all()
    first = np.array([np.nonzero(w[:, r] > 0)[0][0] for r in m[cls == 6]])
    assert np.array_equal(index[0, cls == 6] // M, first)
    # the device's own weights handed back give the same
    again = restate_pf(c["obs"], c["meas"], c["prec"], c["logw"], c["u"], S=S, ratio=RATIO, dtype=dtype, weights=w)
    assert all(np.array_equal(again[k], out[k], equal_nan=True) for k in out)
    # null logw and null u: zeros and 0.5
    null = restate_pf(c["obs"], c["meas"], c["prec"], S=S, ratio=RATIO, dtype=dtype)
    full = restate_pf(c["obs"], c["meas"], c["prec"], np.zeros((S, M)), np.full(M, 0.5), S=S, ratio=RATIO, dtype=dtype)
    assert all(np.array_equal(null[k], full[k], equal_nan=True) for k in out)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_resample_ratio_zero_resamples_exactly_the_robots_with_an_invalid_particle(dtype):
    M, S, D = BRANCH_SHAPE
    c = crafted_pf(M, S, D, dtype=dtype)
    out = restate_pf(c["obs"], c["meas"], c["prec"], c["logw"], c["u"], S=S, ratio=0.0, dtype=dtype)
    count = out["count"]
    assert np.array_equal(out["resampled"] == 1, (count > 0) & (count < S)) and (out["resampled"] == 1).any()
    assert ((count == S) & (out["ess"] < 2)).any()                            # a degenerate robot that ratio 0 leaves alone
    always = restate_pf(c["obs"], c["meas"], c["prec"], c["logw"], c["u"], S=S, ratio=2.0, dtype=dtype)
    assert np.array_equal(always["resampled"] == 1, count > 0)
    # equal weights, resampled (ratio 2) with any u: the identity
    eq = np.arange(M) % 8 == 4
    lanes = np.arange(S * M).reshape(S, M)
    assert np.array_equal(always["index"].reshape(S, M)[:, eq], lanes[:, eq])
    # ... for every u whose rounded sum n + u stays below n + 1 in every slot n < S = 19 < 32: up to 1 - 32 eps.  (Closer to 1
    # the one rounded add of step 11 gives n + 1 in the higher slots, t_n = c_n, and slot n takes particle n + 1: the
    # contract's arithmetic, which the last assertion states for the number next below 1.)
    eps = float(np.finfo(dtype).eps)
    for u in (0.0, 2.0 ** -30, 0.25, 0.5, 0.999, 1.0 - 32 * eps):
        assert np.array_equal(ancestors(np.ones(S), u, dtype), np.arange(S)), u
        assert np.array_equal(ancestors(np.full(S, 0.375), u, dtype), np.arange(S)), u
    edge = ancestors(np.ones(S), float(np.nextafter(dtype(1), dtype(0))), dtype)
    assert np.array_equal(edge, np.minimum(np.arange(S) + (np.arange(S) > 0), S - 1)), edge


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dyadic_weights_give_every_ancestor_its_share_within_one(dtype):
    """Weights that are powers of two, S = 16 and a dyadic u: every prefix, the step and every threshold are exact, and systematic
    resampling gives ancestor s floor or ceil of S w_s / wsum offspring."""
    rng = np.random.default_rng(4)
    S = 16
    for trial in range(40):
        w = 2.0 ** -rng.integers(0, 6, S)
        w[rng.integers(0, S, 3)] = 0.0
        w[rng.integers(0, S)] = 1.0
        u = float(rng.integers(0, 8)) / 8
        a = ancestors(w, u, dtype)
        share = S * w / w.sum()
        got = np.bincount(a, minlength=S)
        assert got.sum() == S and (np.abs(got - share) < 1).all() and (got[w == 0] == 0).all(), (trial, w, u, got)
        assert (np.diff(a) >= 0).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("S", [1, 3, 5, 8])
def test_short_partials_are_the_sum_written_out_by_hand(S, dtype):
    """S <= 8: a partial holds one term or none, an empty one adds 0, and the tree is the left-to-right sum of the pairs."""
    M, D = 9, 4
    c = crafted_pf(M, S, D, seed=S, dtype=dtype)
    out = restate_pf(c["obs"], c["meas"], c["prec"], c["logw"], c["u"], S=S, ratio=RATIO, dtype=dtype)
    w = out["weights"]
    by_hand = {1: lambda x: x[0], 3: lambda x: (x[0] + x[1]) + x[2], 5: lambda x: ((x[0] + x[1]) + (x[2] + x[3])) + x[4],
               8: lambda x: ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]))}[S]
    assert np.array_equal(out["wsum"], by_hand(w)) and np.array_equal(out["Q"], by_hand(w * w)) and out["wsum"].dtype == dtype
    o = c["obs"].astype(dtype).reshape(S, M, D)
    with np.errstate(all="ignore"):
        terms = np.where(np.isnan(o), 0, w[:, :, None] * o)
        E = by_hand(terms.astype(dtype))
        mean = E / out["wsum"][:, None]
    some = out["count"] > 0
    assert np.array_equal(out["est"][some], mean[some]) and some.any()
    if S == 1:
        assert np.array_equal(out["est"][some], o[0][some]) and (out["resampled"] == 0).all() and (out["index"] == -1).all()


# ---------------------------------------------------------------------------------------
# header, table, exports
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import control, pf
    protos = _prototypes("os2r_pf.h", "os2rp")
    assert [p[0] for p in protos] == list(pf.ENTRY_POINTS) == NAMES
    lib = pf.load()
    for name, ret, args in protos:
        argtypes = pf.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2rp_last_error" else C.c_int)
    args = protos[2][2]
    assert args[0] == "const Os2rControlLayout* layout" and args[1] == "int64_t nrobots" and args[2] == "int32_t nparticles"
    assert args[8] == "double resample_ratio" and args[10] == "int32_t* index_dev" and args[-1] == "void* stream" and len(args) == 17
    assert pf.ENTRY_POINTS["os2rp_pf_update"][8] is C.c_double and pf.ENTRY_POINTS["os2rp_pf_update"][1] is C.c_int64
    header = _header("os2r_pf.h")
    assert re.search(r"#define OS2R_PF_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert lib.os2rp_abi_version() == pf.ABI_VERSION == 1
    assert pf.Os2rControlLayout is control.Os2rControlLayout and pf.layout is control.layout
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", pf.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)


def test_the_other_libraries_are_as_they_were():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib, control, mppi, pf, search, steer
    tables = {_lib.LIB_PATH: _lib.ENTRY_POINTS, _lib.RECORD_LIB_PATH: _lib.RECORD_ENTRY_POINTS, control.LIB_PATH: control.ENTRY_POINTS,
              search.LIB_PATH: search.ENTRY_POINTS, steer.LIB_PATH: steer.ENTRY_POINTS, mppi.LIB_PATH: mppi.ENTRY_POINTS}
    others = set().union(*tables.values())
    assert len(tables) == 6 and not set(pf.ENTRY_POINTS) & others and not any(name.startswith("os2rp_") for name in others)
    for name in ("os2r.h", "os2r_control.h", "os2r_record.h", "os2r_search.h", "os2r_steer.h", "os2r_mppi.h"):
        assert "os2rp_" not in _header(name) and "os2r_pf" not in _header(name).lower(), name
    assert len(_lib.ENTRY_POINTS) == 35 and len(_lib.RECORD_ENTRY_POINTS) == 3
    assert list(control.ENTRY_POINTS) == ["os2rc_abi_version", "os2rc_last_error", "os2rc_ilqr_backward"]
    assert list(search.ENTRY_POINTS) == ["os2rs_abi_version", "os2rs_last_error", "os2rs_ilqr_line_search"]
    assert list(steer.ENTRY_POINTS) == ["os2rt_abi_version", "os2rt_last_error", "os2rt_ilqr_backward_mu", "os2rt_ilqr_steer"]
    assert list(mppi.ENTRY_POINTS) == ["os2rm_abi_version", "os2rm_last_error", "os2rm_mppi_update"]
    for path, table in tables.items():
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(table), path
        kernels = kernel_meta.kernel_meta(path)
        assert kernels and not any("pf_update" in k for k in kernels), path


def test_kernel_resources():
    """Exactly two kernels, float and double, are in the built library and neither uses scratch: private_segment_fixed_size 0, no
    VGPR or SGPR spill and no AGPRs in the code-object metadata.  The LDS of a workgroup does not depend on S (the kernel has no
    dynamic LDS: the launch passes 0): [8 waves][64 robots] partials of wsum, Q and the at most 12 E_i, the [8][64] maxima and
    int32 counts of pass 1 and the 12 precisions, (12 + 3) 8 64 sizeof(T) + 8 64 4 + 12 sizeof(T) bytes -- 63584 for double: two
    workgroups fit the 160 KiB of a CU, and with at most 128 registers their sixteen waves fit its register file."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import pf
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(pf.LIB_PATH)
    meta = kernel_meta.kernel_meta(pf.LIB_PATH)
    assert len(meta) == 2, sorted(meta)
    for real, size in (("float", 4), ("double", 8)):
        (name,) = [k for k in meta if f"pf_update_kernel<{real}>" in k]
        m = meta[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
        assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 128, (name, m)
        bound = (MAX_OBS + 3) * CHUNKS * 64 * size + CHUNKS * 64 * 4 + MAX_OBS * size
        assert 0 < m["group_segment_fixed_size"] <= bound and 2 * bound <= 160 * 1024, (name, m, bound)
    src = open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "os2r_pf_inst.hip")).read()
    assert "hipLaunchKernelGGL((pf_update_kernel<T>), grid, block, 0, s, p)" in src         # no dynamic LDS


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def test_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import control, pf
    lib = pf.load()
    M, S, D = 4, 2, 4
    buf = (C.c_double * 4096)()
    base = C.addressof(buf)
    at = lambda i: C.c_void_p(base + 8 * i)
    nan, inf = float("nan"), float("inf")

    def Lay(dtype=abi.F64, **kw):
        lay = control.layout(dtype, 3, 0, [0, 1, 3, -1])
        for k, v in kw.items():
            setattr(lay, k, v)
        return C.byref(lay)
    good = dict(lay=Lay(), M=M, S=S, obs=at(0), meas=at(64), prec=at(128), lin=at(1024), u=at(256), ratio=0.5, lout=at(1024 + S * M),
                index=at(2048), est=None, w=None, ess=None, count=None, res=None)
    name = "os2rp_pf_update"
    assert len(good) + 1 == len(pf.ENTRY_POINTS[name])

    def call(**kw):
        a = dict(good, **kw)
        return lib.os2rp_pf_update(*[a[k] for k in good], None)
    assert lib.os2rp_pf_update(*[None if _is_pointer(t) else 0 for t in pf.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rp_last_error() == b"os2rp_pf_update: null layout"
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"layout->dtype must be OS2R_F32 or OS2R_F64"),
             (dict(lay=Lay(nq=1)), b"layout->nq must be 2..5"), (dict(lay=Lay(nq=6)), b"layout->nq must be 2..5"),
             (dict(lay=Lay(obs_dim=0)), b"layout->obs_dim must be 1..12"), (dict(lay=Lay(obs_dim=13)), b"layout->obs_dim must be 1..12"),
             (dict(M=0), b"nrobots must be >= 1"), (dict(M=-1), b"nrobots must be >= 1"), (dict(S=0), b"nparticles must be >= 1"),
             (dict(S=-2), b"nparticles must be >= 1"), (dict(M=2 ** 62), b"nparticles * nrobots exceeds 2^31 - 1"),
             (dict(M=2 ** 30, S=2), b"nparticles * nrobots exceeds 2^31 - 1"),
             (dict(ratio=nan), b"resample_ratio must be finite"), (dict(ratio=inf), b"resample_ratio must be finite"),
             (dict(ratio=-inf), b"resample_ratio must be finite"), (dict(ratio=-0.5), b"resample_ratio must be >= 0"),
             (dict(ratio=-5e-324), b"resample_ratio must be >= 0"),
             (dict(obs=None), b"null obs_dev"), (dict(meas=None), b"null meas_dev"), (dict(prec=None), b"null prec_dev"),
             (dict(lout=None), b"null logw_out_dev"), (dict(index=None), b"null index_dev"),
             (dict(lout=at(1024)), b"logw_out_dev overlaps logw_in_dev"), (dict(lout=at(1024 + S * M - 1)), b"logw_out_dev overlaps logw_in_dev"),
             (dict(lout=at(1024 - S * M + 1)), b"logw_out_dev overlaps logw_in_dev"),
             # (arrays whose ends wrap round at the top of the address space: the check is on the distance)
             (dict(M=2 ** 31 - 1, S=1, lin=C.c_void_p(2 ** 64 - 65), lout=C.c_void_p(2 ** 64 - 33)), b"logw_out_dev overlaps logw_in_dev")]
    seen = set()
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.os2rp_last_error()
        assert rc == abi.ERR_INVALID and err == b"os2rp_pf_update: " + msg, (kw.keys(), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases}) == 15                  # each cause has a text of its own
    assert not any(buf)                                                   # a refused call wrote nothing
    # the edges are taken: the next refusal is about something else (no call here is let through to a device)
    edges = [dict(ratio=0.0), dict(ratio=-0.0), dict(ratio=1.7e308), dict(dtype=abi.F32, ratio=1e300), dict(lay=Lay(obs_dim=1)),
             dict(lay=Lay(obs_dim=12)), dict(M=2 ** 31 - 1, S=1), dict(M=1, S=2 ** 31 - 1), dict(lin=None, lout=at(1024)),
             dict(lout=at(1024 - S * M))]
    for kw in edges:
        if "dtype" in kw:
            kw = dict(kw, lay=Lay(kw.pop("dtype")))
        kw = dict(kw, index=None)                                           # the last check but one refuses
        if kw.get("lin", 1) is not None and "lout" not in kw:
            kw["lout"] = at(1024 + S * M)
        assert call(**kw) == abi.ERR_INVALID and lib.os2rp_last_error() == b"os2rp_pf_update: null index_dev", kw
    assert call(lout=at(1024 + S * M), index=None) == abi.ERR_INVALID and lib.os2rp_last_error().endswith(b"null index_dev")
    assert not any(buf)
    texts = checks_before_the_device("os2r_pf_capi.hip", name, ("layout_refusal",))
    assert len(texts) == 15 and {("os2rp_pf_update: " + t).encode() for t in texts} == seen


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
    assert callable(HipSim.pf_update) and callable(HipSim.pf_update_into)
    f64 = torch.float64
    s = _bare(f64)
    M, S, D = 4, 2, 4
    N = S * M
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    obs, meas, prec, lout, index = z(N, D), z(M, D), z(D), z(S, M), z(N, dtype=torch.int32)
    ok = dict(particles=S)

    def into(*args, **kw):
        with pytest.raises(ValueError, match="^pf_update: "):
            s.pf_update_into(*args, **dict(ok, **kw))

    def whole(*args, **kw):
        with pytest.raises(ValueError, match="^pf_update: "):
            s.pf_update(*args, **dict(ok, **kw))
    for bad in (0, -1, 3, 2.0, True, None, "2"):
        into(obs, meas, prec, lout, index, particles=bad)
        whole(obs, meas, prec, particles=bad)
    for bad in (-0.5, float("nan"), float("inf"), "x", None, True):
        into(obs, meas, prec, lout, index, resample_ratio=bad)
        whole(obs, meas, prec, resample_ratio=bad)
    for args in ((None, meas, prec, lout, index), (obs, None, prec, lout, index), (obs, meas, None, lout, index), (obs, meas, prec, None, index),
                 (obs, meas, prec, lout, None), (z(N + 1, D), meas, prec, lout, index), (z(N, D + 1), meas, prec, lout, index),
                 (obs.float(), meas, prec, lout, index), (obs.numpy(), meas, prec, lout, index), (z(D, N).t(), meas, prec, lout, index),
                 (obs, z(M + 1, D), prec, lout, index), (obs, meas, z(D + 1), lout, index), (obs, meas, prec.float(), lout, index),
                 (obs, meas, prec, z(M, S), index), (obs, meas, prec, lout, z(N, dtype=torch.int64)), (obs, meas, prec, lout, z(N + 1, dtype=torch.int32))):
        into(*args)
    for kw in (dict(logw_in=z(M, S)), dict(logw_in=lout), dict(logw_in=z(S, M).float()), dict(u=z(M, 1)), dict(u=z(M).float()), dict(est=z(M)),
               dict(est=z(M, D).float()), dict(weights=z(M, S)), dict(ess=z(M, 1)), dict(count=z(M)), dict(count=torch.zeros(M, dtype=torch.int64)),
               dict(resampled=z(M)), dict(resampled=torch.zeros(M + 1, dtype=torch.int32))):
        into(obs, meas, prec, lout, index, **kw)
    for args in ((None, meas, prec), (obs, None, prec), (obs, meas, None), (z(N - 1, D), meas, prec), (obs, z(M, D + 1), prec), (obs, meas, prec.float())):
        whole(*args)
    for kw in (dict(logw=z(M, S)), dict(logw=z(S, M).float()), dict(u=z(M + 1)), dict(u="x")):
        whole(obs, meas, prec, **kw)
