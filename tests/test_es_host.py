"""libos2r_es.so (include/os2r_es.h): the host side -- the numpy restatement of the perturbation and of the ARS V1-t update the GPU
tests compare with (`restate_perturb`, `restate_update`), the directions on the CPU (`cpu_directions`: Box-Muller on the oracle's
uniform2 with the documented counter words), the crafted returns of the GPU tests (`crafted_es`) and the branches they reach, the
restatement against an independent plain statement (np.argsort, np.std, one einsum) in float64 and in float32 against its own
float64 result, the header against the one table of gym_os2r_amd/es.py, the exports of the library, the resources of the fourteen
kernels in the built library, every refusal of both entry points through ctypes without a device, and the argument checks of
HipSim.es_perturb / es_update that need no device.  No GPU needed."""
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
from header_check import HIP_CALL, _agrees, _csrc, _function, _header, _is_pointer, _prototypes  # noqa: E402

NAMES = ["os2ra_abi_version", "os2ra_last_error", "os2ra_es_perturb", "os2ra_es_update"]
CHUNKS = 64
STEP, FLOOR, NU = 0.02, 1e-8, 0.03
NONE_VALID, FLAT = 2, 3                 # the population without a valid direction (M > 2), the one whose returns are all equal (M > 3)
# (M, S) of the GPU tests (tests/test_gpu_es.py): one direction; fewer than 64 with empty partials; exactly 64 (the one-thread
# sum at its boundary) with every crafted population; the wave sum with one full round and one lane more; partials of up to
# three terms; two workgroups of populations in the one-thread sum; and, where the code takes its other paths (1 024 directions
# and more), two rounds of the sixteen-wave sum and two spans of the rank count, neither of them full
SHAPES = [(1, 1), (1, 3), (5, 64), (3, 65), (2, 130), (257, 2), (2, 1100)]
# The largest relative distance (the largest difference over the largest entry of the reference) measured on the CPU this test
# was written on, over SHAPES x D in (10, 3) x the tops of `tops`; the tests print them.  float64: of the restatement from the
# plain statement (np.argsort, np.std, np.einsum); float32: of the float32 restatement from the float64 one.  The bound is
# MARGIN x that.
MEASURED = {np.float64: dict(theta_new=9.375e-17, sigma_r=2.259e-16, grad=2.028e-15),
            np.float32: dict(theta_new=4.982e-8, sigma_r=4.409e-8, grad=1.379e-7)}
MARGIN = 8
FORBIDDEN = ("os2rg_", "os2r_pg", "os2rv_", "os2r_critic", "os2ro_", "os2r_ppo", "os2rn_", "os2r_npg", "os2rx_", "os2r_cem", "os2ru_", "os2r_ukf",
             "os2re_", "os2r_ekf", "os2rp_", "os2r_pf", "os2rm_", "mppi", "os2rt_", "steer", "line_search")


def tops(S):
    """top of the GPU tests: every direction (0), one, half of them rounded up, S itself and more than S."""
    return sorted({0, 1, (S + 1) // 2, S, 2 * S})


# ---------------------------------------------------------------------------------------
# the directions, and the restatement of include/os2r_es.h (need no device)
# ---------------------------------------------------------------------------------------
def cpu_directions(oracle, seed, pop_offset, generation, M, S, D):
    """delta [S M, 2, D+1] in float64, row s M + m: entry e = j (D + 1) + i of delta[m][s] is output e & 1 of Box-Muller on the
    oracle's uniform2(seed, (pop_offset + m) mod 2^32, 6, generation, 16 s + (e >> 1))."""
    from gym_os2r_amd import es
    n = D + 1
    u = np.array([oracle.uniform2(seed, (pop_offset + m) & 0xFFFFFFFF, es.STREAM, generation, 16 * s + q)
                  for s in range(S) for m in range(M) for q in range(n)])
    r = np.sqrt(-2.0 * np.log(1.0 - u[:, 0]))
    th = 6.283185307179586476925286766559 * u[:, 1]
    return np.stack([r * np.cos(th), r * np.sin(th)], axis=1).reshape(S * M, 2, n)


def restate_perturb(theta, delta, nu, *, S, dtype):
    """include/os2r_es.h, os2ra_es_perturb, in numpy and in `dtype` on a given delta [S M, 2, D+1]: p = nu delta rounded, then
    theta + p and theta - p.  -> weights [2 S M, 2, D+1]."""
    theta, delta = np.asarray(theta).astype(dtype), np.asarray(delta).astype(dtype)
    M = theta.shape[0]
    p = np.float64(nu).astype(dtype) * delta
    th = np.broadcast_to(theta[None], (S,) + theta.shape).reshape(S * M, *theta.shape[1:])
    out = np.concatenate([th + p, th - p])
    assert out.dtype == dtype
    return out


def chunked(chains, kept):
    """Step 3: a sum over the kept directions (kept [S, M] bool) in 64 partials and the adjacent-pair tree; partial c walks
    s = c, c + 64, ... in ascending order and adds, for each, the terms of `chains` ([S, M, ...] each) one after the other."""
    S = kept.shape[0]
    parts = []
    for c in range(CHUNKS):
        acc = np.zeros(chains[0].shape[1:], chains[0].dtype)
        for s in range(c, S, CHUNKS):
            k = kept[s].reshape(kept[s].shape + (1,) * (acc.ndim - 1))
            for term in chains:
                acc = np.where(k, acc + term[s], acc)
        parts.append(acc)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
    return parts[0]


def restate_update(returns, theta, delta, *, S, dtype, top=0, step_size=STEP, sigma_floor=FLOOR):
    """include/os2r_es.h, os2ra_es_update, steps 1-3, in numpy and in `dtype`, on a given delta [S M, 2, D+1] (the device's, or
    the CPU's).  returns [2 S M], theta [M, 2, D+1].
    -> dict(theta_new, grad [M, 2, D+1], sigma_r [M], count, used [M] int32, kept [S M] int32)."""
    returns, theta, delta = (np.asarray(a).astype(dtype) for a in (returns, theta, delta))
    M = theta.shape[0]
    E = theta.shape[1] * theta.shape[2]
    rp, rm = returns[:S * M].reshape(S, M), returns[S * M:].reshape(S, M)
    d = delta.reshape(S, M, E)
    step, floor, zero = np.float64(step_size).astype(dtype), np.float64(sigma_floor).astype(dtype), dtype(0)
    with np.errstate(all="ignore"):
        valid = np.isfinite(rp) & np.isfinite(rm)                                  # step 1
        count = valid.sum(0).astype(np.int32)
        score = np.where(valid, np.maximum(rp, rm), zero)
        kept = valid.copy()
        if 0 < top < S:                                                            # step 2, as the header's parenthesis says it
            s_idx = np.arange(S)
            for s in range(S):
                ahead = valid & ((score > score[s][None]) | ((score == score[s][None]) & (s_idx[:, None] < s)))
                kept[s] = valid[s] & (ahead.sum(0) < top)
        used = kept.sum(0).astype(np.int32)                                        # step 3
        some = used > 0
        n2, nb = (2 * used).astype(dtype), used.astype(dtype)
        safe_p, safe_m = np.where(kept, rp, zero), np.where(kept, rm, zero)        # (a return that is not kept touches no chain)
        mean = chunked([safe_p, safe_m], kept) / n2
        dp, dm = safe_p - mean[None], safe_m - mean[None]
        var = chunked([dp * dp, dm * dm], kept) / n2
        sigma = np.sqrt(var)
        sigma = np.where(sigma < floor, floor, sigma)
        diff = safe_p - safe_m
        g = chunked([diff[:, :, None] * d], kept)
        den = nb * sigma
        grad = np.where(some[:, None], g / den[:, None], zero)
        theta_new = np.where(some[:, None], theta.reshape(M, E) + step * grad, theta.reshape(M, E))
        sigma = np.where(some, sigma, zero)
    assert all(a.dtype == dtype for a in (theta_new, grad, sigma)) and all(a.dtype == np.int32 for a in (count, used))
    return dict(theta_new=theta_new.reshape(theta.shape), grad=grad.reshape(theta.shape), sigma_r=sigma, count=count, used=used,
                kept=kept.reshape(S * M).astype(np.int32))


def plain_update(returns, theta, delta, *, S, top=0, step_size=STEP, sigma_floor=FLOOR):
    """The independent statement in float64: per population a stable np.argsort of the negated scores of the valid directions
    (equal scores keep their order: the lower s first), np.std of the kept returns, one einsum."""
    returns, theta, delta = (np.asarray(a, np.float64) for a in (returns, theta, delta))
    M = theta.shape[0]
    rp, rm = returns[:S * M].reshape(S, M), returns[S * M:].reshape(S, M)
    d = delta.reshape(S, M, -1)
    out = dict(theta_new=theta.copy(), grad=np.zeros_like(theta), sigma_r=np.zeros(M), count=np.zeros(M, np.int32), used=np.zeros(M, np.int32),
               kept=np.zeros((S, M), np.int32))
    for m in range(M):
        idx = np.flatnonzero(np.isfinite(rp[:, m]) & np.isfinite(rm[:, m]))
        order = idx[np.argsort(-np.maximum(rp[idx, m], rm[idx, m]), kind="stable")]
        b = min(top or S, len(idx))
        keep = order[:b]
        out["count"][m], out["used"][m] = len(idx), b
        out["kept"][keep, m] = 1
        if b == 0:
            continue
        sigma = max(float(np.std(np.concatenate([rp[keep, m], rm[keep, m]]))), sigma_floor)
        grad = np.einsum("s,se->e", rp[keep, m] - rm[keep, m], d[keep, m]) / (b * sigma)
        out["sigma_r"][m] = sigma
        out["grad"][m] = grad.reshape(theta.shape[1:])
        out["theta_new"][m] = theta[m] + step_size * out["grad"][m]
    out["kept"] = out["kept"].reshape(S * M)
    return out


def crafted_es(M, S, D, dtype, seed=0):
    """The inputs of the GPU tests, in `dtype`.  The returns are small integers and halves (-3 .. 3 in steps of 1/2: every score is
    exact in both dtypes, and most scores tie).  By direction s and population m (where the shape reaches it):
      s % 7 == 3            r+ is a NaN
      s % 11 == 5           r- is +inf
      s % 13 == 6           r+ is -inf
      m == NONE_VALID (M > 2)   every r- is a NaN: the population has no valid direction
      m == FLAT (M > 3)         every return is 2.5: sigma_floor binds and the direction sum is 0
    -> dict(returns [2 S M], theta [M, 2, D+1])"""
    rng = np.random.default_rng(seed + 1000 * M + S)
    r = rng.integers(-6, 7, (2, S, M)).astype(np.float64) / 2.0
    s = np.arange(S)
    if M > 3:
        r[:, :, FLAT] = 2.5
    r[0, s % 7 == 3] = np.nan
    r[1, s % 11 == 5] = np.inf
    r[0, s % 13 == 6] = -np.inf
    if M > 2:
        r[1, :, NONE_VALID] = np.nan
    f = lambda a: np.ascontiguousarray(a.astype(dtype))
    return dict(returns=f(r.reshape(2 * S * M)), theta=f(rng.normal(0, 0.3, (M, 2, D + 1))))


def _far(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.fixture(scope="module")
def directions(oracle):
    """The CPU's directions of every shape at D = 10 and D = 3, made once and left unchanged."""
    return {(M, S, D): cpu_directions(oracle, 7, 5, 3, M, S, D) for M, S in SHAPES for D in (10, 3)}


def test_the_crafted_returns_reach_every_branch(directions):
    M, S, D = 5, 64, 10
    c = crafted_es(M, S, D, np.float64)
    delta = directions[(M, S, D)]
    rp, rm = c["returns"][:S * M].reshape(S, M), c["returns"][S * M:].reshape(S, M)
    full = restate_update(c["returns"], c["theta"], delta, S=S, dtype=np.float64)
    bad = (np.arange(S) % 7 == 3) | (np.arange(S) % 11 == 5) | (np.arange(S) % 13 == 6)
    assert 0 < bad.sum() < S and np.isnan(rp[3, 0]) and rm[5, 0] == np.inf and rp[6, 0] == -np.inf
    assert full["count"].tolist() == [S - bad.sum()] * 2 + [0] + [S - bad.sum()] * 2 and np.array_equal(full["used"], full["count"])
    assert np.array_equal(full["kept"].reshape(S, M)[:, 0], (~bad).astype(np.int32))
    # the population without a valid direction keeps theta, sigma_R = 0, grad = 0
    assert np.array_equal(full["theta_new"][NONE_VALID], c["theta"][NONE_VALID]) and full["sigma_r"][NONE_VALID] == 0
    assert (full["grad"][NONE_VALID] == 0).all() and (full["kept"].reshape(S, M)[:, NONE_VALID] == 0).all()
    # all kept returns equal: the floor binds, the direction sum is 0, theta stays
    assert full["sigma_r"][FLAT] == FLOOR and (full["grad"][FLAT] == 0).all() and np.array_equal(full["theta_new"][FLAT], c["theta"][FLAT])
    assert (full["sigma_r"][[0, 1, 4]] > 0.5).all() and (full["grad"][[0, 1, 4]] != 0).all()
    # top: ties straddle the cut, and the lower s goes first
    for top in tops(S):
        out = restate_update(c["returns"], c["theta"], delta, S=S, dtype=np.float64, top=top)
        want = np.minimum(top if 0 < top < S else S, full["count"])
        assert np.array_equal(out["used"], want) and np.array_equal(out["count"], full["count"]), top
        if top >= S:
            assert all(np.array_equal(out[k], full[k]) for k in full)
    half = restate_update(c["returns"], c["theta"], delta, S=S, dtype=np.float64, top=S // 2)
    k0 = half["kept"].reshape(S, M)[:, 0].astype(bool)
    score = np.where(~bad, np.maximum(rp[:, 0], rm[:, 0]), -np.inf)
    cut = score[k0].min()
    tied = np.flatnonzero((score == cut) & ~bad)
    assert k0.sum() == S // 2 and 0 < k0[tied].sum() < len(tied)                     # the cut goes through a tie ...
    assert k0[tied].tolist() == sorted(k0[tied].tolist(), reverse=True)             # ... and keeps its lower s
    assert (score[k0] >= cut).all() and (score[~k0 & ~bad] <= cut).all()
    one = restate_update(c["returns"], c["theta"], delta, S=S, dtype=np.float64, top=1)
    best = int(np.flatnonzero(one["kept"].reshape(S, M)[:, 0])[0])
    assert score[best] == score.max() and best == int(np.flatnonzero(score == score.max())[0])
    # the perturbation: both lanes move by the same rounded product, plus lanes first
    w = restate_perturb(c["theta"], delta, NU, S=S, dtype=np.float32)
    p = np.float32(NU) * delta.astype(np.float32)
    th = c["theta"].astype(np.float32)
    assert w.shape == (2 * S * M, 2, D + 1) and np.array_equal(w[7 * M + 1], th[1] + p[7 * M + 1]) and np.array_equal(w[S * M + 7 * M + 1], th[1] - p[7 * M + 1])
    # every shape and top of the GPU tests runs
    for (m, s) in SHAPES:
        cs = crafted_es(m, s, 3, np.float32)
        for top in tops(s):
            o = restate_update(cs["returns"], cs["theta"], directions[(m, s, 3)], S=s, dtype=np.float32, top=top)
            assert np.isfinite(o["theta_new"]).all() and o["kept"].sum() == o["used"].sum() and (o["used"] <= o["count"]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_against_a_plain_statement(directions, dtype):
    """float64: the restatement (64 partials, the tree, two passes) against np.argsort, np.std and one einsum; float32: the
    restatement in float32 against itself in float64 on the same rounded inputs.  kept, count and used are equal exactly."""
    worst = dict(theta_new=0.0, sigma_r=0.0, grad=0.0)
    for (M, S) in SHAPES:
        for D in (10, 3):
            c = crafted_es(M, S, D, dtype)
            delta = directions[(M, S, D)].astype(dtype)
            for top in tops(S):
                got = restate_update(c["returns"], c["theta"], delta, S=S, dtype=dtype, top=top)
                if dtype is np.float64:
                    want = plain_update(c["returns"], c["theta"], delta, S=S, top=top)
                else:
                    want = restate_update(c["returns"], c["theta"], delta, S=S, dtype=np.float64, top=top)
                for name in ("kept", "count", "used"):
                    assert np.array_equal(got[name], want[name]), (M, S, D, top, name)
                for name in worst:
                    if np.abs(want[name]).max() > 0:
                        worst[name] = max(worst[name], _far(got[name], want[name]))
    bound = {k: MARGIN * v for k, v in MEASURED[dtype].items()}
    print(f"[es restatement, {dtype.__name__}] worst relative distance {worst}, bound {bound}")
    for name in worst:
        assert worst[name] <= bound[name], (name, worst[name], bound[name])
    assert all(v < (1e-12 if dtype is np.float64 else 1e-4) for v in bound.values())


# ---------------------------------------------------------------------------------------
# header, table, exports, resources
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import _lib, control, es
    protos = _prototypes("os2r_es.h", "os2ra")
    assert [p[0] for p in protos] == list(es.ENTRY_POINTS) == NAMES
    lib = es.load()
    for name, ret, args in protos:
        argtypes = es.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2ra_last_error" else C.c_int)
    perturb, update = protos[2][2], protos[3][2]
    assert perturb[:7] == ["const Os2rControlLayout* layout", "int64_t npops", "int32_t ndirs", "uint32_t flags", "uint64_t seed",
                           "uint32_t pop_offset", "uint32_t generation"]
    assert len(perturb) == 12 and perturb[8] == "double nu" and perturb[-1] == "void* stream"
    assert update[:8] == ["const Os2rControlLayout* layout", "int64_t npops", "int32_t ndirs", "int32_t top", "uint32_t flags", "uint64_t seed",
                          "uint32_t pop_offset", "uint32_t generation"]
    assert len(update) == 20 and update[10] == "double step_size" and update[11] == "double sigma_floor" and update[-1] == "void* stream"
    header = _header("os2r_es.h")
    assert re.search(r"#define OS2R_ES_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert len(re.findall(r"#include", header)) == 1
    assert lib.os2ra_abi_version() == es.ABI_VERSION == 1
    assert es.STREAM == int(re.search(r"#define OS2RA_STREAM (\d+)", header).group(1)) == 6 == abi.STREAM_POLICY_NOISE + 1
    assert es.CHUNKS == int(re.search(r"#define OS2RA_CHUNKS (\d+)", header).group(1)) == CHUNKS
    assert es.MAX_DIRECTIONS == int(re.search(r"#define OS2RA_MAX_DIRECTIONS (\d+)", header).group(1)) == 2 ** 27 - 1
    assert es.Os2rControlLayout is control.Os2rControlLayout and es.layout is control.layout
    assert not set(es.ENTRY_POINTS) & (set(_lib.ENTRY_POINTS) | set(_lib.RECORD_ENTRY_POINTS)) and len(_lib.ENTRY_POINTS) == 35
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", es.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "libos2r_es.map")) as f:
        assert re.search(r"global:\s*os2ra_\*;\s*local:\s*\*;", f.read())
    # the header names no other companion library (their tests forbid it) and no other header declares anything of this one
    for word in FORBIDDEN:
        assert word not in header.lower(), word
    flat = " ".join(header.replace("\n *", " ").split())
    assert "adjacent-pair tree" in flat and "in ascending order onto 0" in flat and "NOT contracted" in flat
    for line in ("MLP policies and scheduled policies", "one-sided (non-antithetic) sampling", "covariance adaptation (CMA-ES)",
                 "a shared noise table", "the caller swaps two buffers"):
        assert line in flat, line
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "os2r_es.h":
            assert "os2ra_" not in _header(name).lower() and "os2r_es.h" not in _header(name).lower(), name
    # the stream constant is the new header's: the stepper's header is as it was, and is included, not copied
    src = _csrc("os2r_es.hpp")
    assert '#include "os2r_device.hpp"' in src and "normal2(" in src and "philox4x32_10" not in src
    assert "kStreamPolicyNoise = 5 }" in _csrc("os2r_device.hpp")


KERNELS = ("es_perturb_kernel", "es_score_kernel", "es_rank_kernel", "es_keep_kernel", "es_sum_kernel", "es_sum_wide_kernel", "es_sum_few_kernel")


def test_kernel_resources():
    """Exactly fourteen kernels, the seven of os2r_es.hpp in float and double, are in the built library and none uses scratch:
    private_segment_fixed_size 0, no VGPR or SGPR spill and no AGPRs in the code-object metadata.  Only the sixteen-wave sum
    uses LDS: the two returns, the two products and the flags of the 1 024 directions of a round.  The VGPR counts are printed (and recorded
    in DESIGN.md section 4); every kernel stays at four waves a SIMD or more, which is what the bound below keeps, and the
    sixteen waves of the wide sum fit a compute unit."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import es
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(es.LIB_PATH)
    meta = kernel_meta.kernel_meta(es.LIB_PATH)
    assert len(meta) == 14, sorted(meta)
    for kernel in KERNELS:
        for real, size in (("float", 4), ("double", 8)):
            (name,) = [k for k in meta if f"{kernel}<{real}>" in k]
            m = meta[name]
            print(f"{kernel}<{real}>: {m['vgpr_count']} VGPRs")
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
            assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 128, (name, m)
            assert m["group_segment_fixed_size"] == (1024 * (4 * size + 4) if kernel == "es_sum_wide_kernel" else 0), (name, m)


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def _layouts():
    from gym_os2r_amd import control

    def Lay(dtype=abi.F64, **kw):
        lay = control.layout(dtype, 3, 0, [0, 1, 3, -1])
        for k, v in kw.items():
            setattr(lay, k, v)
        return C.byref(lay)
    return Lay


def _refused(lib, fn, prefix, good, cases, buf):
    seen = set()
    for kw, msg in cases:
        a = dict(good, **kw)
        rc = fn(*[a[k] for k in good], None)
        err = lib.os2ra_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(prefix), (list(kw), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases})                        # each cause has a text of its own
    assert not any(buf)                                                   # a refused call wrote nothing
    return seen


def _source_checks(unit_function, seen):
    """The source: no HIP call and every refusal of an argument before check_device."""
    body = _function(_csrc("os2r_es_capi.hip"), "int " + unit_function)
    first_hip = body.index("check_device(")
    assert not re.search(HIP_CALL, body[:first_hip]) and body.index("DeviceGuard") > first_hip and body.index("auto launch") > first_hip
    fails = [m.start() for m in re.finditer(r"fail\(OS2R_ERR_INVALID", body)]
    assert fails and all(i < first_hip for i in fails)
    texts = re.findall(r'fail\(OS2R_ERR_INVALID, "([^"]+)"', body) + [t for pair in re.findall(r'\? "([^"]+)" : "([^"]+)"', body) for t in pair]
    texts += re.findall(r'return "([^"]+)";', _function(_csrc("os2r_es_capi.hip"), r"const char\* shape_refusal"))
    assert len(texts) == len(set(texts)) and all(any(t.encode() in e for e in seen) for t in texts), [t for t in texts if not any(t.encode() in e for e in seen)]


def test_perturb_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import es
    lib = es.load()
    Lay = _layouts()
    M, S, D = 2, 3, 4
    E, SM = 2 * (D + 1), S * M
    buf = (C.c_double * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    at = lambda i: C.c_void_p(base + 8 * i)
    nan, inf = float("nan"), float("inf")
    where = dict(theta=0, weights=64, delta=64 + 2 * SM * E)
    size = dict(theta=M * E, weights=2 * SM * E, delta=SM * E)
    assert where["delta"] + size["delta"] < 4000
    good = dict(lay=Lay(), M=M, S=S, flags=0, seed=7, off=0, gen=1, theta=at(where["theta"]), nu=NU, weights=at(where["weights"]),
                delta=at(where["delta"]))
    name = "os2ra_es_perturb"
    assert len(good) + 1 == len(es.ENTRY_POINTS[name])
    assert lib.os2ra_es_perturb(*[None if _is_pointer(t) else 0 for t in es.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2ra_last_error() == b"os2ra_es_perturb: null layout"
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(nq=1)), b"nq must be 2..5"),
             (dict(lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"), (dict(lay=Lay(obs_dim=13)), b"obs_dim must be 1..12"),
             (dict(M=0), b"npops must be >= 1"), (dict(M=-3), b"npops must be >= 1"), (dict(S=0), b"ndirs must be >= 1"),
             (dict(S=-1), b"ndirs must be >= 1"), (dict(S=2 ** 27, M=1), b"ndirs must be < 2^27"), (dict(S=2 ** 31 - 1, M=1), b"ndirs must be < 2^27"),
             (dict(S=2 ** 27 - 1, M=9), b"2 * ndirs * npops exceeds 2^31 - 1"), (dict(S=1, M=2 ** 30), b"2 * ndirs * npops exceeds 2^31 - 1"),
             (dict(M=2 ** 62), b"2 * ndirs * npops exceeds 2^31 - 1"),
             (dict(flags=1), b"unknown flag bits"), (dict(flags=0x80000000), b"unknown flag bits"),
             (dict(nu=nan), b"nu must be finite"), (dict(nu=inf), b"nu must be finite"), (dict(nu=-inf), b"nu must be finite"),
             (dict(nu=-0.03), b"nu must be >= 0"), (dict(nu=-5e-324), b"nu must be >= 0"),
             (dict(theta=None), b"null theta_dev"), (dict(weights=None), b"null weights_dev"),
             (dict(theta=at(1)), b"theta_dev must be aligned to a pair"), (dict(weights=at(65)), b"weights_dev must be aligned to a pair"),
             (dict(delta=at(where["delta"] + 1)), b"delta_dev must be aligned to a pair"),
             (dict(lay=Lay(abi.F32), theta=C.c_void_p(base + 4)), b"theta_dev must be aligned to a pair"),
             (dict(weights=at(size["theta"] - 2)), b"weights_dev overlaps theta_dev"), (dict(theta=at(where["weights"] + size["weights"] - 2)), b"weights_dev overlaps theta_dev"),
             (dict(delta=at(0)), b"delta_dev overlaps theta_dev"), (dict(delta=at(where["weights"] + 2)), b"delta_dev overlaps weights_dev"),
             (dict(delta=at(where["weights"] + size["weights"] - 2)), b"delta_dev overlaps weights_dev")]
    seen = _refused(lib, lib.os2ra_es_perturb, b"os2ra_es_perturb: ", good, cases, buf)
    assert len(seen) == 19
    # the edges are taken: nothing is left to refuse but the device, and no call is let through to one
    edges = [dict(S=2 ** 27 - 1, M=8, weights=at(10 ** 6), delta=None), dict(nu=0.0), dict(nu=-0.0), dict(nu=5e-324), dict(delta=None),
             dict(seed=2 ** 64 - 1, off=2 ** 32 - 1, gen=2 ** 32 - 1), dict(delta=at(where["weights"] + size["weights"])),
             dict(weights=at(size["theta"]), delta=None)]
    for kw in edges:                                  # (device 1000 is never there, with a GPU or without)
        a = dict(good, **dict(kw, lay=Lay(device=1000)))
        assert lib.os2ra_es_perturb(*[a[k] for k in good], None) == abi.ERR_NO_DEVICE and lib.os2ra_last_error().startswith(b"os2ra_es_perturb: "), kw
    assert not any(buf)
    _source_checks(name, seen)


def test_update_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import es
    lib = es.load()
    Lay = _layouts()
    M, S, D = 2, 4, 4
    E, SM = 2 * (D + 1), S * M
    buf = (C.c_double * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    at = lambda i: C.c_void_p(base + 8 * i)
    nan, inf = float("nan"), float("inf")
    size = dict(returns=2 * SM, theta=M * E, theta_out=M * E, sigma_r=M, count=M, used=M, grad=M * E, kept=SM, score=SM)
    where, nxt = {}, 0
    for name, n in size.items():
        if name == "theta_out":
            nxt = 2048
        where[name] = nxt
        nxt += (n + 1) & ~1                               # every array starts at a pair
    assert nxt < 4000
    good = dict(lay=Lay(), M=M, S=S, top=2, flags=0, seed=7, off=0, gen=1, returns=at(where["returns"]), theta=at(where["theta"]), step=STEP,
                floor=FLOOR, theta_out=at(where["theta_out"]), sigma_r=at(where["sigma_r"]), count=at(where["count"]), used=at(where["used"]),
                grad=at(where["grad"]), kept=at(where["kept"]), score=at(where["score"]))
    name = "os2ra_es_update"
    assert len(good) + 1 == len(es.ENTRY_POINTS[name])
    assert lib.os2ra_es_update(*[None if _is_pointer(t) else 0 for t in es.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2ra_last_error() == b"os2ra_es_update: null layout"
    end = lambda n: where[n] + size[n] - 1
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(nq=6)), b"nq must be 2..5"),
             (dict(lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"), (dict(lay=Lay(obs_dim=13)), b"obs_dim must be 1..12"),
             (dict(M=0), b"npops must be >= 1"), (dict(S=0), b"ndirs must be >= 1"), (dict(S=-7), b"ndirs must be >= 1"),
             (dict(S=2 ** 27, M=1), b"ndirs must be < 2^27"), (dict(S=2 ** 27 - 1, M=9), b"2 * ndirs * npops exceeds 2^31 - 1"),
             (dict(S=2 ** 29, M=1), b"ndirs must be < 2^27"), (dict(M=2 ** 40), b"2 * ndirs * npops exceeds 2^31 - 1"),
             (dict(top=-1), b"top must be >= 0"), (dict(top=-2 ** 31), b"top must be >= 0"),
             (dict(flags=2), b"unknown flag bits"), (dict(flags=0xffffffff), b"unknown flag bits"),
             (dict(step=nan), b"step_size must be finite"), (dict(step=inf), b"step_size must be finite"), (dict(step=-0.02), b"step_size must be >= 0"),
             (dict(floor=nan), b"sigma_floor must be finite"), (dict(floor=-inf), b"sigma_floor must be finite"),
             (dict(floor=-1e-8), b"sigma_floor must be >= 0"), (dict(floor=-5e-324), b"sigma_floor must be >= 0"),
             (dict(returns=None), b"null returns_dev"), (dict(theta=None), b"null theta_dev"), (dict(theta_out=None), b"null theta_out_dev"),
             (dict(sigma_r=None), b"null sigma_r_dev"), (dict(count=None), b"null count_dev"), (dict(used=None), b"null used_dev"),
             (dict(kept=None), b"null kept_dev"), (dict(score=None), b"null score_dev with 0 < top < ndirs"),
             (dict(score=None, top=S - 1), b"null score_dev with 0 < top < ndirs"),
             (dict(theta=at(where["theta"] + 1)), b"theta_dev must be aligned to a pair"),
             (dict(theta_out=at(where["theta_out"] + 1)), b"theta_out_dev must be aligned to a pair"),
             (dict(grad=at(where["grad"] + 1)), b"grad_dev must be aligned to a pair"),
             (dict(score=C.c_void_p(base + 8 * where["score"] + 4)), b"score_dev must be aligned to its elements"),
             # an output over an input, from both sides; over another output; the optional ones too
             (dict(theta_out=at(where["theta"])), b"theta_out_dev overlaps theta_dev"),
             (dict(theta_out=at(end("returns") - 1)), b"theta_out_dev overlaps returns_dev"),
             (dict(sigma_r=at(end("returns"))), b"sigma_r_dev overlaps returns_dev"), (dict(count=at(where["theta"])), b"count_dev overlaps theta_dev"),
             (dict(used=at(end("theta"))), b"used_dev overlaps theta_dev"), (dict(grad=at(where["returns"])), b"grad_dev overlaps returns_dev"),
             (dict(kept=at(where["theta"])), b"kept_dev overlaps theta_dev"), (dict(score=at(where["returns"])), b"score_dev overlaps returns_dev"),
             (dict(sigma_r=at(end("theta_out"))), b"sigma_r_dev overlaps theta_out_dev"), (dict(count=at(where["sigma_r"])), b"count_dev overlaps sigma_r_dev"),
             (dict(used=at(where["count"])), b"used_dev overlaps count_dev"), (dict(grad=at(where["used"])), b"grad_dev overlaps used_dev"),
             (dict(kept=at(end("grad"))), b"kept_dev overlaps grad_dev"), (dict(score=at(where["kept"])), b"score_dev overlaps kept_dev")]
    seen = _refused(lib, lib.os2ra_es_update, b"os2ra_es_update: ", good, cases, buf)
    assert len(seen) == 40
    edges = [dict(top=0, score=None), dict(top=S, score=None), dict(top=2 ** 31 - 1, score=None), dict(top=S, score=at(where["returns"])),
             dict(step=0.0, floor=0.0), dict(step=-0.0, floor=5e-324), dict(grad=None), dict(top=0, score=C.c_void_p(base + 4)),
             dict(S=2 ** 27 - 1, top=0, returns=C.c_void_p(2 ** 44), kept=C.c_void_p(2 ** 45), score=None),
             dict(seed=2 ** 64 - 1, off=2 ** 32 - 1, gen=2 ** 32 - 1), dict(sigma_r=at(where["theta_out"] + size["theta_out"]))]
    for kw in edges:
        a = dict(good, **dict(kw, lay=Lay(device=1000)))
        assert lib.os2ra_es_update(*[a[k] for k in good], None) == abi.ERR_NO_DEVICE and lib.os2ra_last_error().startswith(b"os2ra_es_update: "), kw
    assert not any(buf)
    _source_checks(name, seen)


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


def test_python_argument_errors_need_no_device(monkeypatch):
    import torch
    from gym_os2r_amd import es
    from gym_os2r_amd.sim import HipSim
    for method in ("es_perturb", "es_perturb_into", "es_update", "es_update_into"):
        assert callable(getattr(HipSim, method))
    assert "Mania et al. 2018" in HipSim.es_update.__doc__ and "regenerated" in HipSim.es_update.__doc__

    def no_load():
        raise AssertionError("a refused call reached es.load")
    monkeypatch.setattr(es, "load", no_load)
    f64, i32 = torch.float64, torch.int32
    s = _bare(f64)
    M, S, D = 2, 4, 4
    SM, N = S * M, 2 * S * M
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    theta, weights, delta = z(M, 2, D + 1), z(N, 2, D + 1), z(SM, 2, D + 1)
    ok = dict(directions=S, nu=NU, generation=1, seed=3)

    def perturb_into(*args, **kw):
        with pytest.raises(ValueError, match="^es_perturb: "):
            s.es_perturb_into(*args, **dict(ok, **kw))

    def perturb(*args, **kw):
        with pytest.raises(ValueError, match="^es_perturb: "):
            s.es_perturb(*args, **dict(ok, **kw))
    words = (dict(directions=0), dict(directions=-1), dict(directions=2.0), dict(directions=True), dict(directions=None), dict(directions=2 ** 27),
             dict(generation=-1), dict(generation=2 ** 32), dict(generation=1.0), dict(generation=True),
             dict(pop_offset=-1), dict(pop_offset=2 ** 32), dict(pop_offset="0"), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(seed=True))
    for kw in words:
        perturb_into(theta, weights, **kw)
        perturb(theta, **kw)
    for bad in (float("nan"), float("inf"), -0.1, "x", None, True):
        perturb_into(theta, weights, nu=bad)
        perturb(theta, nu=bad)
    for bad in (None, theta.numpy(), z(M, 2), z(0, 2, D + 1), z(M, 3, D + 1), z(M, 2, D), theta.float(), z(2, D + 1, M).permute(2, 0, 1)):
        perturb_into(bad, weights)
        perturb(bad)
    for bad in (None, z(N + 1, 2, D + 1), z(N, 2, D), weights.float(), z(2, N, D + 1).permute(1, 0, 2), weights.numpy()):
        perturb_into(theta, bad)
    for bad in (z(SM + 1, 2, D + 1), delta.float(), z(SM, D + 1, 2)):
        perturb_into(theta, weights, delta=bad)
    perturb_into(theta.to("meta"), weights)                                       # another device than the handle's
    perturb_into(theta, weights.to("meta"))
    perturb_into(theta, weights, delta=delta.to("meta"))
    pool = z(4096)
    E = 2 * (D + 1)
    perturb_into(pool[1:1 + M * E].reshape(M, 2, D + 1), weights)                   # not aligned to a pair
    perturb_into(theta, pool[1:1 + N * E].reshape(N, 2, D + 1))
    perturb_into(theta, weights, delta=pool[3:3 + SM * E].reshape(SM, 2, D + 1))
    perturb_into(pool[:M * E].reshape(M, 2, D + 1), pool[M * E - 2:M * E - 2 + N * E].reshape(N, 2, D + 1))       # overlap
    perturb_into(theta, pool[:N * E].reshape(N, 2, D + 1), delta=pool[N * E - 2:N * E - 2 + SM * E].reshape(SM, 2, D + 1))

    returns, theta_new, sigma_r = z(N), z(M, 2, D + 1), z(M)
    count, used, kept, score = z(M, dtype=i32), z(M, dtype=i32), z(SM, dtype=i32), z(SM)
    full = (returns, theta, theta_new, sigma_r, count, used, kept)
    uok = dict(directions=S, generation=1, step_size=STEP, seed=3)

    def update_into(*args, **kw):
        with pytest.raises(ValueError, match="^es_update: "):
            s.es_update_into(*args, **dict(uok, **kw))

    def update(*args, **kw):
        with pytest.raises(ValueError, match="^es_update: "):
            s.es_update(*args, **dict(uok, **kw))
    for kw in words:
        update_into(*full, **kw)
        update(returns, theta, **kw)
    for bad in (float("nan"), float("inf"), -0.1, "x", None, True):
        update_into(*full, step_size=bad)
        update_into(*full, sigma_floor=bad)
        update(returns, theta, step_size=bad)
        update(returns, theta, sigma_floor=bad)
    for bad in (-1, 1.0, True, None, "2"):
        update_into(*full, top=bad)
        update(returns, theta, top=bad)
    update_into(*full, top=2)                                                    # a top that selects needs score
    update_into(*full, top=S - 1, score=z(SM + 1))
    update_into(*full, top=1, score=score.float())
    for i in range(len(full)):
        update_into(*[None if j == i else t for j, t in enumerate(full)])
    swap = lambda i, t: tuple(t if j == i else a for j, a in enumerate(full))
    for args in (swap(0, z(N + 1)), swap(0, z(2, SM)), swap(0, returns.float()), swap(0, returns.numpy()), swap(1, z(M, 2, D)), swap(2, z(M + 1, 2, D + 1)),
                 swap(2, theta_new.float()), swap(2, theta), swap(3, z(M + 1)), swap(3, z(M, dtype=i32)), swap(4, z(M)), swap(4, z(M + 1, dtype=i32)),
                 swap(5, z(M, dtype=torch.int64)), swap(5, count), swap(6, z(SM)), swap(6, z(S, M, dtype=i32)), swap(6, z(SM + 1, dtype=i32)),
                 swap(2, pool[1:1 + M * E].reshape(M, 2, D + 1)), swap(3, returns[:M])):
        update_into(*args)
    for args in (swap(0, returns.to("meta")), swap(1, theta.to("meta")), swap(2, theta_new.to("meta")), swap(6, kept.to("meta"))):
        update_into(*args)                                                       # another device than the handle's
    for kw in (dict(grad=z(M, 2, D)), dict(grad=theta_new), dict(grad=z(M, 2, D + 1).float()), dict(grad=pool[1:1 + M * E].reshape(M, 2, D + 1)),
               dict(top=2, score=returns[:SM])):
        update_into(*full, **kw)
    for args in ((None, theta), (z(N + 2), theta), (returns.float(), theta), (returns, None), (returns, z(M, 2, D))):
        update(*args)
    # what passes every check reaches the loader, and only then (the bare handle has no cfg to fill a layout from)
    with pytest.raises(AttributeError):
        s.es_perturb_into(theta, weights, delta=delta, **ok)
    with pytest.raises(AttributeError):
        s.es_update_into(*full, top=2, score=score, grad=z(M, 2, D + 1), **uok)
    with pytest.raises(AttributeError):
        s.es_update_into(*full, top=S, **uok)                                    # top >= S selects nothing: no score needed
