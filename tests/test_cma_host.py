"""libos2r_cma.so (include/os2r_cma.h): the host side -- the numpy restatement of the factor and the samples and of the CMA-ES
update the GPU tests compare with (`restate_sample`, `restate_update`), the normals on the CPU (`cpu_normals`: Box-Muller on the
oracle's uniform2 with the documented counter words), the crafted populations of the GPU tests (`crafted_cma`) and the branches
they reach, the restatement against an independent plain statement (np.linalg.cholesky, a stable np.argsort, einsum) in float64
and in float32 against its own float64 result, cma.constants against Hansen's formulas, the restatement as an optimiser of a
22-dimensional ellipsoid, the header against the one table of gym_os2r_amd/cma.py, the exports of the library, the resources of
the eight kernels in the built library, every refusal of both entry points through ctypes without a device, and the argument
checks of HipSim.cma_sample / cma_update that need no device.  No GPU needed."""
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
from header_check import HIP_CALL, _agrees, _csrc, _function, _header, _is_pointer, _prototypes  # noqa: E402

NAMES = ["os2rk_abi_version", "os2rk_last_error", "os2rk_cma_sample", "os2rk_cma_update"]
CHUNKS = 64
AGE = 3                                  # of the crafted updates: it enters hsig_bound only
SIGMA_MIN, SIGMA_MAX = 1e-8, 1.0
# The crafted populations, by role(m) = m where M <= 8, else m % 8 (a shape with fewer populations has the first roles only):
PLAIN, FEW_VALID, FAILS_AT_0, FAILS_LATER, SIGMA_ZERO, STALLED, CLAMPED_HIGH, CLAMPED_LOW = range(8)
LATER = 3                                # the column at which the factor of FAILS_LATER fails
# (M, S) of the GPU tests (tests/test_gpu_cma.py): the fewest samples; fewer than 64 with empty partials; exactly 64 with the first
# five roles; one full round and one lane more; partials of up to three terms; every role, a tree cut to two levels and two
# workgroups of populations in the rank and sample launches; eighteen rounds of the sum, the last not full
SHAPES = [(1, 2), (1, 5), (5, 64), (3, 65), (2, 130), (257, 4), (2, 1100)]
# The largest relative distance (the largest difference over the largest entry of the reference) measured on the CPU this test
# was written on, over SHAPES x D in (10, 3), of the populations with status 0; the tests print them.  float64: of the
# restatement from the plain statement (np.linalg.cholesky, np.argsort, np.einsum); float32: of the float32 restatement from the
# float64 one, on the ranks and the normals of the float32 one.  The bound is MARGIN x that.
MEASURED = {np.float64: dict(factor=2.924e-14, weights=4.458e-15, mean=5.141e-15, sigma=5.552e-17, cov=1.265e-15, p_sigma=1.780e-15, p_c=1.258e-14,
                             yw=1.404e-14, ps_norm=6.486e-16, growth=4.203e-16),
            np.float32: dict(factor=1.606e-5, weights=2.452e-6, mean=2.819e-6, sigma=1.370e-7, cov=1.508e-7, p_sigma=1.651e-7, p_c=6.903e-6,
                             yw=7.696e-6, ps_norm=1.482e-7, growth=2.799e-7)}
MARGIN = 8
FORBIDDEN = ("os2ra_", "os2r_es.h", "os2rz_", "os2r_norm.h", "os2rb_", "os2r_box", "os2rg_", "os2r_pg", "os2rv_", "os2r_critic", "os2ro_",
             "os2r_ppo", "os2rn_", "os2r_npg", "os2rx_", "os2r_cem", "os2ru_", "os2r_ukf", "os2re_", "os2r_ekf", "os2rp_", "os2r_pf", "os2rm_",
             "mppi", "os2rt_", "steer", "line_search")
STATE = ("mean", "sigma", "cov", "p_sigma", "p_c")


# ---------------------------------------------------------------------------------------
# the normals, and the restatement of include/os2r_cma.h (need no device)
# ---------------------------------------------------------------------------------------
def cpu_normals(oracle, seed, pop_offset, generation, M, S, D):
    """z [S M, 2, D+1] in float64, row s M + m: entry e = j (D + 1) + i of z[m][s] is output e & 1 of Box-Muller on the oracle's
    uniform2(seed, (pop_offset + m) mod 2^32, 7, generation, 16 s + (e >> 1))."""
    from gym_os2r_amd import cma
    n = D + 1
    u = np.array([oracle.uniform2(seed, (pop_offset + m) & 0xFFFFFFFF, cma.STREAM, generation, 16 * s + q)
                  for s in range(S) for m in range(M) for q in range(n)])
    r = np.sqrt(-2.0 * np.log(1.0 - u[:, 0]))
    th = 6.283185307179586476925286766559 * u[:, 1]
    return np.stack([r * np.cos(th), r * np.sin(th)], axis=1).reshape(S * M, 2, n)


def _positive(x):
    return np.isfinite(x) & (x > 0)


def _chains(A, z):
    """y[..., e] = the chain A[e][0] z[0], + A[e][j] z[j] for j = 1 .. e.  A [M, E, E], z [S, M, E] -> [S, M, E]."""
    E = A.shape[-1]
    y = A[None, :, :, 0] * z[:, :, 0:1]
    for j in range(1, E):
        y[:, :, j:] = y[:, :, j:] + A[None, :, j:, j] * z[:, :, j:j + 1]
    return y


def restate_sample(state, z, *, S, dtype):
    """include/os2r_cma.h, os2rk_cma_sample, in numpy and in `dtype` on given normals z [S M, 2, D+1] (the device's, or the
    CPU's).  state: dict(mean [M, 2, D+1], sigma [M], cov [M, E, E], ...).
    -> dict(factor [M, E, E], failed [M] int32, weights [S M, 2, D+1], y [S, M, E])."""
    mean, sigma, C_ = (np.asarray(state[k]).astype(dtype) for k in ("mean", "sigma", "cov"))
    M, E = mean.shape[0], mean.shape[1] * mean.shape[2]
    z = np.asarray(z).astype(dtype).reshape(S, M, E)
    A = np.zeros((M, E, E), dtype)
    failed = np.zeros(M, np.int32)
    with np.errstate(all="ignore"):
        for j in range(E):                                                        # step 1: by columns, rows i >= j at once
            acc = C_[:, j:, j].copy()
            for k in range(j):
                acc = acc - A[:, j:, k] * A[:, j:j + 1, k]
            bad = ~_positive(acc[:, 0])
            failed[bad & (failed == 0)] = j + 1
            root = np.sqrt(acc[:, 0])
            A[:, j, j] = root
            A[:, j + 1:, j] = acc[:, 1:] / root[:, None]
        failed[(failed == 0) & ~_positive(sigma)] = E + 1
        A[failed != 0] = 0
        y = _chains(A, z)                                                         # step 2
        w = mean.reshape(1, M, E) + sigma[None, :, None] * y                      # step 3
        w = np.where((failed != 0)[None, :, None], mean.reshape(1, M, E), w)
    assert all(a.dtype == dtype for a in (A, y, w))
    return dict(factor=A, failed=failed, weights=w.reshape(S * M, *mean.shape[1:]), y=y)


def restate_ranks(returns, S, M):
    """Steps 1 and 2: -> (valid [S, M] bool, count [M] int32, rank [S, M] int32)."""
    r = np.asarray(returns).reshape(S, M)
    valid = np.isfinite(r)
    count = valid.sum(0).astype(np.int32)
    s_idx = np.arange(S)
    with np.errstate(all="ignore"):
        ahead = valid[:, None, :] & ((r[:, None, :] > r[None, :, :]) | ((r[:, None, :] == r[None, :, :]) & (s_idx[:, None, None] < s_idx[None, :, None])))
    rank_valid = ahead.sum(0)                                                     # [s', s, m] summed over s'
    below = np.cumsum(~valid, axis=0) - (~valid)
    rank = np.where(valid, rank_valid, count[None] + below).astype(np.int32)
    return valid, count, rank


def chunked(terms, parent):
    """Step 3: the sum over the parents (parent [S, M] bool) of terms [S, M, ...] in 64 partials and the adjacent-pair tree;
    partial c walks s = c, c + 64, ... in ascending order."""
    S = parent.shape[0]
    rounds = -(-S // CHUNKS)
    pad = rounds * CHUNKS - S
    t = np.concatenate([terms, np.zeros((pad,) + terms.shape[1:], terms.dtype)]).reshape((rounds, CHUNKS) + terms.shape[1:])
    p = np.concatenate([parent, np.zeros((pad,) + parent.shape[1:], bool)]).reshape((rounds, CHUNKS) + parent.shape[1:])
    p = p.reshape(p.shape + (1,) * (t.ndim - p.ndim))
    acc = np.zeros(t.shape[1:], terms.dtype)
    for r in range(rounds):
        acc = np.where(p[r], acc + t[r], acc)
    parts = acc
    while parts.shape[0] > 1:
        parts = parts[0::2] + parts[1::2]
    return parts[0]


def restate_update(returns, rankw, state, factor, failed, z, consts, *, S, dtype, growth=None):
    """include/os2r_cma.h, os2rk_cma_update, steps 1-8, in numpy and in `dtype`, on given normals z [S M, 2, D+1] and, where
    given, on the device's growth [M] (its exp is within 8 ulp, everything else is exact).  consts: the Os2rkCmaConstants.
    -> dict(mean, sigma, cov, p_sigma, p_c, count, status, rank [S M], yw [M, 2, D+1], ps_norm, growth)."""
    f = lambda a: np.asarray(a).astype(dtype)
    returns, rankw, factor = f(returns), f(rankw), f(factor)
    mean, sigma, cov, ps, pc = (f(state[k]) for k in STATE)
    M, E, mu = mean.shape[0], mean.shape[1] * mean.shape[2], len(rankw)
    k = {name: np.float64(getattr(consts, name)).astype(dtype) for name, _ in consts._fields_}
    z = f(z).reshape(S, M, E)
    valid, count, rank = restate_ranks(returns, S, M)                              # steps 1, 2
    status = np.where(np.asarray(failed) != 0, 2, np.where(count < mu, 1, 0)).astype(np.int32)
    parent = rank < mu
    w = np.where(parent, rankw[np.minimum(rank, mu - 1)], dtype(0))
    with np.errstate(all="ignore"):
        y = _chains(factor, z)                                                     # step 3
        t = w[:, :, None] * y
        zw = chunked(w[:, :, None] * z, parent)
        yw = chunked(t, parent)
        R = chunked(t[:, :, :, None] * y[:, :, None, :], parent)
        mean_new = mean.reshape(M, E) + sigma[:, None] * yw                       # step 4
        ps_new = k["a_sigma"] * ps + k["b_sigma"] * zw                            # step 5
        sq = np.zeros(M, dtype)
        for e in range(E):
            sq = sq + ps_new[:, e] * ps_new[:, e]
        nrm = np.sqrt(sq)
        h = nrm < k["hsig_bound"]
        keep = k["a_c"] * pc                                                      # step 6
        pc_new = np.where(h[:, None], keep + k["b_c"] * yw, keep)
        k0 = np.where(h, k["k0_moving"], k["k0_stalled"])                         # step 7
        low = (k0[:, None, None] * cov + k["c_1"] * (pc_new[:, :, None] * pc_new[:, None, :])) + k["c_mu"] * R
        low = np.tril(low)
        cov_new = low + np.swapaxes(np.tril(low, -1), 1, 2)
        g = np.exp(k["g_sigma"] * (nrm / k["chi"] - dtype(1))) if growth is None else f(growth)     # step 8
        sigma_new = np.minimum(np.maximum(sigma * g, k["sigma_min"]), k["sigma_max"])
    stay = status != 0
    out = dict(mean=np.where(stay[:, None], mean.reshape(M, E), mean_new).reshape(mean.shape), sigma=np.where(stay, sigma, sigma_new),
               cov=np.where(stay[:, None, None], cov, cov_new), p_sigma=np.where(stay[:, None], ps, ps_new),
               p_c=np.where(stay[:, None], pc, pc_new), yw=np.where(stay[:, None], dtype(0), yw).reshape(mean.shape),
               ps_norm=np.where(stay, dtype(0), nrm), growth=np.where(stay, dtype(1), g))
    assert all(a.dtype == dtype for a in out.values()), {n: a.dtype for n, a in out.items()}
    out.update(count=count, status=status, rank=rank.reshape(S * M), h=h)
    return out


def plain_generation(returns, rankw, state, z, consts, *, S):
    """The independent statement in float64, a population at a time: np.linalg.cholesky, a stable np.argsort of the negated valid
    returns, einsum.  -> the outputs of both calls in one dict (factor, failed != 0, weights, and those of the update)."""
    f = lambda a: np.asarray(a, np.float64)
    returns, rankw = f(returns), f(rankw)
    mean, sigma, cov, ps, pc = (f(state[k]) for k in STATE)
    M, E, mu = mean.shape[0], mean.shape[1] * mean.shape[2], len(rankw)
    z, r = f(z).reshape(S, M, E), returns.reshape(S, M)
    k = {name: getattr(consts, name) for name, _ in consts._fields_}
    out = dict(factor=np.zeros((M, E, E)), failed=np.zeros(M, bool), weights=np.zeros((S, M, E)), mean=mean.copy(), sigma=sigma.copy(), cov=cov.copy(),
               p_sigma=ps.copy(), p_c=pc.copy(), count=np.zeros(M, np.int32), status=np.zeros(M, np.int32), rank=np.zeros((S, M), np.int32),
               yw=np.zeros((M, E)), ps_norm=np.zeros(M), growth=np.ones(M))
    for m in range(M):
        sym = np.tril(cov[m]) + np.tril(cov[m], -1).T
        try:
            A = np.linalg.cholesky(sym)
            ok = bool(np.isfinite(A).all() and np.isfinite(sigma[m]) and sigma[m] > 0)
        except np.linalg.LinAlgError:
            ok = False
        idx = np.flatnonzero(np.isfinite(r[:, m]))
        order = np.concatenate([idx[np.argsort(-r[idx, m], kind="stable")], np.flatnonzero(~np.isfinite(r[:, m]))])
        out["rank"][order, m] = np.arange(S)
        out["count"][m] = len(idx)
        out["failed"][m] = not ok
        out["status"][m] = 2 if not ok else (1 if len(idx) < mu else 0)
        out["weights"][:, m] = mean[m].reshape(E)
        if not ok:
            continue
        out["factor"][m] = A
        y = z[:, m] @ A.T
        out["weights"][:, m] = mean[m].reshape(E) + sigma[m] * y
        if out["status"][m]:
            continue
        par = order[:mu]
        yw, zw = np.einsum("r,re->e", rankw, y[par]), np.einsum("r,re->e", rankw, z[par, m])
        out["yw"][m] = yw
        out["mean"][m] = mean[m] + sigma[m] * yw.reshape(mean[m].shape)
        p = k["a_sigma"] * ps[m] + k["b_sigma"] * zw
        nrm = float(np.linalg.norm(p))
        h = nrm < k["hsig_bound"]
        q = k["a_c"] * pc[m] + (k["b_c"] * yw if h else 0.0)
        out["p_sigma"][m], out["p_c"][m], out["ps_norm"][m] = p, q, nrm
        out["cov"][m] = (k["k0_moving"] if h else k["k0_stalled"]) * sym + k["c_1"] * np.outer(q, q) + k["c_mu"] * np.einsum("r,ri,rj->ij", rankw, y[par], y[par])
        out["growth"][m] = math.exp(k["g_sigma"] * (nrm / k["chi"] - 1.0))
        out["sigma"][m] = min(max(sigma[m] * out["growth"][m], k["sigma_min"]), k["sigma_max"])
    out["weights"] = out["weights"].reshape(S * M, *mean.shape[1:])
    out["yw"] = out["yw"].reshape(mean.shape)
    out["rank"] = out["rank"].reshape(S * M)
    return out


def role(m, M):
    return m if M <= 8 else m % 8


def crafted_consts(D, S, age=AGE):
    from gym_os2r_amd import cma
    return cma.constants(2 * (D + 1), S, None, age, SIGMA_MIN, SIGMA_MAX)


def crafted_cma(M, S, D, dtype, seed=0):
    """The inputs of the GPU tests, in `dtype`.  The returns are small integers and halves (-3 .. 3 in steps of 1/2: most tie, and
    the zeros of odd s are -0).  By sample s: s % 7 == 3 is a NaN, s % 11 == 5 is +inf, s % 13 == 6 is -inf.  By role(m, M):
      PLAIN          a random positive definite covariance, paths of 0.3, sigma 0.3
      FEW_VALID      every return but that of s = 0 is a NaN: count = 1 < mu wherever S >= 4
      FAILS_AT_0     cov[0][0] = -1
      FAILS_LATER    cov[LATER][LATER] is what the columns before it take away, less 1/4
      SIGMA_ZERO     sigma = 0
      STALLED        p_sigma = 3 in every entry: h does not hold
      CLAMPED_HIGH   p_sigma = 10 in every entry and sigma = 0.999: sigma_max binds
      CLAMPED_LOW    p_sigma = 0 and sigma = 1.00001 sigma_min: where the new path is shorter than chi, in most of them, sigma_min binds
    The upper triangle of every covariance is a NaN: it is not read.
    -> dict(returns [S M], mean [M, 2, D+1], sigma [M], cov [M, E, E], p_sigma, p_c [M, E], rankw [mu], consts)"""
    rng = np.random.default_rng(seed + 1000 * M + S)
    n, E = D + 1, 2 * (D + 1)
    r = rng.integers(-6, 7, (S, M)).astype(np.float64) / 2.0
    s = np.arange(S)
    r[(r == 0) & (s[:, None] % 2 == 1)] = -0.0
    r[s % 7 == 3] = np.nan
    r[s % 11 == 5] = np.inf
    r[s % 13 == 6] = -np.inf
    B = np.eye(E)[None] + 0.15 * rng.normal(0, 1, (M, E, E))
    cov = B @ np.swapaxes(B, 1, 2)
    sigma = np.full(M, 0.3)
    ps, pc = rng.normal(0, 0.3, (M, E)), rng.normal(0, 0.3, (M, E))
    for m in range(M):
        what = role(m, M)
        if what == FEW_VALID:
            r[1:, m] = np.nan
            r[0, m] = 1.5
        elif what == FAILS_AT_0:
            cov[m, 0, 0] = -1.0
        elif what == FAILS_LATER:
            A = np.linalg.cholesky(cov[m])
            cov[m, LATER, LATER] = float(A[LATER, :LATER] @ A[LATER, :LATER]) - 0.25
        elif what == SIGMA_ZERO:
            sigma[m] = 0.0
        elif what == STALLED:
            ps[m] = 3.0
        elif what == CLAMPED_HIGH:
            ps[m], sigma[m] = 10.0, 0.999
        elif what == CLAMPED_LOW:
            ps[m], sigma[m] = 0.0, 1.00001 * SIGMA_MIN
    cov[:, np.triu_indices(E, 1)[0], np.triu_indices(E, 1)[1]] = np.nan
    rankw, consts = crafted_consts(D, S)
    f = lambda a: np.ascontiguousarray(np.asarray(a).astype(dtype))
    return dict(returns=f(r.reshape(S * M)), mean=f(rng.normal(0, 0.3, (M, 2, n))), sigma=f(sigma), cov=f(cov), p_sigma=f(ps), p_c=f(pc),
                rankw=f(rankw), consts=consts)


def _far(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.fixture(scope="module")
def normals(oracle):
    """The CPU's normals of every shape at D = 10 and D = 3, made once and left unchanged."""
    return {(M, S, D): cpu_normals(oracle, 7, 5, 3, M, S, D) for M, S in SHAPES for D in (10, 3)}


def _generation(c, z, S, dtype):
    smp = restate_sample(c, z, S=S, dtype=dtype)
    upd = restate_update(c["returns"], c["rankw"], c, smp["factor"], smp["failed"], z, c["consts"], S=S, dtype=dtype)
    return smp, upd


def test_the_crafted_populations_reach_every_branch(normals):
    M, S, D = 5, 64, 10
    E = 2 * (D + 1)
    c = crafted_cma(M, S, D, np.float64)
    smp, upd = _generation(c, normals[(M, S, D)], S, np.float64)
    r = c["returns"].reshape(S, M)
    mu = len(c["rankw"])
    assert mu == S // 2 and np.isnan(r[3, 0]) and r[5, 0] == np.inf and r[6, 0] == -np.inf
    bad = (np.arange(S) % 7 == 3) | (np.arange(S) % 11 == 5) | (np.arange(S) % 13 == 6)
    # the factor: fine, failing at column 0, at a later column, and a step size of 0
    assert smp["failed"].tolist() == [0, 0, 1, LATER + 1, E + 1]
    assert (smp["factor"][2:] == 0).all() and (np.triu(smp["factor"][0], 1) == 0).all() and (np.diag(smp["factor"][0]) > 0).all()
    low = np.tril(c["cov"][0])
    assert np.allclose(smp["factor"][0] @ smp["factor"][0].T, low + np.tril(low, -1).T, rtol=1e-12, atol=1e-12)
    w = smp["weights"].reshape(S, M, E)
    assert all(np.array_equal(w[:, m], np.broadcast_to(c["mean"][m].reshape(E), (S, E))) for m in (2, 3, 4)) and (w[:, 0] != c["mean"][0].reshape(E)).all()
    # validity, ranks and status: NaN and +-inf among the would-be parents, ties, -0 and +0, count < mu
    assert upd["count"].tolist() == [S - bad.sum(), 1, S - bad.sum(), S - bad.sum(), S - bad.sum()] and upd["status"].tolist() == [0, 1, 2, 2, 2]
    rank = upd["rank"].reshape(S, M)
    assert all(sorted(rank[:, m].tolist()) == list(range(S)) for m in range(M))                   # a permutation, whatever the lane is
    assert (rank[bad, 0] >= upd["count"][0]).all() and rank[bad, 0].tolist() == sorted(rank[bad, 0].tolist())
    good = np.flatnonzero(~bad)
    order = good[np.argsort(rank[good, 0])]
    assert (np.diff(r[order, 0]) <= 0).all() and len(set(r[good, 0].tolist())) < len(good) // 2   # descending, with ties ...
    tied = [a for a, b in zip(order[:-1], order[1:]) if r[a, 0] == r[b, 0]]
    assert tied and all(a < b for a, b in zip(order[:-1], order[1:]) if r[a, 0] == r[b, 0])      # ... that keep the lower s first
    zeros = good[r[good, 0] == 0]
    assert np.signbit(r[zeros, 0]).any() and not np.signbit(r[zeros, 0]).all() and sorted(zeros.tolist()) == zeros[np.argsort(rank[zeros, 0])].tolist()
    cut = r[order[mu - 1], 0]
    assert r[order[mu], 0] == cut                                                               # the cut goes through a tie
    assert rank[0, 1] == 0 and rank[1:, 1].tolist() == list(range(1, S))                         # invalid lanes: count + those below
    # status != 0: the state as it was, yw = 0, ps_norm = 0, growth = 1
    for m in (1, 2, 3, 4):
        assert all(np.array_equal(upd[k][m], c[k][m], equal_nan=True) for k in STATE), m
        assert (upd["yw"][m] == 0).all() and upd["ps_norm"][m] == 0 and upd["growth"][m] == 1
    assert upd["h"][0] and all((upd[k][0] != c[k][0]).any() for k in STATE)
    assert np.array_equal(upd["cov"][0], np.swapaxes(upd["cov"][0], 0, 1)) and np.isfinite(upd["cov"][0]).all()   # (the NaN above the diagonal was not read)
    # every role, where 257 populations of four samples have them: h false, sigma clamped at each bound
    M, S = 257, 4
    for D in (10, 3):
        c = crafted_cma(M, S, D, np.float64)
        smp, upd = _generation(c, normals[(M, S, D)], S, np.float64)
        roles = np.array([role(m, M) for m in range(M)])
        ran = upd["status"] == 0
        assert set(roles[ran]) == {PLAIN, STALLED, CLAMPED_HIGH, CLAMPED_LOW} and set(roles[upd["status"] == 1]) == {FEW_VALID}
        assert not upd["h"][ran & (roles == STALLED)].any() and not upd["h"][ran & (roles == CLAMPED_HIGH)].any()
        assert upd["h"][ran & (roles == PLAIN)].any() and upd["h"][ran & (roles == CLAMPED_LOW)].any()
        stalled = np.flatnonzero(roles == STALLED)
        k = c["consts"]
        assert np.array_equal(upd["p_c"][stalled], np.float64(k.a_c) * c["p_c"][stalled])          # the path is only shortened
        assert (upd["sigma"][roles == CLAMPED_HIGH] == SIGMA_MAX).all() and (upd["growth"][roles == CLAMPED_HIGH] > 1.01).all()
        low = upd["sigma"][roles == CLAMPED_LOW] == SIGMA_MIN                                   # (a path of two parents is now and then longer than chi)
        assert 2 * low.sum() > low.size and (upd["growth"][roles == CLAMPED_LOW][low] < 0.9999).all()
        inner = ran & (roles == PLAIN)
        assert ((upd["sigma"][inner] > SIGMA_MIN) & (upd["sigma"][inner] < SIGMA_MAX)).all()
    # every shape of the GPU tests runs, in float32 too
    for (m, s) in SHAPES:
        c = crafted_cma(m, s, 3, np.float32)
        smp, upd = _generation(c, normals[(m, s, 3)], s, np.float32)
        assert np.isfinite(upd["mean"]).all() and (upd["status"] == 0).any() and np.isfinite(smp["weights"]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_against_a_plain_statement(normals, dtype):
    """float64: the restatement (columns, chains, 64 partials, the tree) against np.linalg.cholesky, np.argsort and einsum;
    float32: the restatement in float32 against itself in float64 on the same rounded inputs.  rank, count and status are
    equal exactly."""
    worst = {k: 0.0 for k in MEASURED[dtype]}
    for (M, S) in SHAPES:
        for D in (10, 3):
            c = crafted_cma(M, S, D, dtype)
            z = normals[(M, S, D)].astype(dtype)
            smp, upd = _generation(c, z, S, dtype)
            got = dict(upd, factor=smp["factor"], weights=smp["weights"])
            if dtype is np.float64:
                want = plain_generation(c["returns"], c["rankw"], c, z, c["consts"], S=S)
                assert np.array_equal(smp["failed"] != 0, want["failed"]), (M, S, D)
            else:
                s64, want = _generation(c, z, S, np.float64)
                want = dict(want, factor=s64["factor"], weights=s64["weights"])
                assert np.array_equal(smp["failed"], s64["failed"]), (M, S, D)
            for name in ("rank", "count", "status"):
                assert np.array_equal(got[name], want[name]), (M, S, D, name)
            ran = got["status"] == 0
            for name in worst:
                if name == "weights":
                    a, b = got[name].reshape(S, M, -1)[:, ran], want[name].reshape(S, M, -1)[:, ran]
                elif name == "cov":                                                 # (what is not read is not compared: the NaN above the diagonal)
                    a, b = got[name][ran], want[name][ran]
                    assert np.array_equal(a, np.swapaxes(a, 1, 2))
                else:
                    a, b = got[name][ran], want[name][ran]
                if a.size and np.abs(b).max() > 0:
                    worst[name] = max(worst[name], _far(a, b))
    bound = {k: MARGIN * v for k, v in MEASURED[dtype].items()}
    print(f"[cma restatement, {dtype.__name__}] worst relative distance {worst}, bound {bound}")
    for name in worst:
        assert worst[name] <= bound[name], (name, worst[name], bound[name])
    assert all(v < (1e-11 if dtype is np.float64 else 1e-3) for v in bound.values())


# ---------------------------------------------------------------------------------------
# the constants
# ---------------------------------------------------------------------------------------
def test_constants_are_hansens_defaults():
    from gym_os2r_amd import cma
    for E, S in ((22, 32), (22, 14), (8, 4), (26, 4096), (4, 2)):
        rankw, k = cma.constants(E, S)
        mu = S // 2
        assert len(rankw) == mu and abs(sum(rankw) - 1.0) < 1e-15 and all(a > b > 0 for a, b in zip(rankw[:-1], rankw[1:]))
        raw = np.log(mu + 0.5) - np.log(np.arange(mu) + 1.0)
        assert np.allclose(rankw, raw / raw.sum(), rtol=1e-14, atol=0)
        mu_eff = 1.0 / np.sum(np.square(rankw))
        assert 1.0 <= mu_eff <= mu + 1e-12
        c_sigma = (mu_eff + 2) / (E + mu_eff + 5)
        d_sigma = 1 + 2 * max(0.0, math.sqrt((mu_eff - 1) / (E + 1)) - 1) + c_sigma
        c_c = (4 + mu_eff / E) / (E + 4 + 2 * mu_eff / E)
        c_1 = 2 / ((E + 1.3) ** 2 + mu_eff)
        c_mu = min(1 - c_1, 2 * (mu_eff - 2 + 1 / mu_eff) / ((E + 2) ** 2 + mu_eff))
        chi = math.sqrt(E) * (1 - 1 / (4 * E) + 1 / (21 * E * E))
        want = dict(a_sigma=1 - c_sigma, b_sigma=math.sqrt(c_sigma * (2 - c_sigma) * mu_eff), a_c=1 - c_c, b_c=math.sqrt(c_c * (2 - c_c) * mu_eff),
                    k0_moving=1 - c_1 - c_mu, k0_stalled=1 - c_1 - c_mu + c_1 * c_c * (2 - c_c), c_1=c_1, c_mu=c_mu, g_sigma=c_sigma / d_sigma, chi=chi,
                    hsig_bound=(1.4 + 2 / (E + 1)) * chi * math.sqrt(1 - (1 - c_sigma) ** 2), sigma_min=1e-8, sigma_max=1.0)
        assert [n for n, _ in k._fields_] == list(cma.CONSTANT_NAMES) and set(want) == set(cma.CONSTANT_NAMES)
        for name, v in want.items():
            assert math.isclose(getattr(k, name), v, rel_tol=1e-13, abs_tol=1e-300), (E, S, name)
        assert 0 < k.c_1 and 0 <= k.c_mu and 0 <= k.k0_moving < k.k0_stalled <= 1 and 0 < k.a_sigma < 1 and 0 < k.a_c < 1
        bounds = [cma.constants(E, S, age=a)[1].hsig_bound for a in (0, 1, 2, 10, 1000)]
        assert all(a < b for a, b in zip(bounds[:-2], bounds[1:-1])) and bounds[-2] <= bounds[-1] == (1.4 + 2 / (E + 1)) * chi
    rankw, k = cma.constants(22, 32, parents=5, age=2, sigma_min=1e-3, sigma_max=2.0)
    assert len(rankw) == 5 and k.sigma_min == 1e-3 and k.sigma_max == 2.0
    for bad in (0, 33):
        with pytest.raises(ValueError, match="parents"):
            cma.constants(22, 32, parents=bad)


# ---------------------------------------------------------------------------------------
# the restatement as an optimiser
# ---------------------------------------------------------------------------------------
N_OPT, S_OPT, CONDITION = 22, 32, 1e6
OPT_SEEDS = (1, 2, 3, 4, 5)
# Generations the float64 restatement took to bring the ellipsoid below 1e-8 f(x0) from x0 = 1, sigma0 = 0.5, one population per
# seed, measured on the CPU this test was written on (np.random normals took 601 to 704, the issue says):
OPT_MEASURED = {1: 628, 2: 625, 3: 630, 4: 631, 5: 708}
OPT_BUDGET = 2 * max(OPT_MEASURED.values())


def _ellipsoid(x):
    scale = CONDITION ** (np.arange(N_OPT) / (N_OPT - 1.0))
    return np.sum(scale * np.square(x), axis=-1)


def minimise(oracle, seeds, budget, adapt=True):
    """Cholesky-CMA-ES through restate_sample and restate_update, a population per seed, normals from the oracle's uniform2.
    -> per seed the first generation count at which the mean's value is below 1e-8 f(x0), or None within `budget`."""
    from gym_os2r_amd import cma
    D, M, S = N_OPT // 2 - 1, len(seeds), S_OPT
    E = 2 * (D + 1)
    state = dict(mean=np.ones((M, 2, D + 1)), sigma=np.full(M, 0.5), cov=np.tile(np.eye(E), (M, 1, 1)), p_sigma=np.zeros((M, E)), p_c=np.zeros((M, E)))
    target = 1e-8 * _ellipsoid(np.ones(E))
    done = [None] * M
    for g in range(budget):
        z = np.concatenate([cpu_normals(oracle, seed, 0, g, 1, S, D) for seed in seeds], axis=1).reshape(S, M, 2, D + 1).reshape(S * M, 2, D + 1)
        rankw, k = cma.constants(E, S, age=g, sigma_min=1e-300, sigma_max=1e300)
        if not adapt:
            k.c_1, k.c_mu, k.k0_moving, k.k0_stalled = 0.0, 0.0, 1.0, 1.0
        smp = restate_sample(state, z, S=S, dtype=np.float64)
        assert not smp["failed"].any(), (g, smp["failed"])
        returns = -_ellipsoid(smp["weights"].reshape(S * M, E))
        upd = restate_update(returns, rankw, state, smp["factor"], smp["failed"], z, k, S=S, dtype=np.float64)
        assert not upd["status"].any()
        state = {name: upd[name] for name in STATE}
        value = _ellipsoid(state["mean"].reshape(M, E))
        for m in range(M):
            if done[m] is None and value[m] < target:
                done[m] = g + 1
        if all(d is not None for d in done):
            break
    return done


def test_the_restatement_minimises_an_ellipsoid_and_the_covariance_does_the_work(oracle):
    """n = 22 (D = 10), condition 1e6, S = 32, five seeds: every one is below 1e-8 f(x0) within twice the largest measured
    count; without covariance adaptation (c_1 = c_mu = 0, the step size still adapts) the first seed is not, in the same budget."""
    took = minimise(oracle, OPT_SEEDS, OPT_BUDGET)
    print(f"[cma optimiser] generations to 1e-8 f(x0) by seed: {dict(zip(OPT_SEEDS, took))}, measured {OPT_MEASURED}, budget {OPT_BUDGET}")
    assert all(t is not None and t <= OPT_BUDGET for t in took), took
    plain = minimise(oracle, OPT_SEEDS[:1], OPT_BUDGET, adapt=False)
    print(f"[cma optimiser] without covariance adaptation: {plain}")
    assert plain == [None]


# ---------------------------------------------------------------------------------------
# header, table, exports, resources
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import _lib, cma, control, es
    protos = _prototypes("os2r_cma.h", "os2rk")
    assert [p[0] for p in protos] == list(cma.ENTRY_POINTS) == NAMES
    lib = cma.load()
    for name, ret, args in protos:
        argtypes = cma.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2rk_last_error" else C.c_int)
    sample, update = protos[2][2], protos[3][2]
    assert sample[:7] == ["const Os2rControlLayout* layout", "int64_t npops", "int32_t nsamples", "uint32_t flags", "uint64_t seed",
                          "uint32_t pop_offset", "uint32_t generation"]
    assert len(sample) == 15 and sample[-1] == "void* stream" and sample[-2] == "void* z_dev"
    assert update[:8] == ["const Os2rControlLayout* layout", "int64_t npops", "int32_t nsamples", "int32_t mu", "uint32_t flags", "uint64_t seed",
                          "uint32_t pop_offset", "uint32_t generation"]
    assert len(update) == 30 and update[17] == "const Os2rkCmaConstants* constants" and update[-1] == "void* stream"
    assert cma.ENTRY_POINTS["os2rk_cma_update"][17] is C.POINTER(cma.Os2rkCmaConstants)
    header = _header("os2r_cma.h")
    assert re.search(r"#define OS2R_CMA_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert len(re.findall(r"#include", header)) == 1
    assert lib.os2rk_abi_version() == cma.ABI_VERSION == 1
    assert cma.STREAM == int(re.search(r"#define OS2RK_STREAM (\d+)", header).group(1)) == 7 == es.STREAM + 1
    assert cma.CHUNKS == int(re.search(r"#define OS2RK_CHUNKS (\d+)", header).group(1)) == CHUNKS
    assert cma.MAX_SAMPLES == int(re.search(r"#define OS2RK_MAX_SAMPLES (\d+)", header).group(1)) == 2 ** 27 - 1
    # the struct of the header is the ctypes one, field by field
    body = re.sub(r"/\*.*?\*/", " ", re.search(r"typedef struct Os2rkCmaConstants \{(.*?)\} Os2rkCmaConstants;", header, re.S).group(1), flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("double", "").split(",")]
    assert fields == list(cma.CONSTANT_NAMES) == [n for n, _ in cma.Os2rkCmaConstants._fields_] and C.sizeof(cma.Os2rkCmaConstants) == 8 * 13
    assert cma.Os2rControlLayout is control.Os2rControlLayout and cma.layout is control.layout
    assert not set(cma.ENTRY_POINTS) & (set(_lib.ENTRY_POINTS) | set(_lib.RECORD_ENTRY_POINTS)) and len(_lib.ENTRY_POINTS) == 35
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", cma.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "libos2r_cma.map")) as f:
        assert re.search(r"global:\s*os2rk_\*;\s*local:\s*\*;", f.read())
    # the header names no other companion library (their tests forbid it) and no other header declares anything of this one
    for word in FORBIDDEN:
        assert word not in header.lower(), word
    flat = " ".join(header.replace("\n *", " ").split())
    assert "adjacent-pair tree" in flat and "in ascending order onto 0" in flat and "NOT contracted" in flat
    for line in ("mirrored or antithetic sampling", "active (negative-weight) CMA", "sep- and LM-CMA", "restarts and population-size schedules (IPOP / BIPOP)",
                 "constants per population", "an eigendecomposition or condition-number output", "MLP and scheduled policies",
                 "cost-valued (minimising) inputs", "in-place state updates", "the caller swaps two state sets"):
        assert line in flat, line
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "os2r_cma.h":
            assert "os2rk_" not in _header(name).lower() and "os2r_cma.h" not in _header(name).lower(), name
    assert "covariance adaptation (CMA-ES) (since built as `libos2r_cma.so`)" in " ".join(_header("os2r_es.h").replace("\n *", " ").split())
    # the counter RNG is the stepper's, included, not copied
    src = _csrc("os2r_cma.hpp")
    assert '#include "os2r_es.hpp"' in src and "normal2(" in src and "philox4x32_10" not in src
    assert '#include "os2r_device.hpp"' in _csrc("os2r_es.hpp") and "kStreamPolicyNoise = 5 }" in _csrc("os2r_device.hpp")


KERNELS = ("cma_factor_kernel", "cma_sample_kernel", "cma_rank_kernel", "cma_sum_kernel")


def test_kernel_resources():
    """Exactly eight kernels, the four of os2r_cma.hpp in float and double, are in the built library and none uses scratch:
    private_segment_fixed_size 0, no VGPR or SGPR spill and no AGPRs in the code-object metadata.  The VGPR counts are printed
    (and recorded in DESIGN.md section 4).  The occupancy the kernels are designed for: the sum kernel is a workgroup of
    sixteen waves, four a SIMD, which 128 VGPRs allow (26 accumulators a lane, 52 registers in double, beside the Box-Muller
    pair); the factor, sample and rank kernels stay at four waves a SIMD or more as well.  LDS: the factor's 26 x 26 entries;
    the sample kernel's 512 normals; the sum kernel's 79 rows of a round, the factor, the 403 totals, the two paths, two
    scalars, 64 flags and the 416 row pairs."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import cma
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(cma.LIB_PATH)
    meta = kernel_meta.kernel_meta(cma.LIB_PATH)
    assert len(meta) == 8, sorted(meta)
    for kernel in KERNELS:
        for real, size in (("float", 4), ("double", 8)):
            (name,) = [k for k in meta if f"{kernel}<{real}>" in k]
            m = meta[name]
            print(f"{kernel}<{real}>: {m['vgpr_count']} VGPRs, {m['sgpr_count']} SGPRs, {m['group_segment_fixed_size']} bytes of LDS")
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
            assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 128, (name, m)
            lds = {"cma_factor_kernel": 676 * size, "cma_sample_kernel": 512 * size, "cma_rank_kernel": 0,
                   "cma_sum_kernel": (79 * 64 + 676 + 403 + 26 + 26 + 2) * size + 4 * (64 + 416)}[kernel]
            assert lds <= m["group_segment_fixed_size"] <= lds + 64, (name, m, lds)              # (the arrays' own alignment)


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
        err = lib.os2rk_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(prefix), (list(kw), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases})                        # each cause has a text of its own
    assert not any(buf)                                                   # a refused call wrote nothing
    return seen


def _source_checks(unit_function):
    """The source: no HIP call and every refusal of an argument before check_device."""
    body = _function(_csrc("os2r_cma_capi.hip"), "int " + unit_function)
    first_hip = body.index("check_device(")
    assert not re.search(HIP_CALL, body[:first_hip]) and body.index("DeviceGuard") > first_hip and body.index("auto launch") > first_hip
    fails = [m.start() for m in re.finditer(r"fail\(OS2R_ERR_INVALID", body)]
    assert fails and all(i < first_hip for i in fails)
    for helper in ("overlap_refusal", "null_refusal", "constants_refusal", r"const char\* shape_refusal"):
        text = _function(_csrc("os2r_cma_capi.hip"), helper if helper.startswith("const") else r"[a-z:* ]+ " + helper)
        assert not re.search(HIP_CALL + r"|check_device|DeviceGuard|launch", text), helper


def _planned(names_and_sizes, split_at):
    where, nxt = {}, 0
    for name, n in names_and_sizes.items():
        if name == split_at:
            nxt = 8192
        where[name] = nxt
        nxt += (n + 1) & ~1                                  # every array starts at a pair
    assert nxt < 16000
    return where


def test_sample_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import cma
    lib = cma.load()
    Lay = _layouts()
    M, S, D = 2, 3, 4
    E, SM = 2 * (D + 1), S * M
    buf = (C.c_double * 16384)()
    base = (C.addressof(buf) + 15) & ~15
    at = lambda i: C.c_void_p(base + 8 * i)
    size = dict(mean=M * E, sigma=M, cov=M * E * E, factor=M * E * E, failed=M, weights=SM * E, z=SM * E)
    where = _planned(size, "factor")
    good = dict(lay=Lay(), M=M, S=S, flags=0, seed=7, off=0, gen=1, **{k: at(where[k]) for k in size})
    name = "os2rk_cma_sample"
    assert len(good) + 1 == len(cma.ENTRY_POINTS[name])
    assert lib.os2rk_cma_sample(*[None if _is_pointer(t) else 0 for t in cma.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rk_last_error() == b"os2rk_cma_sample: null layout"
    end = lambda n: where[n] + size[n] - 1
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(nq=1)), b"nq must be 2..5"),
             (dict(lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"), (dict(lay=Lay(obs_dim=13)), b"obs_dim must be 1..12"),
             (dict(M=0), b"npops must be >= 1"), (dict(M=-3), b"npops must be >= 1"), (dict(S=1), b"nsamples must be >= 2"),
             (dict(S=-1), b"nsamples must be >= 2"), (dict(S=2 ** 27, M=1), b"nsamples must be < 2^27"),
             (dict(S=2 ** 27 - 1, M=17), b"nsamples * npops exceeds 2^31 - 1"), (dict(S=2, M=2 ** 30), b"nsamples * npops exceeds 2^31 - 1"),
             (dict(M=2 ** 62), b"nsamples * npops exceeds 2^31 - 1"), (dict(flags=1), b"unknown flag bits"), (dict(flags=0x80000000), b"unknown flag bits"),
             (dict(mean=None), b"null mean_dev"), (dict(sigma=None), b"null sigma_dev"), (dict(cov=None), b"null cov_dev"),
             (dict(factor=None), b"null factor_dev"), (dict(failed=None), b"null failed_dev"), (dict(weights=None), b"null weights_dev"),
             (dict(mean=at(where["mean"] + 1)), b"mean_dev must be aligned to a pair"), (dict(weights=at(where["weights"] + 1)), b"weights_dev must be aligned to a pair"),
             (dict(z=at(where["z"] + 1)), b"z_dev must be aligned to a pair"),
             (dict(lay=Lay(abi.F32), mean=C.c_void_p(base + 4)), b"mean_dev must be aligned to a pair"),
             (dict(factor=at(end("cov") - 1)), b"factor_dev overlaps cov_dev"), (dict(factor=at(where["mean"])), b"factor_dev overlaps mean_dev"),
             (dict(failed=at(where["sigma"])), b"failed_dev overlaps sigma_dev"), (dict(failed=at(end("factor"))), b"failed_dev overlaps factor_dev"),
             (dict(weights=at(where["mean"])), b"weights_dev overlaps mean_dev"), (dict(weights=at(end("failed") - 1)), b"weights_dev overlaps failed_dev"),
             (dict(z=at(where["cov"])), b"z_dev overlaps cov_dev"), (dict(z=at(end("weights") - 1)), b"z_dev overlaps weights_dev")]
    seen = _refused(lib, lib.os2rk_cma_sample, b"os2rk_cma_sample: ", good, cases, buf)
    assert len(seen) == 26
    # the edges are taken: nothing is left to refuse but the device, and no call is let through to one
    edges = [dict(S=2 ** 27 - 1, weights=C.c_void_p(2 ** 44), z=None), dict(z=None), dict(S=2),
             dict(seed=2 ** 64 - 1, off=2 ** 32 - 1, gen=2 ** 32 - 1), dict(z=at(where["weights"] + size["weights"]))]
    for kw in edges:                                  # (device 1000 is never there, with a GPU or without)
        a = dict(good, **dict(kw, lay=Lay(device=1000)))
        assert lib.os2rk_cma_sample(*[a[k] for k in good], None) == abi.ERR_NO_DEVICE and lib.os2rk_last_error().startswith(b"os2rk_cma_sample: "), kw
    assert not any(buf)
    _source_checks(name)


def test_update_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import cma
    lib = cma.load()
    Lay = _layouts()
    M, S, D, mu = 2, 4, 4, 2
    E, SM = 2 * (D + 1), S * M
    buf = (C.c_double * 16384)()
    base = (C.addressof(buf) + 15) & ~15
    at = lambda i: C.c_void_p(base + 8 * i)
    nan, inf = float("nan"), float("inf")
    size = dict(returns=SM, rankw=mu, mean=M * E, sigma=M, cov=M * E * E, p_sigma=M * E, p_c=M * E, factor=M * E * E, failed=M,
                mean_out=M * E, sigma_out=M, cov_out=M * E * E, p_sigma_out=M * E, p_c_out=M * E, count=M, status=M, rank=SM, yw=M * E, ps_norm=M, growth=M)
    where = _planned(size, "mean_out")
    _, consts = cma.constants(E, S)

    def K(**kw):
        k = cma.Os2rkCmaConstants.from_buffer_copy(consts)
        for n, v in kw.items():
            setattr(k, n, v)
        return C.byref(k)
    order = list(size)
    good = dict(lay=Lay(), M=M, S=S, mu=mu, flags=0, seed=7, off=0, gen=1, **{k: at(where[k]) for k in order[:9]}, consts=K(),
                **{k: at(where[k]) for k in order[9:]})
    name = "os2rk_cma_update"
    assert len(good) + 1 == len(cma.ENTRY_POINTS[name])
    assert lib.os2rk_cma_update(*[None if _is_pointer(t) else 0 for t in cma.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rk_last_error() == b"os2rk_cma_update: null layout"
    end = lambda n: where[n] + size[n] - 1
    required = [n for n in order if n not in ("yw", "ps_norm", "growth")]
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(nq=6)), b"nq must be 2..5"),
             (dict(lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"), (dict(M=0), b"npops must be >= 1"), (dict(S=1), b"nsamples must be >= 2"),
             (dict(S=2 ** 27, M=1), b"nsamples must be < 2^27"), (dict(S=2 ** 27 - 1, M=17), b"nsamples * npops exceeds 2^31 - 1"),
             (dict(mu=0), b"mu must be >= 1"), (dict(mu=-2 ** 31), b"mu must be >= 1"), (dict(mu=S + 1), b"mu must be <= nsamples"),
             (dict(flags=2), b"unknown flag bits"), (dict(consts=None), b"null constants")]
    cases += [(dict(consts=K(**{n: bad})), b"constants->" + n.encode() + b" must be finite") for n in cma.CONSTANT_NAMES for bad in (nan, inf, -inf)]
    cases += [(dict(**{n: None}), b"null " + n.encode() + b"_dev") for n in required]
    cases += [(dict(mean=at(where["mean"] + 1)), b"mean_dev must be aligned to a pair"),
              (dict(mean_out=at(where["mean_out"] + 1)), b"mean_out_dev must be aligned to a pair"),
              (dict(yw=at(where["yw"] + 1)), b"yw_dev must be aligned to a pair"),
              # an output over an input, from both sides; over another output; the optional ones too
              (dict(mean_out=at(where["mean"])), b"mean_out_dev overlaps mean_dev"), (dict(mean_out=at(end("returns") - 1)), b"mean_out_dev overlaps returns_dev"),
              (dict(sigma_out=at(where["rankw"])), b"sigma_out_dev overlaps rankw_dev"), (dict(cov_out=at(where["cov"])), b"cov_out_dev overlaps cov_dev"),
              (dict(p_sigma_out=at(where["p_sigma"])), b"p_sigma_out_dev overlaps p_sigma_dev"), (dict(p_c_out=at(end("p_c"))), b"p_c_out_dev overlaps p_c_dev"),
              (dict(count=at(where["failed"])), b"count_dev overlaps failed_dev"), (dict(status=at(end("factor"))), b"status_dev overlaps factor_dev"),
              (dict(rank=at(where["sigma"])), b"rank_dev overlaps sigma_dev"), (dict(yw=at(where["mean"])), b"yw_dev overlaps mean_dev"),
              (dict(ps_norm=at(where["returns"])), b"ps_norm_dev overlaps returns_dev"), (dict(growth=at(where["sigma"])), b"growth_dev overlaps sigma_dev"),
              (dict(sigma_out=at(end("mean_out"))), b"sigma_out_dev overlaps mean_out_dev"), (dict(status=at(where["count"])), b"status_dev overlaps count_dev"),
              (dict(rank=at(where["status"])), b"rank_dev overlaps status_dev"), (dict(yw=at(where["rank"])), b"yw_dev overlaps rank_dev"),
              (dict(growth=at(where["ps_norm"])), b"growth_dev overlaps ps_norm_dev")]
    seen = _refused(lib, lib.os2rk_cma_update, b"os2rk_cma_update: ", good, cases, buf)
    assert len(required) == 17 and len(seen) == 12 + 13 + len(required) + 3 + 17
    edges = [dict(mu=1), dict(mu=S), dict(yw=None, ps_norm=None, growth=None), dict(seed=2 ** 64 - 1, off=2 ** 32 - 1, gen=2 ** 32 - 1),
             dict(consts=K(sigma_min=0.0, sigma_max=1e300, c_1=0.0, c_mu=0.0)), dict(sigma_out=at(where["mean_out"] + size["mean_out"])),
             dict(S=2 ** 27 - 1, mu=2 ** 27 - 1, returns=C.c_void_p(2 ** 44), rank=C.c_void_p(2 ** 45), rankw=C.c_void_p(2 ** 46))]
    for kw in edges:
        a = dict(good, **dict(kw, lay=Lay(device=1000)))
        assert lib.os2rk_cma_update(*[a[k] for k in good], None) == abi.ERR_NO_DEVICE and lib.os2rk_last_error().startswith(b"os2rk_cma_update: "), kw
    assert not any(buf)
    _source_checks(name)


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
    from gym_os2r_amd import cma
    from gym_os2r_amd.sim import HipSim
    for method in ("cma_init", "cma_sample", "cma_sample_into", "cma_update", "cma_update_into"):
        assert callable(getattr(HipSim, method))
    assert "Suttorp, Hansen and Igel 2009" in HipSim.cma_update.__doc__ and "regenerated" in HipSim.cma_update.__doc__

    def no_load():
        raise AssertionError("a refused call reached cma.load")
    monkeypatch.setattr(cma, "load", no_load)
    f64, i32 = torch.float64, torch.int32
    s = _bare(f64)
    M, S, D = 2, 4, 4
    E, N = 2 * (D + 1), S * M
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    # cma_init: the state's shapes, cov = I, zero paths
    with pytest.raises(ValueError, match="^cma_init: "):
        s.cma_init(z(M, 2, D), 0.5)
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, None, "x"):
        with pytest.raises(ValueError, match="^cma_init: "):
            s.cma_init(z(M, 2, D + 1), bad)
    state = s.cma_init(torch.ones(M, 2, D + 1, dtype=f64), 0.5)
    assert [tuple(t.shape) for t in state] == [(M, 2, D + 1), (M,), (M, E, E), (M, E), (M, E)] and all(t.dtype == f64 for t in state)
    assert (state[0] == 1).all() and (state[1] == 0.5).all() and torch.equal(state[2], torch.eye(E, dtype=f64).repeat(M, 1, 1))
    assert (state[3] == 0).all() and (state[4] == 0).all()
    assert torch.equal(s.cma_init(z(M, 2, D + 1), torch.tensor([0.1, 0.2], dtype=f64))[1], torch.tensor([0.1, 0.2], dtype=f64))
    factor, failed, weights, zs = z(M, E, E), z(M, dtype=i32), z(N, 2, D + 1), z(N, 2, D + 1)
    ok = dict(samples=S, generation=1, seed=3)

    def sample_into(*args, **kw):
        with pytest.raises(ValueError, match="^cma_sample: "):
            s.cma_sample_into(*args, **dict(ok, **kw))

    def sample(*args, **kw):
        with pytest.raises(ValueError, match="^cma_sample: "):
            s.cma_sample(*args, **dict(ok, **kw))
    words = (dict(samples=1), dict(samples=0), dict(samples=2.0), dict(samples=True), dict(samples=None), dict(samples=2 ** 27),
             dict(generation=-1), dict(generation=2 ** 32), dict(generation=1.0), dict(generation=True),
             dict(pop_offset=-1), dict(pop_offset=2 ** 32), dict(pop_offset="0"), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(seed=True))
    for kw in words:
        sample_into(state, factor, failed, weights, **kw)
        sample(state, **kw)
    swap = lambda seq, i, t: tuple(t if j == i else a for j, a in enumerate(seq))
    bad_states = (None, state[:4], swap(state, 0, None), swap(state, 0, z(M, 2, D)), swap(state, 1, z(M + 1)), swap(state, 2, z(M, E, E + 1)),
                  swap(state, 3, z(M, E).float()), swap(state, 4, z(E, M).t()), swap(state, 2, state[2].numpy()), swap(state, 1, z(M).to("meta")))
    for bad in bad_states:
        sample_into(bad, factor, failed, weights)
        sample(bad)
    for args in ((None, failed, weights), (factor, None, weights), (factor, failed, None), (z(M, E, E + 1), failed, weights), (factor.float(), failed, weights),
                 (factor, z(M), weights), (factor, z(M + 1, dtype=i32), weights), (factor, failed, z(N + 1, 2, D + 1)), (factor, failed, z(N, D + 1, 2)),
                 (factor, failed, weights.to("meta")), (factor.to("meta"), failed, weights)):
        sample_into(state, *args)
    for bad in (z(N + 1, 2, D + 1), zs.float(), z(N, D + 1, 2), zs.to("meta")):
        sample_into(state, factor, failed, weights, z=bad)
    pool = z(8192)
    sample_into(swap(state, 0, pool[1:1 + M * E].reshape(M, 2, D + 1)), factor, failed, weights)            # not aligned to a pair
    sample_into(state, factor, failed, pool[1:1 + N * E].reshape(N, 2, D + 1))
    sample_into(state, factor, failed, weights, z=pool[3:3 + N * E].reshape(N, 2, D + 1))
    sample_into(state, state[2], failed, weights)                                                          # overlap
    sample_into(state, factor, failed, pool[:N * E].reshape(N, 2, D + 1), z=pool[N * E - 2:2 * N * E - 2].reshape(N, 2, D + 1))
    sample_into(swap(state, 0, pool[:M * E].reshape(M, 2, D + 1)), factor, failed, pool[M * E - 2:M * E - 2 + N * E].reshape(N, 2, D + 1))

    returns, count, status, rank = z(N), z(M, dtype=i32), z(M, dtype=i32), z(N, dtype=i32)
    new = tuple(torch.zeros_like(t) for t in state)
    rankw_list, consts = cma.constants(E, S)
    rankw = torch.tensor(rankw_list, dtype=f64)
    full = (returns, state, factor, failed, new, count, status, rank)
    uok = dict(samples=S, generation=1, rankw=rankw, constants=consts, seed=3)

    def update_into(*args, **kw):
        with pytest.raises(ValueError, match="^cma_update: "):
            s.cma_update_into(*args, **dict(uok, **kw))

    def update(*args, **kw):
        with pytest.raises(ValueError, match="^cma_update: "):
            s.cma_update(*args, **dict(dict(samples=S, generation=1, seed=3), **kw))
    for kw in words:
        update_into(*full, **kw)
        update(returns, state, factor, failed, **kw)
    for bad in (None, rankw_list, z(0), z(S + 1), z(2, 1), rankw.float(), rankw.to("meta")):
        update_into(*full, rankw=bad)
    broken = cma.Os2rkCmaConstants.from_buffer_copy(consts)
    broken.chi = float("nan")
    for bad in (None, dict(), broken):
        update_into(*full, constants=bad)
    for i in (0, 2, 3, 5, 6, 7):
        update_into(*swap(full, i, None))
    for bad in bad_states:
        update_into(*swap(full, 1, bad))
        update_into(*swap(full, 4, bad))
        update(returns, bad, factor, failed)
    for args in (swap(full, 0, z(N + 1)), swap(full, 0, z(S, M)), swap(full, 0, returns.float()), swap(full, 0, returns.numpy()),
                 swap(full, 2, z(M, E, E - 1)), swap(full, 3, z(M)), swap(full, 4, tuple(torch.zeros(M + 1, *t.shape[1:], dtype=f64) for t in state)),
                 swap(full, 5, z(M)), swap(full, 5, z(M + 1, dtype=i32)), swap(full, 6, z(M, dtype=torch.int64)), swap(full, 7, z(N)),
                 swap(full, 7, z(S, M, dtype=i32)), swap(full, 0, returns.to("meta")), swap(full, 7, rank.to("meta")),
                 swap(full, 4, state), swap(full, 4, swap(new, 2, state[2])), swap(full, 6, count), swap(full, 4, swap(new, 1, returns[:M])),
                 swap(full, 4, swap(new, 0, pool[1:1 + M * E].reshape(M, 2, D + 1)))):
        update_into(*args)
    for kw in (dict(yw=z(M, 2, D)), dict(yw=new[0]), dict(yw=z(M, 2, D + 1).float()), dict(yw=pool[1:1 + M * E].reshape(M, 2, D + 1)),
               dict(ps_norm=z(M + 1)), dict(ps_norm=new[1]), dict(growth=z(M, dtype=i32)), dict(growth=state[1])):
        update_into(*full, **kw)
    for kw in (dict(parents=0), dict(parents=S + 1), dict(parents=1.0), dict(parents=True), dict(age=-1), dict(age=1.5), dict(age=True),
               dict(sigma_min=-1.0), dict(sigma_min=float("nan")), dict(sigma_max=float("inf")), dict(sigma_min=1.0, sigma_max=0.5), dict(sigma_max=True)):
        update(returns, state, factor, failed, **kw)
    for args in ((None, state, factor, failed), (z(N + 2), state, factor, failed), (returns, state, None, failed), (returns, state, factor, z(M))):
        update(*args)
    # what passes every check reaches the loader, and only then (the bare handle has no cfg to fill a layout from)
    with pytest.raises(AttributeError):
        s.cma_sample_into(state, factor, failed, weights, z=zs, **ok)
    with pytest.raises(AttributeError):
        s.cma_update_into(*full, yw=z(M, 2, D + 1), ps_norm=z(M), growth=z(M), **uok)
    with pytest.raises(AttributeError):
        s.cma_update(returns, state, factor, failed, S, 1, parents=1, age=0, want_yw=True, want_norm=True, want_growth=True)
