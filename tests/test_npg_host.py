"""libos2r_npg.so (include/os2r_npg.h): the host side -- the numpy restatement of the natural-gradient step the GPU tests compare
with (`restate_npg`), the crafted inputs of the GPU tests (`crafted_npg`) and the branches they reach, the restatement against
np.linalg.solve in float64 and in float32 against its own float64 result, the trust-region property (the mean divergence of
the step, formed directly from the observations, is kl), the identity with `restate_fit` of tests/test_critic_host.py (one open
mask, sigma = 1: the same moments bit for bit), the header against the one table of gym_os2r_amd/npg.py, the exports of the
library, the resources of the eight kernels in the built library, every refusal of os2rn_natural_step through ctypes without a
device, and the argument checks of HipSim.natural_step that need no device.  No GPU needed."""
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
from test_critic_host import moment_index, restate_fit  # noqa: E402
from test_pg_host import CHUNKS, NONE_VALID, chunked_sum, crafted_pg  # noqa: E402

NAMES = ["os2rn_abi_version", "os2rn_last_error", "os2rn_natural_step"]
DAMPING, KL = 1e-3, 0.01
CLIPPED = 1                             # the policy whose component 1 is clipped on every step (where P > 1)
# K, P, S, D of the GPU tests (tests/test_gpu_npg.py): a wave of lanes that is not full, P = 3 divides nothing; the wave sum with
# partials of up to three terms at one policy; the fewest steps and the smallest D with exactly 64 samples (the few-samples sum
# at its boundary); S = 1 (the per-environment layout) with the largest D
SHAPES = [(7, 3, 5, 10), (3, 1, 130, 10), (1, 2, 64, 1), (9, 5, 1, 12)]
# The largest relative distance (the largest difference over the largest entry of the reference) measured on the CPU this test
# was written on, on the inputs of `plain_npg` (observations ~ N(0, 1), D = 10, 4 policies x 24 samples x 12 steps: K S = 288 >=
# 8 (D + 1)); the tests print them.  step, dir: of the restatement in float64 from np.linalg.solve on the same A, and in float32
# from the float64 restatement; kl: of the mean divergence of the float64 step, formed directly from the observations, from kl.
# The bound is MARGIN x that.
MEASURED = {np.float64: dict(step=8.569e-16, dir=8.350e-16, kl=8.882e-16),
            np.float32: dict(step=1.948e-7, dir=1.899e-7)}
MARGIN = 8
FORBIDDEN = ("os2rg_", "os2r_pg", "os2rv_", "os2r_critic", "os2ro_", "os2r_ppo", "os2rx_", "os2r_cem", "os2ru_", "os2r_ukf", "os2re_",
             "os2r_ekf", "os2rp_", "os2r_pf", "os2rm_", "mppi", "os2rt_", "steer", "line_search")


# ---------------------------------------------------------------------------------------
# the restatement of include/os2r_npg.h (needs no device)
# ---------------------------------------------------------------------------------------
def restate_npg(obs, sigma, grad, *, P, dtype, obs0=None, action=None, tanh=False, length=None, lsig_grad=None, damping=DAMPING, kl=KL):
    """include/os2r_npg.h, steps 1-3, in numpy and in `dtype`.  obs [K, N, D], action [K, N, 2], sigma [2] or [2, N], grad
    [2, D+1, P], lsig_grad [2, P] or None.
    -> dict(step, dir [2, D+1, P], lsig_step [2, P] (None without lsig_grad), beta, quad [P], failed [3, P], steps [P], open [2, P],
    valid [P], lane_mom [2 Tri, N], mom [2 Tri, P], lane_count [4, N])."""
    f = lambda a: None if a is None else np.asarray(a).astype(dtype)
    obs, obs0, action, grad, lsig_grad = (f(a) for a in (obs, obs0, action, grad, lsig_grad))
    K, N, D = obs.shape
    S, n = N // P, D + 1
    at, tri = moment_index(D)
    sig = np.broadcast_to(f(sigma).reshape(2, -1), (2, N))
    damp, bound = np.float64(damping).astype(dtype), np.float64(kl).astype(dtype)     # each rounded once
    ln = np.full(N, K, np.int64) if length is None else np.clip(np.asarray(length, np.int64), 0, K)
    zero = dtype(0)
    lane, nopen = np.zeros((2, tri, N), dtype), np.zeros((2, N), np.int32)
    with np.errstate(all="ignore"):
        wide = sig > 0                                                         # (a NaN is not)
        for k in range(K - 1, -1, -1):                                         # step 1
            counted = k < ln
            x = obs[k] if obs0 is None else (obs0 if k == 0 else obs[k - 1])
            opened = []
            for j in range(2):
                inside = np.ones(N, bool) if tanh else np.abs(action[k, :, j]) < 1      # (a NaN is not)
                opened.append(counted & wide[j] & inside)
                nopen[j] += opened[j]
            for i in range(D):
                for m in range(i, D):
                    prod = x[:, i] * x[:, m]                                   # formed once, added under both masks
                    for j in range(2):
                        lane[j, at[(i, m)]] = np.where(opened[j], lane[j, at[(i, m)]] + prod, lane[j, at[(i, m)]])
                for j in range(2):
                    lane[j, at[(i, D)]] = np.where(opened[j], lane[j, at[(i, D)]] + x[:, i], lane[j, at[(i, D)]])
        for j in range(2):
            lane[j, at[(D, D)]] = nopen[j].astype(dtype)
            s2 = sig[j] * sig[j]
            lane[j] = np.where(wide[j][None], lane[j] / s2[None], zero)
        lane = lane.reshape(2 * tri, N)
        fine = np.isfinite(lane).all(0)
        shaped = fine.reshape(S, P)
        mom = chunked_sum(lane.reshape(2 * tri, S, P), shaped)                # step 2
        count = np.stack([ln.astype(np.int32), nopen[0], nopen[1], fine.astype(np.int32)])
        steps, open0, open1, valid = (chunked_sum(row.reshape(S, P), shaped) for row in count)
        opens = np.stack([open0, open1])
        # step 3, every policy at once: a policy that has failed carries numbers nobody reads
        c = steps.astype(dtype)
        some = steps != 0
        d, failed = np.zeros((2, n, P), dtype), np.zeros((3, P), np.int32)
        dls = np.zeros((2, P), dtype)
        g = grad / c[None, None]
        for j in range(2):
            Fm = mom[j * tri:(j + 1) * tri] / c[None]
            A = lambda i, m: Fm[at[(i, m)]] + damp if i == m else Fm[at[(i, m)]]
            L = np.zeros((n, n, P), dtype)
            alive = some.copy()
            failed[j] = np.where(some, 0, 1)
            for m in range(n):
                t = A(m, m)
                if m > 0:
                    st = L[m, 0] * L[m, 0]
                    for q in range(1, m):
                        st = st + L[m, q] * L[m, q]
                    t = t - st
                bad = alive & ~(np.isfinite(t) & (t > 0))
                failed[j] = np.where(bad, m + 1, failed[j])
                alive = alive & ~bad
                L[m, m] = np.sqrt(t)
                for i in range(m + 1, n):
                    u = A(m, i)
                    if m > 0:
                        su = L[i, 0] * L[m, 0]
                        for q in range(1, m):
                            su = su + L[i, q] * L[m, q]
                        u = u - su
                    L[i, m] = u / L[m, m]
            z = np.zeros((n, P), dtype)
            for i in range(n):
                rhs = g[j, i]
                if i > 0:
                    s = L[i, 0] * z[0]
                    for q in range(1, i):
                        s = s + L[i, q] * z[q]
                    rhs = rhs - s
                z[i] = rhs / L[i, i]
            w = np.zeros((n, P), dtype)
            for i in range(n - 1, -1, -1):
                v = z[i]
                if i + 1 < n:
                    s = L[i + 1, i] * w[i + 1]
                    for q in range(i + 2, n):
                        s = s + L[q, i] * w[q]
                    v = v - s
                w[i] = v / L[i, i]
            d[j] = np.where(alive[None], w, zero)
            if lsig_grad is not None:
                nn = opens[j].astype(dtype)
                den = (nn + nn) / c + damp
                dls[j] = np.where(some & np.isfinite(den) & (den > 0), (lsig_grad[j] / c) / den, zero)
        q = g[0, 0] * d[0, 0]
        for j in range(2):
            for i in range(n):
                if (j, i) != (0, 0):
                    q = q + g[j, i] * d[j, i]
        if lsig_grad is not None:
            q = q + (lsig_grad[0] / c) * dls[0]
            q = q + (lsig_grad[1] / c) * dls[1]
        q = np.where(some, q, zero)
        good = np.isfinite(q) & (q > 0)
        failed[2] = np.where(good, 0, 1)
        scale = np.ones(P, dtype) if float(kl) == 0.0 else np.sqrt((bound + bound) / q)
        beta = np.where(good, scale, zero)
        step = beta[None, None] * d
        lsig_step = None if lsig_grad is None else beta[None] * dls
    assert all(a.dtype == dtype for a in (lane, mom, d, step, beta, q)) and all(a.dtype == np.int32 for a in (count, failed, steps, opens, valid))
    return dict(step=step, dir=d, lsig_step=lsig_step, beta=beta, quad=q, failed=failed, steps=steps, open=opens, valid=valid, lane_mom=lane,
                mom=mom, lane_count=count)


def crafted_npg(K, P, S, D, dtype, seed=0):
    """The inputs of the GPU tests, in `dtype`: obs, obs0, action, sigma, lane_sigma and length are crafted_pg's, with its lengths of
    0, K, -3 and K + 5 (l % 11 == 1, 2, 3, 4), its NaNs beyond len (l % 7 == 6), its actions of exactly +-1 (l % 5 == 0) and its
    per-lane sigma of 0 and NaN (l % 9 == 1, 3).  Beside them, by lane l = s P + p (where the shape reaches it):
      s % 8 == 5 (S >= 6)    a NaN in the first observation (in obs0 and in obs[0]), the length K, both components open at step 0:
                             the lane is invalid
      p == 2 (P > 2)         the same in every lane of the policy: none of its lanes is valid
      p == CLIPPED (P > 1)   component 1 of the action is 1 at every step of every lane: the component never opens
    -> dict(obs, obs0, action, sigma [2], lane_sigma [2, N], length, grad [2, D+1, P], lsig_grad [2, P])"""
    c = crafted_pg(K, P, S, D, dtype, seed)
    rng = np.random.default_rng(seed + 2000)
    N = S * P
    l = np.arange(N)
    s, p = l // P, l % P
    obs, obs0, action = (c[k].copy() for k in ("obs", "obs0", "action"))
    broken = ((s % 8 == 5) & (S >= 6)) | ((p == NONE_VALID) & (P > 2))
    obs0[broken, 0], obs[0, broken, 0] = np.nan, np.nan
    if P > 1:
        action[:, p == CLIPPED, 1] = 1.0
        action[0, broken & (p == CLIPPED), 0] = 0.5
    f = lambda a: np.ascontiguousarray(a.astype(dtype))
    return dict(obs=obs, obs0=obs0, action=action, sigma=c["sigma"], lane_sigma=c["lane_sigma"], length=c["length"],
                grad=f(rng.normal(0, 1, (2, D + 1, P))), lsig_grad=f(rng.normal(0, 1, (2, P))), broken=broken)


def npg_kwargs(c, P, dtype, *, obs0=True, per_lane=False, tanh=False, lsig=True, damping=DAMPING, kl=KL):
    """The arguments of restate_npg for one configuration of the crafted inputs `c` -> (positional, keywords)."""
    return ((c["obs"], c["lane_sigma"] if per_lane else c["sigma"], c["grad"]),
            dict(P=P, dtype=dtype, obs0=c["obs0"] if obs0 else None, action=None if tanh else c["action"], tanh=tanh, length=c["length"],
                 lsig_grad=c["lsig_grad"] if lsig else None, damping=damping, kl=kl))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_on_crafted_inputs_that_reach_every_branch(dtype):
    from gym_os2r_amd import npg, pg
    assert CHUNKS == npg.CHUNKS == pg.CHUNKS == int(re.search(r"#define OS2RN_CHUNKS (\d+)", _header("os2r_npg.h")).group(1))
    K, P, S, D = 7, 3, 130, 10
    n = D + 1
    at, tri = moment_index(D)
    c = crafted_npg(K, P, S, D, dtype)
    N, l = S * P, np.arange(S * P)
    s, p = l // P, l % P
    args, kw = npg_kwargs(c, P, dtype)
    out = restate_npg(*args, **kw)
    ln, n0, n1, fine = out["lane_count"]
    # the four lengths; a lane of length 0 has zeros for sums, opened nothing and is valid
    assert set(c["length"][[1, 2, 3, 4]]) == {0, K, -3, K + 5} and ln[1] == 0 == ln[3] and ln[2] == K == ln[4]
    assert (out["lane_mom"][:, 1] == 0).all() and fine[1] == 1 and n0[1] == 0 == n1[1]
    # a NaN observation inside the length: the lane is invalid and left out of every sum; NaNs beyond the length change nothing
    broken = c["broken"]
    assert np.array_equal(fine == 0, broken) and broken.sum() == S + (S // 8) * (P - 1) and np.isnan(out["lane_mom"][:, broken]).any(0).all()
    held = (l % 7 == 6) & (ln < K) & ~broken
    assert held.any() and np.isnan(c["obs"][-1, held]).all() and np.isfinite(out["lane_mom"][:, held]).all()
    for name, row in (("steps", ln), ("valid", fine)):
        assert np.array_equal(out[name], np.where(broken, 0, row).reshape(S, P).sum(0))
    assert np.array_equal(out["open"], np.stack([np.where(broken, 0, r).reshape(S, P).sum(0) for r in (n0, n1)]))
    assert np.isfinite(out["mom"]).all() and (out["mom"][:, NONE_VALID] == 0).all()
    # the policy with no valid lane: steps 0, both components fail, q = 0, beta = 0, the step is 0
    assert out["steps"][NONE_VALID] == 0 == out["valid"][NONE_VALID] and out["failed"][:, NONE_VALID].tolist() == [1, 1, 1]
    assert (out["step"][:, :, NONE_VALID] == 0).all() and (out["dir"][:, :, NONE_VALID] == 0).all() and out["beta"][NONE_VALID] == 0
    assert out["quad"][NONE_VALID] == 0 and (out["lsig_step"][:, NONE_VALID] == 0).all()
    # actions of exactly +-1 close the component on that step, the nearest values below do not
    five = np.flatnonzero((l % 5 == 0) & ~broken & (ln == K) & (p == 0))[0]
    assert n0[five] == n1[five] == len([k for k in range(K) if k % 4 >= 2])
    # the component clipped on every step: never open, all sums 0; with damping > 0 d is g / damping (up to the two roundings of
    # the factor's square root), and the width's denominator is the damping alone
    assert (n1[p == CLIPPED] == 0).all() and (out["lane_mom"][tri:, p == CLIPPED] == 0).all() and out["open"][1, CLIPPED] == 0
    assert out["failed"][:, CLIPPED].tolist() == [0, 0, 0] and out["open"][0, CLIPPED] > 0
    g1 = c["grad"][1, :, CLIPPED] / dtype(out["steps"][CLIPPED])
    eps = np.finfo(dtype).eps
    assert np.allclose(out["dir"][1, :, CLIPPED], g1 / dtype(DAMPING), rtol=4 * eps, atol=0)
    assert np.allclose(out["lsig_step"][1, CLIPPED] / out["beta"][CLIPPED],
                       (c["lsig_grad"][1, CLIPPED] / dtype(out["steps"][CLIPPED])) / dtype(DAMPING), rtol=4 * eps, atol=0)
    # ... with damping = 0 its factor fails at column 0, d_1 = 0, the width's step is 0, and the other component still steps
    a0, k0 = npg_kwargs(c, P, dtype, damping=0.0)
    bare = restate_npg(*a0, **k0)
    assert bare["failed"][:, CLIPPED].tolist() == [0, 1, 0] and (bare["dir"][1, :, CLIPPED] == 0).all() and bare["lsig_step"][1, CLIPPED] == 0
    assert (bare["dir"][0, :, CLIPPED] != 0).all() and bare["beta"][CLIPPED] > 0 and bare["failed"][:, 0].tolist() == [0, 0, 0]
    # the healthy policy: beta = sqrt(2 kl / q), the step is beta d, q is the chain's value
    q = out["quad"][0]
    assert q > 0 and out["beta"][0] == np.sqrt((dtype(KL) + dtype(KL)) / q) and np.array_equal(out["step"][:, :, 0], out["beta"][0] * out["dir"][:, :, 0])
    with np.errstate(all="ignore"):
        g = c["grad"] / out["steps"].astype(dtype)[None, None]
    want = float((g[:, :, 0].astype(np.float64) * out["dir"][:, :, 0]).sum()
                 + ((c["lsig_grad"][:, 0] / dtype(out["steps"][0])).astype(np.float64) * (out["lsig_step"][:, 0] / out["beta"][0])).sum())
    mag = float(np.abs(g[:, :, 0].astype(np.float64) * out["dir"][:, :, 0]).sum()) + abs(want)
    assert abs(q - want) <= 32 * eps * mag                                   # (a chain of 2 n + 2 rounded products)
    # kl = 0: beta = 1 and the step is the direction; a kl so small that it rounds to 0 in float32 is not that case
    a1, k1 = npg_kwargs(c, P, dtype, kl=0.0)
    unit = restate_npg(*a1, **k1)
    assert unit["beta"].tolist() == [1, 1, 0] and np.array_equal(unit["step"], unit["dir"]) and np.array_equal(unit["dir"], out["dir"])
    tiny = restate_npg(*a1, **dict(k1, kl=1e-60))
    assert (tiny["beta"][:2] == 0).all() if dtype is np.float32 else (tiny["beta"][:2] > 0).all()
    assert tiny["failed"][2].tolist() == [0, 0, 1]
    # without lsig_grad: no step of the widths, q loses their two products, the direction is the same
    a2, k2 = npg_kwargs(c, P, dtype, lsig=False)
    mean = restate_npg(*a2, **k2)
    assert mean["lsig_step"] is None and np.array_equal(mean["dir"], out["dir"]) and (mean["quad"][:2] < out["quad"][:2]).all()
    # tanh: no clip counts, the actions are not read: every step of a lane with sigma > 0 is open
    a3, k3 = npg_kwargs(c, P, dtype, tanh=True)
    th = restate_npg(*a3, **k3)
    assert np.array_equal(th["lane_count"][1], ln) and np.array_equal(th["lane_count"][2], ln) and th["open"][1, CLIPPED] > 0
    # obs0 null: obs[k] itself is what step k saw
    shifted = dict(c, obs=np.concatenate([c["obs0"][None], c["obs"][:-1]]))
    a4, k4 = npg_kwargs(shifted, P, dtype, obs0=False)
    moved = restate_npg(*a4, **k4)
    for name in ("lane_mom", "mom", "step", "quad", "lane_count"):
        assert np.array_equal(moved[name], out[name], equal_nan=True), name
    # a per-lane sigma of 0 and NaN: the component's sums and its count are 0, the other component's are not; the lane is valid
    a5, k5 = npg_kwargs(c, P, dtype, per_lane=True)
    lane = restate_npg(*a5, **k5)
    fine_l, ln_l = lane["lane_count"][3], lane["lane_count"][0]
    z0, nan = (np.flatnonzero((l % 9 == m) & (l % 5 != 0) & (fine_l == 1) & (ln_l > 1))[0] for m in (1, 3))
    assert c["lane_sigma"][0, z0] == 0 and np.isnan(c["lane_sigma"][1, nan])
    assert (lane["lane_mom"][:tri, z0] == 0).all() and lane["lane_count"][1, z0] == 0 and p[z0] == CLIPPED      # (l % 9 == 1 is policy 1 here)
    open_l = restate_npg(*a5, **dict(k5, tanh=True, action=None))
    assert (open_l["lane_mom"][:tri, z0] == 0).all() and (open_l["lane_mom"][tri:, z0] != 0).all() and open_l["lane_count"][3, z0] == 1
    assert (lane["lane_mom"][tri:, nan] == 0).all() and lane["lane_count"][2, nan] == 0 and (lane["lane_mom"][:tri, nan] != 0).all()
    # ... and the quotient is by the lane's own sigma: the corner is n_j / sigma_j^2
    free = np.flatnonzero((fine_l == 1) & (ln_l > 1) & (l % 9 != 1))[0]
    s2 = c["lane_sigma"][0, free] * c["lane_sigma"][0, free]
    assert lane["lane_mom"][at[(D, D)], free] == dtype(lane["lane_count"][1, free]) / s2 and s2.dtype == dtype
    # S = 130: partials of up to three terms; fewer than 64 samples: empty partials; every shape of the GPU tests runs
    assert S == 2 * CHUNKS + 2
    for shape in SHAPES:
        cs = crafted_npg(*shape, dtype)
        for config in (dict(), dict(per_lane=True, lsig=False), dict(tanh=True, obs0=False)):
            a, k = npg_kwargs(cs, shape[1], dtype, **config)
            o = restate_npg(*a, **k)
            assert np.isfinite(o["step"]).all() and np.isfinite(o["mom"]).all() and o["step"].shape == (2, shape[3] + 1, shape[1])
            assert np.array_equal(o["lane_count"][3] == 0, cs["broken"]) and (o["failed"][2] == (o["beta"] == 0)).all()
    few = crafted_npg(4, 2, 5, 3, dtype)
    a, k = npg_kwargs(few, 2, dtype)
    o = restate_npg(*a, **k)
    assert o["valid"].tolist() == [5, 5] and o["failed"][:, 0].tolist() == [0, 0, 0] and n == 11


def plain_npg(dtype, seed=0, K=12, P=4, S=24, D=10, clipped=False):
    """A batch on which every Fisher matrix is well conditioned, rounded to `dtype` and returned in float64: observations ~ N(0, 1),
    K S >= 8 (D + 1) steps per policy, mixed lengths, no lane invalid; without `clipped` no action at the bound."""
    rng = np.random.default_rng(seed)
    N = S * P
    r = lambda a: a.astype(dtype).astype(np.float64)
    A = rng.normal(0.0, 0.7, (K, N, 2))
    A = np.clip(A, -1.0, 1.0) if clipped else np.clip(A, -0.99, 0.99)
    return dict(obs0=r(rng.normal(0, 1, (N, D))), obs=r(rng.normal(0, 1, (K, N, D))), action=r(A), sigma=r(np.array([0.2, 0.3])),
                length=rng.integers(K // 2, K + 1, N).astype(np.int32), grad=r(rng.normal(0, 1, (2, D + 1, P))),
                lsig_grad=r(rng.normal(0, 1, (2, P))), K=K, P=P, S=S, D=D, N=N)


def _far(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def _features(c):
    """phi [K, S, P, D+1], the open masks [K, S, P, 2] (as float64) and the counted steps [K, S, P] of a plain batch."""
    K, P, S, D, N = (c[k] for k in ("K", "P", "S", "D", "N"))
    x = np.concatenate([c["obs0"][None], c["obs"][:-1]])
    phi = np.concatenate([x, np.ones((K, N, 1))], 2).reshape(K, S, P, D + 1)
    counted = (np.arange(K)[:, None] < c["length"][None]).reshape(K, S, P)
    opened = ((np.abs(c["action"]) < 1.0) & counted.reshape(K, N)[..., None]).reshape(K, S, P, 2).astype(np.float64)
    return phi, opened, counted


def textbook_npg(c, damping, kl):
    """The reference in float64: the masked einsum for the two moment matrices, np.linalg.solve on A = F / steps + damping I, the
    widths' scalar entries, and the trust-region scaling.  -> (step, dir) [2, D+1, P]"""
    P, D = c["P"], c["D"]
    phi, opened, counted = _features(c)
    steps = counted.sum((0, 1)).astype(np.float64)                               # [P]
    F = np.einsum("kspj,kspa,kspb->jpab", opened, phi, phi) / (c["sigma"] ** 2)[:, None, None, None] / steps[None, :, None, None]
    g = c["grad"] / steps[None, None]
    d = np.zeros((2, D + 1, P))
    for j in range(2):
        for p in range(P):
            d[j, :, p] = np.linalg.solve(F[j, p] + damping * np.eye(D + 1), g[j, :, p])
    g_ls = c["lsig_grad"] / steps[None]
    d_ls = g_ls / (2.0 * opened.sum((0, 1)).T / steps[None] + damping)
    q = (g * d).sum((0, 1)) + (g_ls * d_ls).sum(0)
    beta = np.sqrt(2.0 * kl / q)
    return beta[None, None] * d, d


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_is_the_solve_of_the_textbook(dtype):
    """step and dir in float64 within MARGIN x the distance measured from np.linalg.solve on the same A (8.6e-16 and 8.4e-16,
    relative to the largest entry), and in float32 within MARGIN x the distance measured from the float64 restatement on the
    same (float32-rounded) inputs (1.9e-7 and 1.9e-7): the order of the value fit's ridge solve."""
    worst = dict(step=0.0, dir=0.0)
    for seed, clipped in ((0, False), (1, True)):
        c = plain_npg(dtype, seed, clipped=clipped)
        kw = dict(P=c["P"], obs0=c["obs0"], action=c["action"], length=c["length"], lsig_grad=c["lsig_grad"], damping=DAMPING, kl=KL)
        got = restate_npg(c["obs"], c["sigma"], c["grad"], dtype=dtype, **kw)
        assert got["valid"].tolist() == [c["S"]] * c["P"] and (got["failed"] == 0).all()
        if dtype is np.float64:
            step, d = textbook_npg(c, DAMPING, KL)
        else:
            wide = restate_npg(c["obs"], c["sigma"], c["grad"], dtype=np.float64, **kw)
            step, d = wide["step"], wide["dir"]
        worst["step"], worst["dir"] = max(worst["step"], _far(got["step"], step)), max(worst["dir"], _far(got["dir"], d))
    print(f"restate_npg against the reference, {dtype.__name__}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for name, value in worst.items():
        assert value <= MARGIN * MEASURED[dtype][name], (name, value)


def test_the_step_has_the_divergence_asked_for():
    """The trust-region property in float64 with damping = 0, the widths unchanged and no clipped step: the mean over the
    counted steps of 1/2 sum_j (step_j . phi)^2 / sigma_j^2, formed directly from the observations, is kl within MARGIN x the
    8.9e-16 (relative) measured."""
    worst = 0.0
    for seed, kl in ((0, 0.01), (1, 0.5), (2, 1e-4)):
        c = plain_npg(np.float64, seed)
        got = restate_npg(c["obs"], c["sigma"], c["grad"], P=c["P"], dtype=np.float64, obs0=c["obs0"], action=c["action"], length=c["length"],
                          damping=0.0, kl=kl)
        assert (got["failed"] == 0).all() and np.array_equal(got["open"][0], got["steps"]) and np.array_equal(got["open"][1], got["steps"])
        phi, opened, counted = _features(c)
        shift = np.einsum("kspa,jap->kspj", phi, got["step"])                    # step_j . phi of every step
        div = 0.5 * (opened * shift * shift / (c["sigma"] ** 2)).sum(3)
        mean = (div * counted).sum((0, 1)) / counted.sum((0, 1))
        worst = max(worst, float(np.abs(mean / kl - 1).max()))
    print(f"the mean divergence of the step against kl, float64: {worst:.3e}")
    assert worst <= MARGIN * MEASURED[np.float64]["kl"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_moments_of_one_open_mask_are_the_value_fits(dtype):
    """With one open mask (tanh: every counted step is open) and sigma = 1, F of component 0 -- per lane and summed -- is M of the
    value fit's restatement on the same arrays bit for bit, and so is component 1's; lane_count agrees in len and valid."""
    for K, P, S, D in [(7, 3, 65, 10), (4, 1, 130, 7), (3, 2, 5, 12)]:
        c = crafted_npg(K, P, S, D, dtype)
        at, tri = moment_index(D)
        fit = restate_fit(c["obs"], c["obs0"], np.zeros((K, S * P)), P=P, dtype=dtype, length=c["length"])
        got = restate_npg(c["obs"], np.ones(2), c["grad"], P=P, dtype=dtype, obs0=c["obs0"], tanh=True, length=c["length"])
        for j in range(2):
            assert np.array_equal(got["lane_mom"][j * tri:(j + 1) * tri], fit["lane_mom"][:tri], equal_nan=True), (K, P, S, D, j)
            assert np.array_equal(got["mom"][j * tri:(j + 1) * tri], fit["mom"][:tri]), (K, P, S, D, j)
        assert np.array_equal(got["lane_count"][[0, 3]], fit["lane_count"]) and np.array_equal(got["steps"], fit["steps"])
        assert np.array_equal(got["valid"], fit["valid"]) and np.array_equal(got["lane_count"][1], got["lane_count"][0])


# ---------------------------------------------------------------------------------------
# header, table, exports, resources
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import _lib, control, critic, npg, pg
    protos = _prototypes("os2r_npg.h", "os2rn")
    assert [p[0] for p in protos] == list(npg.ENTRY_POINTS) == NAMES
    lib = npg.load()
    for name, ret, args in protos:
        argtypes = npg.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2rn_last_error" else C.c_int)
    args = protos[2][2]
    assert args[:5] == ["const Os2rControlLayout* layout", "int32_t nsteps", "int64_t npolicies", "int32_t nsamples", "uint32_t flags"]
    assert len(args) == 27 and args[12] == "double damping" and args[13] == "double kl"
    assert npg.ENTRY_POINTS["os2rn_natural_step"][12] is C.c_double and npg.ENTRY_POINTS["os2rn_natural_step"][13] is C.c_double
    assert args[-1] == "void* stream" and args[-2] == "int32_t* lane_count_dev" and npg.ENTRY_POINTS["os2rn_natural_step"][2] is C.c_int64
    header = _header("os2r_npg.h")
    assert re.search(r"#define OS2R_NPG_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert len(re.findall(r"#include", header)) == 1
    assert lib.os2rn_abi_version() == npg.ABI_VERSION == 1
    # the flags are the score-function library's, redeclared under this prefix with the same values
    assert npg.TANH == int(re.search(r"#define OS2RN_TANH (\d)u", header).group(1)) == pg.TANH == 1
    assert npg.SIGMA_PER_LANE == int(re.search(r"#define OS2RN_SIGMA_PER_LANE (\d)u", header).group(1)) == pg.SIGMA_PER_LANE == 2
    assert npg.CHUNKS == int(re.search(r"#define OS2RN_CHUNKS (\d+)", header).group(1)) == pg.CHUNKS == 64
    assert npg.LANE_COUNTS == int(re.search(r"#define OS2RN_LANE_COUNTS (\d+)", header).group(1)) == 4
    assert [npg.moments(d) for d in (1, 7, 10, 12)] == [6, 72, 132, 182] and npg.moments(10) - 2 * 11 == 2 * (critic.moments(10) - 2 * 11)
    assert npg.Os2rControlLayout is control.Os2rControlLayout and npg.layout is control.layout
    assert not set(npg.ENTRY_POINTS) & (set(_lib.ENTRY_POINTS) | set(_lib.RECORD_ENTRY_POINTS)) and len(_lib.ENTRY_POINTS) == 35
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", npg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "libos2r_npg.map")) as f:
        assert re.search(r"global:\s*os2rn_\*;\s*local:\s*\*;", f.read())
    # the header names no other companion library (their tests forbid it) and no other header declares anything of this one; the
    # sums over the samples are said in words, and are the included bodies
    for word in FORBIDDEN:
        assert word not in header.lower(), word
    assert "adjacent-pair tree" in header and "in ascending order onto 0" in header
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "os2r_npg.h":
            assert "os2rn_" not in _header(name).lower() and "os2r_npg.h" not in _header(name).lower(), name
    src = _csrc("os2r_npg.hpp")
    assert '#include "os2r_critic.hpp"' in src and "pg_wave_sum<T>" in src and "pg_few_sum<T>" in src and "cr_positive(" in src
    # the out-of-scope lines of the two gradient headers say where the natural gradient went
    for name in ("os2r_pg.h", "os2r_ppo.h"):
        assert "natural-gradient and Fisher terms (since built as `libos2r_npg.so`)" in " ".join(_header(name).replace(" * ", " ").split()), name


KERNELS = ("npg_moment_kernel", "npg_sum_kernel", "npg_sum_few_kernel", "npg_solve_kernel")


def test_kernel_resources():
    """Exactly eight kernels, the four of os2r_npg.hpp in float and double, are in the built library and none uses scratch:
    private_segment_fixed_size 0, no VGPR or SGPR spill and no AGPRs in the code-object metadata; only the solve uses LDS (the
    factor, d and d_ls of every thread of its wave, 105 entries x 64 threads) -- the moment kernel none, like its sibling.  The
    moment kernel holds two masked sets of 15 chains and two steps of loads: 126 VGPRs in float and 194 in double when this was
    written (the value fit's, one set of 17 chains, stands at 117 and 158) -- four waves a SIMD in float, two in double, which
    is what the bound below keeps."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import npg
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(npg.LIB_PATH)
    meta = kernel_meta.kernel_meta(npg.LIB_PATH)
    assert len(meta) == 8, sorted(meta)
    for kernel in KERNELS:
        for real, size in (("float", 4), ("double", 8)):
            (name,) = [k for k in meta if f"{kernel}<{real}>" in k]
            m = meta[name]
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
            assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 256, (name, m)
            assert m["group_segment_fixed_size"] == (105 * 64 * size if kernel == "npg_solve_kernel" else 0), (name, m)
            if kernel == "npg_moment_kernel":
                print(f"{kernel}<{real}>: {m['vgpr_count']} VGPRs")
                assert m["vgpr_count"] <= (256 if real == "double" else 128), (name, m)


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def test_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import control, npg
    lib = npg.load()
    K, P, S, D = 3, 2, 2, 4
    N = S * P
    E = npg.moments(D)
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) & ~15                  # a pair of doubles is 16 bytes
    at = lambda i: C.c_void_p(base + 8 * i)
    nan, inf = float("nan"), float("inf")

    def Lay(dtype=abi.F64, **kw):
        lay = control.layout(dtype, 3, 0, [0, 1, 3, -1])
        for k, v in kw.items():
            setattr(lay, k, v)
        return C.byref(lay)
    # the inputs from element 0, the outputs from element 4096; sizes in elements of 8 bytes
    size = dict(obs=K * N * D, obs0=N * D, act=K * N * 2, sigma=2, length=N, grad=2 * (D + 1) * P, lsig=2 * P, step=2 * (D + 1) * P,
                dir=2 * (D + 1) * P, lsig_step=2 * P, beta=P, quad=P, failed=3 * P, steps=P, open=2 * P, valid=P, lane_mom=E * N, mom=E * P,
                count=4 * N)
    where, nxt = {}, 0
    for name, n in size.items():
        if name == "step":
            assert nxt < 4096
            nxt = 4096
        where[name] = nxt
        nxt += (n + 1) & ~1                               # every array starts at a pair
    assert nxt < 8000
    good = dict(lay=Lay(), K=K, P=P, S=S, flags=0, obs=at(where["obs"]), obs0=at(where["obs0"]), act=at(where["act"]), sigma=at(where["sigma"]),
                length=at(where["length"]), grad=at(where["grad"]), lsig=at(where["lsig"]), damping=1e-3, kl=0.01, step=at(where["step"]),
                dir=at(where["dir"]), lsig_step=at(where["lsig_step"]), beta=at(where["beta"]), quad=at(where["quad"]),
                failed=at(where["failed"]), steps=at(where["steps"]), open=at(where["open"]), valid=at(where["valid"]),
                lane_mom=at(where["lane_mom"]), mom=at(where["mom"]), count=at(where["count"]))
    name = "os2rn_natural_step"
    assert len(good) + 1 == len(npg.ENTRY_POINTS[name])

    def call(**kw):
        a = dict(good, **kw)
        return lib.os2rn_natural_step(*[a[k] for k in good], None)
    assert lib.os2rn_natural_step(*[None if _is_pointer(t) else 0 for t in npg.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rn_last_error() == b"os2rn_natural_step: null layout"
    end = lambda n: where[n] + size[n] - 1
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(nq=1)), b"nq must be 2..5"),
             (dict(lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"), (dict(lay=Lay(obs_dim=13)), b"obs_dim must be 1..12"),
             (dict(K=0), b"nsteps must be >= 1"), (dict(K=-2), b"nsteps must be >= 1"), (dict(K=65536), b"nsteps must be <= 65535"),
             (dict(P=0), b"npolicies must be >= 1"), (dict(P=-1), b"npolicies must be >= 1"), (dict(S=0), b"nsamples must be >= 1"),
             (dict(S=-4), b"nsamples must be >= 1"), (dict(P=2 ** 62), b"nsamples * npolicies exceeds 2^31 - 1"),
             (dict(P=2 ** 30, S=2), b"nsamples * npolicies exceeds 2^31 - 1"), (dict(P=1, S=2 ** 30, K=2), b"nsamples * nsteps exceeds 2^31 - 1"),
             (dict(flags=4), b"unknown flag bits"), (dict(flags=0x80000001), b"unknown flag bits"),
             (dict(damping=nan), b"damping must be finite"), (dict(damping=inf), b"damping must be finite"),
             (dict(damping=-inf), b"damping must be finite"), (dict(damping=-1e-3), b"damping must be >= 0"),
             (dict(kl=nan), b"kl must be finite"), (dict(kl=inf), b"kl must be finite"), (dict(kl=-0.01), b"kl must be >= 0"),
             (dict(kl=-5e-324), b"kl must be >= 0"),
             (dict(obs=None), b"null obs_dev"), (dict(sigma=None), b"null sigma_dev"), (dict(grad=None), b"null grad_dev"),
             (dict(step=None), b"null step_dev"), (dict(lane_mom=None), b"null lane_mom_dev"), (dict(mom=None), b"null mom_dev"),
             (dict(count=None), b"null lane_count_dev"), (dict(act=None), b"null action_dev without OS2RN_TANH"),
             (dict(lsig=None), b"lsig_step_dev needs lsig_grad_dev"), (dict(lsig_step=None), b"lsig_grad_dev needs lsig_step_dev"),
             (dict(act=at(where["act"] + 1)), b"action_dev must be aligned to a pair"),
             (dict(lay=Lay(abi.F32), act=C.c_void_p(base + 8 * where["act"] + 4)), b"action_dev must be aligned to a pair"),
             # an output over an input, from both sides; over another output; the optional ones too
             (dict(step=at(end("obs"))), b"step_dev overlaps obs_dev"),
             (dict(step=at(where["obs0"] - size["step"] + 1)), b"step_dev overlaps obs_dev"),
             (dict(dir=at(where["obs0"])), b"dir_dev overlaps obs0_dev"), (dict(lsig_step=at(where["act"])), b"lsig_step_dev overlaps action_dev"),
             (dict(beta=at(where["sigma"] + 1)), b"beta_dev overlaps sigma_dev"), (dict(quad=at(where["length"])), b"quad_dev overlaps length_dev"),
             (dict(step=at(where["grad"])), b"step_dev overlaps grad_dev"), (dict(failed=at(end("grad"))), b"failed_dev overlaps grad_dev"),
             (dict(lsig_step=at(where["lsig"])), b"lsig_step_dev overlaps lsig_grad_dev"), (dict(steps=at(end("lsig"))), b"steps_dev overlaps lsig_grad_dev"),
             (dict(open=at(where["obs"])), b"open_dev overlaps obs_dev"), (dict(valid=at(where["act"])), b"valid_dev overlaps action_dev"),
             (dict(lane_mom=at(where["grad"])), b"lane_mom_dev overlaps grad_dev"), (dict(mom=at(where["sigma"])), b"mom_dev overlaps sigma_dev"),
             (dict(count=at(where["length"])), b"lane_count_dev overlaps length_dev"),
             (dict(dir=at(end("step"))), b"dir_dev overlaps step_dev"), (dict(lsig_step=at(where["dir"])), b"lsig_step_dev overlaps dir_dev"),
             (dict(beta=at(where["lsig_step"] + 1)), b"beta_dev overlaps lsig_step_dev"), (dict(quad=at(where["beta"])), b"quad_dev overlaps beta_dev"),
             (dict(failed=at(where["quad"])), b"failed_dev overlaps quad_dev"), (dict(steps=at(where["failed"] + 1)), b"steps_dev overlaps failed_dev"),
             (dict(open=at(where["steps"])), b"open_dev overlaps steps_dev"), (dict(valid=at(where["open"] + 1)), b"valid_dev overlaps open_dev"),
             (dict(lane_mom=at(where["valid"])), b"lane_mom_dev overlaps valid_dev"), (dict(mom=at(end("lane_mom"))), b"mom_dev overlaps lane_mom_dev"),
             (dict(count=at(end("mom"))), b"lane_count_dev overlaps mom_dev")]
    seen = set()
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.os2rn_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(b"os2rn_natural_step: "), (kw.keys(), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases}) == 51              # each cause has a text of its own
    assert not any(buf)                                                   # a refused call wrote nothing
    # the edges are taken: nothing is left to refuse but the device, and no call is let through to one
    edges = [dict(K=65535, S=1, P=1, obs=at(10 ** 6), act=at(3 * 10 ** 6)), dict(damping=0.0, kl=0.0), dict(damping=-0.0, kl=5e-324),
             dict(flags=3, act=None, sigma=at(where["obs"])), dict(flags=1, act=at(where["act"] + 1)), dict(lsig=None, lsig_step=None),
             dict(dir=None, beta=None, quad=None, failed=None, steps=None, open=None, valid=None), dict(obs0=None, length=None),
             dict(dir=at(where["step"] + size["step"])), dict(flags=1, act=at(where["act"]), step=at(where["act"]))]
    for kw in edges:                                  # (device 1000 is never there, with a GPU or without)
        kw = dict(kw, lay=Lay(device=1000))
        assert call(**kw) == abi.ERR_NO_DEVICE and lib.os2rn_last_error().startswith(b"os2rn_natural_step: "), kw
    assert not any(buf)
    # the source: no HIP call and every refusal of an argument before check_device
    body = _function(_csrc("os2r_npg_capi.hip"), "int " + name)
    first_hip = body.index("check_device(")
    assert not re.search(HIP_CALL, body[:first_hip]) and body.index("DeviceGuard") > first_hip and body.index("auto launch") > first_hip
    fails = [m.start() for m in re.finditer(r"fail\(OS2R_ERR_INVALID", body)]
    assert len(fails) == 25 and all(i < first_hip for i in fails)
    texts = re.findall(r'fail\(OS2R_ERR_INVALID, "([^"]+)"', body)
    assert len(texts) == len(set(texts)) == 23 and all(any(t.encode() in e for e in seen) for t in texts)


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
    from gym_os2r_amd import npg
    from gym_os2r_amd.sim import HipSim
    assert callable(HipSim.natural_step) and callable(HipSim.natural_step_into)
    assert "1/2 Delta' F Delta" in HipSim.natural_step.__doc__ and "nats" in HipSim.natural_step.__doc__

    def no_load():
        raise AssertionError("a refused call reached npg.load")
    monkeypatch.setattr(npg, "load", no_load)
    f64, i32 = torch.float64, torch.int32
    s = _bare(f64)
    K, P, S, D = 3, 2, 2, 4
    N = S * P
    E = npg.moments(D)
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    obs, act, sig, grad = z(K, N, D), z(K, N, 2), z(2), z(2, D + 1, P)
    step, lane_mom, mom, count = z(2, D + 1, P), z(E, N), z(E, P), z(4, N, dtype=i32)
    ok = dict(policies=P, actions=act)

    def into(*args, **kw):
        with pytest.raises(ValueError, match="^natural_step: "):
            s.natural_step_into(*args, **dict(ok, **kw))

    def whole(*args, **kw):
        with pytest.raises(ValueError, match="^natural_step: "):
            s.natural_step(*args, **dict(ok, **kw))
    full = (obs, sig, grad, step, lane_mom, mom, count)
    gv = z(P, 2, D + 1)
    surface = (obs, sig, gv)
    for bad in (0, -1, 3, 2.0, True, None, "2"):
        into(*full, policies=bad)
        whole(*surface, policies=bad)
    for bad in (float("nan"), float("inf"), -0.1, "x", None, True):
        into(*full, damping=bad)
        into(*full, kl=bad)
        whole(*surface, damping=bad)
        whole(*surface, kl=bad)
    into(*full, actions=None)
    whole(*surface, actions=None)
    into(*full, lsig_grad=z(2, P))
    into(*full, lsig_step=z(2, P))
    for i in range(len(full)):
        into(*[None if j == i else t for j, t in enumerate(full)])
    swap = lambda i, t: tuple(t if j == i else a for j, a in enumerate(full))
    for args in (swap(0, z(K, N)), swap(0, z(0, N, D)), swap(0, obs.numpy()), swap(0, z(K, N + 1, D)), swap(0, z(K, N, D + 1)), swap(0, obs.float()),
                 swap(0, z(N, K, D).permute(1, 0, 2)), swap(1, z(3)), swap(1, z(N, 2)), swap(1, z(2, N + 1)), swap(2, z(P, 2, D + 1)),
                 swap(2, grad.float()), swap(2, z(2, D, P)), swap(3, z(P, 2, D + 1)), swap(3, grad), swap(4, z(E + 1, N)), swap(4, z(N, E)),
                 swap(5, z(E, P + 1)), swap(5, mom.float()), swap(6, z(4, N)), swap(6, z(5, N, dtype=i32)),
                 swap(3, obs.reshape(-1)[:2 * (D + 1) * P].reshape(2, D + 1, P)), swap(4, z(0))):
        into(*args)
    misaligned = z(K * N * 2 + 1)[1:].reshape(K, N, 2)
    into(*full, actions=misaligned)
    pool = z(8192)
    into(obs, sig, grad, pool[:2 * (D + 1) * P].reshape(2, D + 1, P), pool[5:5 + E * N].reshape(E, N), mom, count)
    for kw in (dict(obs0=z(N, D + 1)), dict(obs0=z(N, D).float()), dict(length=z(N)), dict(length=z(N + 1, dtype=i32)), dict(steps=z(P)),
               dict(steps=z(P + 1, dtype=i32)), dict(open=z(P, 3, dtype=i32)), dict(valid=z(P, dtype=torch.int64)), dict(failed=z(3, P)),
               dict(failed=z(2, P, dtype=i32)), dict(beta=z(P + 1)), dict(quad=z(P).float()), dict(dir=z(P, 2, D + 1)), dict(dir=step),
               dict(lsig_grad=z(P, 3), lsig_step=z(2, P)), dict(lsig_grad=z(2, P), lsig_step=z(P, 3)), dict(actions=z(K, N, 3)),
               dict(steps=count[0, :P]), dict(beta=mom[0])):
        into(*full, **kw)
    for args in ((None, sig, gv), (obs, None, gv), (obs, True, gv), (obs, z(N + 1, 2), gv), (obs, "wide", gv), (z(K, N + 1, D), sig, gv),
                 (obs, z(2).float(), gv), (obs, sig, None), (obs, sig, z(2, D + 1, P + 1)), (obs, sig, z(P, 2, D))):
        whole(*args)
    for kw in (dict(obs0=z(N)), dict(length=z(N)), dict(lsig_grad=z(P, 3)), dict(lsig_grad=z(P + 1, 2))):
        whole(*surface, **kw)
    # what passes every check reaches the loader, and only then
    with pytest.raises(AttributeError):                                    # (the bare handle has no cfg to fill a layout from)
        s.natural_step_into(*full, **ok)
    with pytest.raises(AttributeError):
        s.natural_step_into(*full, lsig_grad=z(2, P), lsig_step=z(2, P), dir=z(2, D + 1, P), tanh=True, policies=P)
