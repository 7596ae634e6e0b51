"""libos2r_critic.so (include/os2r_critic.h): the host side -- the numpy restatements of both calls the GPU tests compare with
(`restate_gae`, `restate_fit`) against textbook statements in float64 (the sum of discounted deltas within an episode, the plain
discounted reward-to-go, np.linalg.lstsq on the stacked ridge-augmented system), their edge semantics, the crafted inputs of the
GPU tests (`crafted_critic`), the header against the one table of gym_os2r_amd/critic.py, the exports of the library, the
resources of its kernels in the built library, every refusal of both entry points through ctypes without a device, and the
argument checks of HipSim.gae and HipSim.value_fit that need no device.  No GPU needed."""
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
from test_pg_host import chunked_sum  # noqa: E402  (step 5 of os2r_pg.h, which step 3 of os2rv_value_fit is word for word)

NAMES = ["os2rv_abi_version", "os2rv_last_error", "os2rv_gae", "os2rv_value_fit"]
CHUNKS = 64
# K, P, S, D of the GPU tests (tests/test_gpu_critic.py).  K: below, at and past a round of four loads; S: the two sum kernels
# and their boundary, partials of up to three terms; P = 3 divides nothing; N no multiple of a wave; D = 12 and 7 beside the 10
# of the robot
SHAPES = [(1, 1, 1, 7), (3, 3, 63, 12), (4, 1, 64, 10), (9, 3, 65, 10), (4, 3, 130, 7), (9, 1, 130, 12), (3, 1, 65, 10)]
NONE_VALID = 2                          # the policy none of whose lanes is valid (where P > 2)
# The largest relative distance (the largest difference over the largest entry of the textbook result) of the restatements from
# the textbook statements in float64 on the data of `plain_critic` (observations uniform in [-1, 1], D = 10, 4 policies x 96
# samples x 12 steps, mixed lengths), measured on the CPU this test was written on (the tests print them): the bound is
# MARGIN x that, the margin of tests/test_pg_host.py.
# adv: of adv and ret against the sum of deltas; ret: of ret at lambda = 1 under a zero critic against the reward-to-go (in float64
# both sides run the same operations: the distance is 0 and the bound is equality); fit0, fit1: of w against lstsq at ridge 0, 1e-3.
MEASURED = {np.float64: dict(adv=4.734e-16, ret=0.0, fit0=1.078e-15, fit1=5.987e-16),
            np.float32: dict(adv=3.221e-7, ret=1.574e-7, fit0=8.756e-8, fit1=1.212e-7)}
MARGIN = 100
RIDGES = (0.0, 1e-3)


# ---------------------------------------------------------------------------------------
# the restatements of include/os2r_critic.h (need no device)
# ---------------------------------------------------------------------------------------
def _val(x, wl):
    """val(x; w) = (((w_D + w_0 x_0) + w_1 x_1) + ...) of x [N, D] under the lanes' weights wl [D+1, N]."""
    D = x.shape[1]
    acc = wl[D].copy()
    for d in range(D):
        acc = acc + wl[d] * x[:, d]
    return acc


def _lengths(length, K, N):
    return np.full(N, K, np.int64) if length is None else np.clip(np.asarray(length, np.int64), 0, K)


def restate_gae(obs, obs0, reward, done, value_w, *, P, dtype, term_obs=None, length=None, gamma=0.99, lam=0.95):
    """os2rv_gae in numpy and in `dtype`.  obs [K, N, D], obs0 [N, D], reward and done [K, N], value_w [D+1, P].
    -> dict(adv, ret, value), each [K, N]."""
    f = lambda a: None if a is None else np.asarray(a).astype(dtype)
    obs, obs0, reward, value_w, term_obs = (f(a) for a in (obs, obs0, reward, value_w, term_obs))
    done = np.asarray(done).astype(np.uint8)
    K, N, D = obs.shape
    g, lm = np.float64(gamma).astype(dtype), np.float64(lam).astype(dtype)       # each rounded once
    c = g * lm                                                                # formed in T
    assert c.dtype == dtype
    ln = _lengths(length, K, N)
    wl = value_w[:, np.arange(N) % P]
    adv, ret, value = (np.zeros((K, N), dtype) for _ in range(3))
    trace = np.zeros(N, dtype)
    zero = dtype(0)
    with np.errstate(all="ignore"):
        for k in range(K - 1, -1, -1):
            counted = k < ln
            v = _val(obs0 if k == 0 else obs[k - 1], wl)
            flag = done[k]
            hard = (flag & 5) != 0
            trunc = ~hard & ((flag & 2) != 0)
            at_end = _val(term_obs[k], wl) if term_obs is not None else np.zeros(N, dtype)
            nv = np.where(hard, zero, np.where(trunc, at_end, _val(obs[k], wl)))
            delta = (reward[k] + g * nv) - v
            trace = np.where(counted, np.where(hard | trunc, delta, delta + c * trace), trace)
            adv[k] = np.where(counted, trace, zero)
            ret[k] = np.where(counted, trace + v, zero)
            value[k] = np.where(counted, v, zero)
    assert all(a.dtype == dtype for a in (adv, ret, value))
    return dict(adv=adv, ret=ret, value=value)


def moment_index(D):
    """The entry order of lane_mom and mom: {(i, j): index} for i <= j <= D, and the index of b[0]."""
    n = D + 1
    return {(i, j): i * n - i * (i - 1) // 2 + (j - i) for i in range(n) for j in range(i, n)}, n * (n + 1) // 2


def restate_fit(obs, obs0, target, *, P, dtype, length=None, prev=None, ridge=0.0):
    """os2rv_value_fit, steps 1-4, in numpy and in `dtype`.  obs [K, N, D], obs0 [N, D], target [K, N], prev [D+1, P] or None.
    -> dict(w [D+1, P], lane_mom [E, N], mom [E, P], lane_count [2, N], failed [P], steps [P], valid [P])."""
    f = lambda a: None if a is None else np.asarray(a).astype(dtype)
    obs, obs0, target, prev = (f(a) for a in (obs, obs0, target, prev))
    K, N, D = obs.shape
    S, n = N // P, D + 1
    at, tri = moment_index(D)
    E = tri + n
    ln = _lengths(length, K, N)
    rdg = np.float64(ridge).astype(dtype)
    lane = np.zeros((E, N), dtype)
    one = np.ones(N, dtype)
    with np.errstate(all="ignore"):
        for k in range(K - 1, -1, -1):                                        # step 1
            counted = k < ln
            x = obs0 if k == 0 else obs[k - 1]
            y = target[k]
            add = lambda e, term: lane.__setitem__(e, np.where(counted, lane[e] + term, lane[e]))
            for i in range(D):
                for j in range(i, D):
                    add(at[(i, j)], x[:, i] * x[:, j])
                add(at[(i, D)], x[:, i])
                add(tri + i, x[:, i] * y)
            add(at[(D, D)], one)
            add(tri + D, y)
        fine = np.isfinite(lane).all(0)                                       # step 2
        shaped = fine.reshape(S, P)
        mom = chunked_sum(lane.reshape(E, S, P), shaped)                      # step 3
        count = np.stack([ln.astype(np.int32), fine.astype(np.int32)])
        steps, valid = (chunked_sum(row.reshape(S, P), shaped) for row in count)
        w, failed = np.zeros((n, P), dtype), np.zeros(P, np.int32)
        for p in range(P):                                                    # step 4
            A = lambda i, j: mom[at[(i, j)], p] + rdg if i == j else mom[at[(i, j)], p]
            L = np.zeros((n, n), dtype)
            for j in range(n):
                t = A(j, j)
                if j > 0:
                    st = L[j, 0] * L[j, 0]
                    for q in range(1, j):
                        st = st + L[j, q] * L[j, q]
                    t = t - st
                if not (np.isfinite(t) and t > 0):
                    failed[p] = j + 1
                    break
                L[j, j] = np.sqrt(t)
                for i in range(j + 1, n):
                    u = A(j, i)
                    if j > 0:
                        su = L[i, 0] * L[j, 0]
                        for q in range(1, j):
                            su = su + L[i, q] * L[j, q]
                        u = u - su
                    L[i, j] = u / L[j, j]
            if failed[p]:
                w[:, p] = 0 if prev is None else prev[:, p]
                continue
            z = np.zeros(n, dtype)
            for i in range(n):
                rhs = mom[tri + i, p]
                if prev is not None:
                    rhs = rhs + rdg * prev[i, p]
                if i > 0:
                    s = L[i, 0] * z[0]
                    for q in range(1, i):
                        s = s + L[i, q] * z[q]
                    rhs = rhs - s
                z[i] = rhs / L[i, i]
            for i in range(n - 1, -1, -1):
                v = z[i]
                if i + 1 < n:
                    s = L[i + 1, i] * w[i + 1, p]
                    for q in range(i + 2, n):
                        s = s + L[q, i] * w[q, p]
                    v = v - s
                w[i, p] = v / L[i, i]
    assert all(a.dtype == dtype for a in (w, lane, mom)) and all(a.dtype == np.int32 for a in (count, failed, steps, valid))
    return dict(w=w, lane_mom=lane, mom=mom, lane_count=count, failed=failed, steps=steps, valid=valid)


# ---------------------------------------------------------------------------------------
# the restatements against the textbook
# ---------------------------------------------------------------------------------------
def plain_critic(dtype, seed=0, K=12, P=4, S=96, D=10):
    """A window as the example sees one, rounded to `dtype` and returned in float64: observations uniform in [-1, 1], mixed
    lengths, falls, truncations with terminal observations, no lane invalid."""
    rng = np.random.default_rng(seed)
    N = S * P
    r = lambda a: a.astype(dtype).astype(np.float64)
    u = rng.uniform(size=(K, N))
    done = np.where(u < 0.06, 1, np.where(u < 0.10, 2, 0)).astype(np.uint8)
    return dict(obs0=r(rng.uniform(-1, 1, (N, D))), obs=r(rng.uniform(-1, 1, (K, N, D))), term=r(rng.uniform(-1, 1, (K, N, D))),
                reward=r(rng.uniform(0, 1, (K, N))), done=done, length=rng.integers(1, K + 1, N).astype(np.int32),
                w=r(rng.normal(0, 0.5, (D + 1, P))), prev=r(rng.normal(0, 0.5, (D + 1, P))), K=K, P=P, S=S, D=D, N=N)


def _far(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def textbook_gae(c, gamma, lam, w, term=True, length=True):
    """A_k = sum_i (gamma lambda)^i delta_{k+i} within an episode, in float64: the deltas from matrix products, the sum written
    out per step.  -> (adv, ret) [K, N], 0 where k >= len"""
    K, N, P = c["K"], c["N"], c["P"]
    wl = w[:, np.arange(N) % P]                                                # [D+1, N]
    V = lambda X: np.einsum("...nd,dn->...n", X, wl[:-1]) + wl[-1]
    prev = np.concatenate([c["obs0"][None], c["obs"][:-1]])
    v, v_next = V(prev), V(c["obs"])
    hard, trunc = (c["done"] & 5) != 0, ((c["done"] & 5) == 0) & ((c["done"] & 2) != 0)
    v_next = np.where(hard, 0.0, np.where(trunc, V(c["term"]) if term else 0.0, v_next))
    delta = c["reward"] + gamma * v_next - v
    ln = c["length"] if length else np.full(N, K)
    adv = np.zeros((K, N))
    for l in range(N):
        for k in range(ln[l]):
            i = k
            while True:
                adv[k, l] += (gamma * lam) ** (i - k) * delta[i, l]
                if hard[i, l] or trunc[i, l] or i == ln[l] - 1:
                    break
                i += 1
    counted = np.arange(K)[:, None] < ln[None]
    return adv, np.where(counted, adv + v, 0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restated_gae_is_the_textbook_sum_of_deltas(dtype):
    """adv against A_k = sum_i (gamma lambda)^i delta_{k+i} within an episode, and ret at lambda = 1 with a zero critic and no
    truncation against the plain discounted reward-to-go, both in float64, within MARGIN x the distance measured when this was
    written (relative to the largest entry): see MEASURED."""
    c = plain_critic(dtype)
    K, N, P = c["K"], c["N"], c["P"]
    gamma, lam = float(dtype(0.97)), float(dtype(0.9))
    got = restate_gae(c["obs"], c["obs0"], c["reward"], c["done"], c["w"], P=P, dtype=dtype, term_obs=c["term"], length=c["length"],
                      gamma=gamma, lam=lam)
    assert all(np.isfinite(a).all() for a in got.values())
    adv, ret = textbook_gae(c, gamma * 1.0, lam, c["w"])
    far_adv = max(_far(got["adv"], adv), _far(got["ret"], ret))
    # lambda = 1, a zero critic, no truncation (bit 1 cleared): ret is the discounted reward-to-go
    done = c["done"] & 1
    zero = restate_gae(c["obs"], c["obs0"], c["reward"], done, np.zeros_like(c["w"]), P=P, dtype=dtype, length=c["length"], gamma=gamma, lam=1.0)
    G, rtg = np.zeros(N), np.zeros((K, N))
    for k in range(K - 1, -1, -1):
        counted = k < c["length"]
        G = np.where(counted, np.where(done[k] != 0, c["reward"][k], c["reward"][k] + gamma * G), G)
        rtg[k] = np.where(counted, G, 0.0)
    far_ret = _far(zero["ret"], rtg)
    assert np.array_equal(zero["adv"], zero["ret"]) and (zero["value"] == 0).all()
    print(f"restate_gae against the textbook, {dtype.__name__}: adv {far_adv:.3e}, ret {far_ret:.3e}")
    assert far_adv <= MARGIN * MEASURED[dtype]["adv"], far_adv
    assert far_ret <= MARGIN * MEASURED[dtype]["ret"], far_ret


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restated_fit_is_least_squares(dtype):
    """w against np.linalg.lstsq in float64 on the stacked system [phi; sqrt(ridge) I] w = [y; sqrt(ridge) prev] of every policy,
    ridge 0 and 1e-3, within MARGIN x the distance measured when this was written: see MEASURED."""
    c = plain_critic(dtype)
    K, N, P, S, D = c["K"], c["N"], c["P"], c["S"], c["D"]
    target = restate_gae(c["obs"], c["obs0"], c["reward"], c["done"], c["w"], P=P, dtype=dtype, term_obs=c["term"], length=c["length"],
                         gamma=0.97, lam=0.9)["ret"].astype(np.float64)
    prev_rows = np.concatenate([c["obs0"][None], c["obs"][:-1]])
    counted = np.arange(K)[:, None] < c["length"][None]
    for name, ridge in zip(("fit0", "fit1"), RIDGES):
        ridge = float(dtype(ridge))
        got = restate_fit(c["obs"], c["obs0"], target, P=P, dtype=dtype, length=c["length"], prev=c["prev"], ridge=ridge)
        # the data are chosen so that no policy fails and every lane is valid
        assert got["failed"].tolist() == [0] * P and got["valid"].tolist() == [S] * P and got["lane_count"][1].all()
        assert np.array_equal(got["steps"], c["length"].reshape(S, P).sum(0))
        want = np.zeros((D + 1, P))
        for p in range(P):
            mine = counted & ((np.arange(N) % P) == p)[None]
            phi = np.concatenate([prev_rows[mine], np.ones((mine.sum(), 1))], 1)
            A = np.concatenate([phi, np.sqrt(ridge) * np.eye(D + 1)])
            b = np.concatenate([target[mine], np.sqrt(ridge) * c["prev"][:, p]])
            want[:, p] = np.linalg.lstsq(A, b, rcond=None)[0]
        far = _far(got["w"], want)
        print(f"restate_fit against lstsq, {dtype.__name__}, ridge {ridge:g}: {far:.3e}")
        assert far <= MARGIN * MEASURED[dtype][name], (name, far)


# ---------------------------------------------------------------------------------------
# crafted inputs and edge semantics
# ---------------------------------------------------------------------------------------
def crafted_critic(K, P, S, D, dtype, seed=0, zero_col=None):
    """The inputs of the GPU tests, in `dtype`.  By lane l = s P + p (where the shape reaches it):
      l % 11 == 1, 2, 3, 4   length 0, K, -3 and K + 5
      l % 7 == 6             NaNs in obs, term_obs, reward and target at every step k >= len: they change nothing
      s % 8 == 5 (S >= 6)    an invalid lane: a NaN reward and a NaN target at step 0, the length K
      p == 2 (P > 2)         the same in every lane of the policy: none of its lanes is valid
    done bytes: 0 with probability 0.7, else one of 1, 2, 3, 4, 6, 8, 255 -- a fall, a truncation, both, the guard, the guard on a
    truncation, a bit nobody reads, all.  zero_col: that observation column is 0 everywhere (a rank-deficient batch).
    -> dict(obs, obs0, term_obs, reward, done, length, value_w, prev, target)"""
    rng = np.random.default_rng(seed)
    N = S * P
    l = np.arange(N)
    s, p = l // P, l % P
    obs, obs0, term = rng.uniform(-1, 1, (K, N, D)), rng.uniform(-1, 1, (N, D)), rng.uniform(-1, 1, (K, N, D))
    if zero_col is not None:
        obs[:, :, zero_col], obs0[:, zero_col] = 0.0, 0.0
    reward, target = rng.uniform(0, 1, (K, N)), rng.normal(0, 1, (K, N))
    done = np.where(rng.uniform(size=(K, N)) < 0.7, 0, rng.choice([1, 2, 3, 4, 6, 8, 255], (K, N)))
    length = rng.integers(1, K + 1, N).astype(np.int32)
    for rest, value in ((1, 0), (2, K), (3, -3), (4, K + 5)):
        length[l % 11 == rest] = value
    broken = ((s % 8 == 5) & (S >= 6)) | ((p == NONE_VALID) & (P > 2))
    length[broken] = K
    reward[0, broken], target[0, broken] = np.nan, np.nan
    beyond = (np.arange(K)[:, None] >= np.clip(length, 0, K)[None]) & (l % 7 == 6)[None]
    obs[beyond], term[beyond], reward[beyond], target[beyond] = np.nan, np.nan, np.nan, np.nan
    f = lambda a: np.ascontiguousarray(a.astype(dtype))
    return dict(obs=f(obs), obs0=f(obs0), term_obs=f(term), reward=f(reward), done=np.ascontiguousarray(done.astype(np.uint8)), length=length,
                value_w=f(rng.normal(0, 0.5, (D + 1, P))), prev=f(rng.normal(0, 0.5, (D + 1, P))), target=f(target))


def broken_lanes(P, S):
    l = np.arange(S * P)
    return ((l // P % 8 == 5) & (S >= 6)) | ((l % P == NONE_VALID) & (P > 2))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_edge_semantics_of_the_restated_gae(dtype):
    K, P, S, D = 9, 3, 65, 10
    c = crafted_critic(K, P, S, D, dtype)
    N, l = S * P, np.arange(S * P)
    kw = dict(P=P, dtype=dtype, length=c["length"], gamma=0.97, lam=0.9)
    out = restate_gae(c["obs"], c["obs0"], c["reward"], c["done"], c["value_w"], term_obs=c["term_obs"], **kw)
    bare = restate_gae(c["obs"], c["obs0"], c["reward"], c["done"], c["value_w"], **kw)
    ln = np.clip(c["length"], 0, K)
    # the four lengths: 0 and -3 count nothing, K and K + 5 everything; nothing behind len
    assert set(c["length"][[1, 2, 3, 4]]) == {0, K, -3, K + 5} and ln[1] == 0 == ln[3] and ln[2] == K == ln[4]
    behind = np.arange(K)[:, None] >= ln[None]
    for a in out.values():
        assert (a[behind] == 0).all() and (a[:, 1] == 0).all() and (a[:, 3] == 0).all()
    # a NaN reward poisons its own lane's adv and no other; NaNs beyond len change nothing
    broken = broken_lanes(P, S)
    assert np.isnan(out["adv"][0, broken]).all() and np.isfinite(out["adv"][:, ~broken]).all() and np.isfinite(out["value"]).all()
    assert ((l % 7 == 6) & (ln < K) & ~broken).any()
    g, c_ = dtype(0.97), dtype(0.97) * dtype(0.9)
    wl = c["value_w"][:, l % P]
    flags = c["done"]
    seen = set()
    for k, lane in np.argwhere(~behind & ~broken[None] & (np.arange(K)[:, None] < ln[None] - 1)):
        f = int(flags[k, lane])
        v, r = out["value"][k, lane], c["reward"][k, lane]
        if f & 5:                                                            # a fall, the guard: nothing behind the step
            want, kind = r - v, "hard"
        elif f & 2:                                                          # a truncation: the terminal observation's value, or 0
            tv = _val(c["term_obs"][k, lane][None], wl[:, lane][:, None])[0]
            want, kind = (r + g * tv) - v, "trunc"
            assert bare["adv"][k, lane] == r - v and (tv == 0 or want != r - v)
        else:                                                                # bit 3 alone is no flag of this call
            want, kind = ((r + g * out["value"][k + 1, lane]) - v) + c_ * out["adv"][k + 1, lane], "open" if f == 0 else "other-bit"
        assert out["adv"][k, lane] == want and out["ret"][k, lane] == want + v, (k, lane, f)
        seen.add((kind, f))
    assert {f for _, f in seen} == {0, 1, 2, 3, 4, 6, 8, 255} and ("other-bit", 8) in seen and ("hard", 3) in seen and ("hard", 6) in seen
    # one window holds a fall, a truncation and a guard flag in some lane
    per_lane = [set(flags[:ln[i], i]) for i in range(N)]
    assert any({1, 2, 4} <= fs for fs in per_lane)
    # the bootstrap behind the last counted step is val(obs[len - 1])
    lane = int(np.flatnonzero((ln == K) & ~broken & (flags[K - 1] == 0))[0])
    boot = _val(c["obs"][K - 1, lane][None], wl[:, lane][:, None])[0]
    assert out["adv"][K - 1, lane] == (c["reward"][K - 1, lane] + g * boot) - out["value"][K - 1, lane]
    # gamma = 0: adv = r - v;  lambda = 0: adv = delta
    zero = restate_gae(c["obs"], c["obs0"], c["reward"], c["done"], c["value_w"], term_obs=c["term_obs"], P=P, dtype=dtype,
                       length=c["length"], gamma=0.0, lam=0.9)
    keep = ~behind & ~broken[None]
    assert np.array_equal(zero["adv"][keep], (c["reward"] - zero["value"])[keep])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_edge_semantics_of_the_restated_fit(dtype):
    K, P, S, D = 9, 3, 65, 10
    c = crafted_critic(K, P, S, D, dtype)
    N = S * P
    at, tri = moment_index(D)
    assert len(at) == tri == 66 and tri + D + 1 == 77
    broken = broken_lanes(P, S)
    ln = np.clip(c["length"], 0, K)
    kw = dict(P=P, dtype=dtype, length=c["length"], prev=c["prev"])
    out = restate_fit(c["obs"], c["obs0"], c["target"], ridge=0.0, **kw)
    fine = out["lane_count"][1].astype(bool)
    # a lane with a NaN target is left out; a lane of length 0 is valid with zeros for sums; M[D][D] is len
    assert np.array_equal(fine, ~broken) and np.array_equal(out["lane_count"][0], ln) and (out["lane_mom"][:, 1] == 0).all() and fine[1]
    assert np.array_equal(out["lane_mom"][at[(D, D)]], ln.astype(dtype)) and np.isnan(out["lane_mom"][tri + D, broken]).all()
    assert np.isfinite(out["lane_mom"][:, fine]).all() and np.isfinite(out["mom"]).all()
    assert np.array_equal(out["valid"], fine.reshape(S, P).sum(0)) and np.array_equal(out["steps"], np.where(fine, ln, 0).reshape(S, P).sum(0))
    # the policy without a valid lane: zeros for moments; ridge = 0 fails at column 0 and keeps prev, ridge > 0 does not fail
    assert out["valid"][NONE_VALID] == 0 and (out["mom"][:, NONE_VALID] == 0).all()
    assert out["failed"].tolist() == [0, 0, 1] and np.array_equal(out["w"][:, NONE_VALID], c["prev"][:, NONE_VALID])
    assert not np.array_equal(out["w"][:, 0], c["prev"][:, 0]) and np.isfinite(out["w"]).all()
    none = restate_fit(c["obs"], c["obs0"], c["target"], P=P, dtype=dtype, length=c["length"], ridge=0.0)
    assert none["failed"].tolist() == [0, 0, 1] and (none["w"][:, NONE_VALID] == 0).all() and np.array_equal(none["w"][:, :2], out["w"][:, :2])
    pulled = restate_fit(c["obs"], c["obs0"], c["target"], ridge=1e-3, **kw)
    assert pulled["failed"].tolist() == [0, 0, 0]
    np.testing.assert_allclose(pulled["w"][:, NONE_VALID], c["prev"][:, NONE_VALID], rtol=1e-5 if dtype == np.float32 else 1e-13)
    # a rank-deficient batch: a column that is 0 everywhere fails at that column under ridge = 0, not under ridge > 0
    col = 4
    z = crafted_critic(K, P, S, D, dtype, zero_col=col)
    flat = restate_fit(z["obs"], z["obs0"], z["target"], ridge=0.0, **kw)
    assert flat["failed"].tolist() == [col + 1, col + 1, 1] and np.array_equal(flat["w"], c["prev"])
    assert restate_fit(z["obs"], z["obs0"], z["target"], ridge=1e-3, **kw)["failed"].tolist() == [0, 0, 0]
    for shape in SHAPES:
        c = crafted_critic(*shape, dtype)
        out = restate_fit(c["obs"], c["obs0"], c["target"], P=shape[1], dtype=dtype, length=c["length"], prev=c["prev"], ridge=1e-3)
        assert np.array_equal(out["lane_count"][1].astype(bool), ~broken_lanes(shape[1], shape[2])) and np.isfinite(out["w"]).all()


# ---------------------------------------------------------------------------------------
# header, table, exports, resources
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import control, critic
    protos = _prototypes("os2r_critic.h", "os2rv")
    assert [p[0] for p in protos] == list(critic.ENTRY_POINTS) == NAMES
    lib = critic.load()
    for name, ret, args in protos:
        argtypes = critic.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2rv_last_error" else C.c_int)
    gae, fit = protos[2][2], protos[3][2]
    assert len(gae) == 17 and gae[11] == "double gamma" and gae[12] == "double lambda" and gae[-1] == "void* stream"
    assert len(fit) == 18 and fit[9] == "double ridge" and fit[-1] == "void* stream"
    for args in (gae, fit):
        assert args[:4] == ["const Os2rControlLayout* layout", "int32_t nsteps", "int64_t npolicies", "int32_t nsamples"]
    header = _header("os2r_critic.h")
    assert re.search(r"#define OS2R_CRITIC_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert lib.os2rv_abi_version() == critic.ABI_VERSION == 1
    assert CHUNKS == critic.CHUNKS == int(re.search(r"#define OS2RV_CHUNKS (\d+)", header).group(1))
    assert critic.CHUNKS == int(re.search(r"#define OS2RG_CHUNKS (\d+)", _header("os2r_pg.h")).group(1))
    assert critic.LANE_COUNTS == int(re.search(r"#define OS2RV_LANE_COUNTS (\d+)", header).group(1)) == 2
    assert [critic.moments(d) for d in (1, 7, 10, 12)] == [5, 44, 77, 104]
    assert critic.Os2rControlLayout is control.Os2rControlLayout and critic.layout is control.layout
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", critic.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "libos2r_critic.map")) as f:
        assert re.search(r"global:\s*os2rv_\*;\s*local:\s*\*;", f.read())
    # no other header speaks of this library, and the header the sums come from is as it was: it is included, not edited
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "os2r_critic.h":
            assert "os2rv_" not in _header(name) and "os2r_critic" not in _header(name).lower(), name
    assert '#include "os2r_pg.hpp"' in _csrc("os2r_critic.hpp") and "pg_wave_sum<T>" in _csrc("os2r_critic.hpp")


KERNELS = ("critic_value_kernel", "critic_scan_kernel", "critic_moment_kernel", "critic_sum_kernel", "critic_sum_few_kernel",
           "critic_solve_kernel")


def test_kernel_resources():
    """Exactly twelve kernels, the six of os2r_critic.hpp in float and double, are in the built library and none uses scratch:
    private_segment_fixed_size 0, no VGPR or SGPR spill and no AGPRs in the code-object metadata; only the solve uses LDS (the
    factor of every policy of its workgroup, 104 entries x 64 threads)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import critic
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(critic.LIB_PATH)
    meta = kernel_meta.kernel_meta(critic.LIB_PATH)
    assert len(meta) == 12, sorted(meta)
    for kernel in KERNELS:
        for real, size in (("float", 4), ("double", 8)):
            (name,) = [k for k in meta if f"{kernel}<{real}>" in k]
            m = meta[name]
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
            assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 256, (name, m)
            assert m["group_segment_fixed_size"] == (104 * 64 * size if kernel == "critic_solve_kernel" else 0), (name, m)


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
SHAPE_CASES = [(dict(lay=None), b"null layout"), (dict(lay=("dtype", 2)), b"dtype must be"), (dict(lay=("nq", 1)), b"nq must be 2..5"),
               (dict(lay=("obs_dim", 0)), b"obs_dim must be 1..12"), (dict(lay=("obs_dim", 13)), b"obs_dim must be 1..12"),
               (dict(K=0), b"nsteps must be >= 1"), (dict(K=-2), b"nsteps must be >= 1"), (dict(K=65536), b"nsteps must be <= 65535"),
               (dict(P=0), b"npolicies must be >= 1"), (dict(P=-1), b"npolicies must be >= 1"), (dict(S=0), b"nsamples must be >= 1"),
               (dict(S=-4), b"nsamples must be >= 1"), (dict(P=2 ** 62), b"nsamples * npolicies exceeds 2^31 - 1"),
               (dict(P=2 ** 30, S=2), b"nsamples * npolicies exceeds 2^31 - 1"), (dict(P=1, S=2 ** 30, K=2), b"nsamples * nsteps exceeds 2^31 - 1")]


def _refusal_rig(sizes, first_output):
    """A host buffer and the element offsets of the arrays `sizes` (in elements of 8 bytes) in it: the inputs from element 0, the
    outputs from element 4096."""
    buf = (C.c_double * 8192)()
    base = (C.addressof(buf) + 15) & ~15
    at = lambda i: C.c_void_p(base + 8 * i)
    where, nxt = {}, 0
    for name, n in sizes.items():
        if name == first_output:
            assert nxt < 4096
            nxt = 4096
        where[name] = nxt
        nxt += (n + 1) & ~1
    assert nxt < 8000
    return buf, at, where


def _lay(dtype=abi.F64, **kw):
    from gym_os2r_amd import control
    lay = control.layout(dtype, 3, 0, [0, 1, 3, -1])
    for k, v in kw.items():
        setattr(lay, k, v)
    return C.byref(lay)


def _run_refusals(entry, good, cases, edges, buf, fails_in_source):
    from gym_os2r_amd import critic
    lib = critic.load()
    fn, prefix = getattr(lib, entry), entry.encode() + b": "
    assert len(good) + 1 == len(critic.ENTRY_POINTS[entry])

    def call(**kw):
        a = dict(good, **kw)
        if isinstance(a["lay"], tuple):
            a["lay"] = _lay(**{a["lay"][0]: a["lay"][1]})
        return fn(*[a[k] for k in good], None)
    assert fn(*[None if _is_pointer(t) else 0 for t in critic.ENTRY_POINTS[entry]]) == abi.ERR_INVALID
    assert lib.os2rv_last_error() == prefix + b"null layout"
    seen = set()
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.os2rv_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(prefix), (kw.keys(), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases})                     # each cause has a text of its own
    assert not any(buf)                                                   # a refused call wrote nothing
    for kw in edges:                                  # (device 1000 is never there, with a GPU or without)
        kw = dict(kw, lay=_lay(device=1000))
        assert call(**kw) == abi.ERR_NO_DEVICE and lib.os2rv_last_error().startswith(prefix), kw
    assert not any(buf)
    # the source: no HIP call and every refusal of an argument before check_device
    body = _function(_csrc("os2r_critic_capi.hip"), "int " + entry)
    first_hip = body.index("check_device(")
    assert not re.search(HIP_CALL, body[:first_hip]) and body.index("DeviceGuard") > first_hip and body.index("auto launch") > first_hip
    fails = [m.start() for m in re.finditer(r"fail\(OS2R_ERR_INVALID", body)]
    assert len(fails) == fails_in_source and all(i < first_hip for i in fails)
    texts = re.findall(r'"([^"]+)"', body[:first_hip])[1:]              # (the first string is the entry point's prefix)
    helper = _function(_csrc("os2r_critic_capi.hip"), r"const char\* shape_refusal")
    assert not re.search(HIP_CALL, helper)
    texts += re.findall(r'return "([^"]+)";', helper)
    assert len(texts) == len(set(texts))
    for t in texts:
        assert any(t.encode() in e for e in seen) or t.endswith("_dev") or t == " overlaps ", t     # (the names of the spans)
    return seen


def test_gae_refusals_come_through_ctypes_without_a_device():
    K, P, S, D = 3, 2, 2, 4
    N = S * P
    sizes = dict(obs=K * N * D, obs0=N * D, term=K * N * D, reward=K * N, done=K * N, length=N, w=(D + 1) * P, adv=K * N, ret=K * N,
                 value=K * N)
    buf, at, where = _refusal_rig(sizes, "adv")
    nan, inf = float("nan"), float("inf")
    good = dict(lay=_lay(), K=K, P=P, S=S, obs=at(where["obs"]), obs0=at(where["obs0"]), term=at(where["term"]), reward=at(where["reward"]),
                done=at(where["done"]), length=at(where["length"]), w=at(where["w"]), gamma=0.99, lam=0.95, adv=at(where["adv"]),
                ret=at(where["ret"]), value=at(where["value"]))
    cases = SHAPE_CASES + [
        (dict(gamma=nan), b"gamma must be finite"), (dict(gamma=inf), b"gamma must be finite"), (dict(gamma=-inf), b"gamma must be finite"),
        (dict(gamma=-1e-300), b"gamma must be in [0, 1]"), (dict(gamma=1.0000001), b"gamma must be in [0, 1]"),
        (dict(lam=nan), b"lambda must be finite"), (dict(lam=-inf), b"lambda must be finite"), (dict(lam=-1e-300), b"lambda must be in [0, 1]"),
        (dict(lam=2.0), b"lambda must be in [0, 1]"),
        (dict(obs=None), b"null obs_dev"), (dict(obs0=None), b"null obs0_dev"), (dict(reward=None), b"null reward_dev"),
        (dict(done=None), b"null done_dev"), (dict(w=None), b"null value_w_dev"), (dict(adv=None), b"null adv_dev"),
        (dict(value=None), b"null value_dev"),
        # an output over an input, from both sides; over another output; the optional ones too
        (dict(adv=at(where["obs"] + sizes["obs"] - 1)), b"adv_dev overlaps obs_dev"),
        (dict(adv=at(where["obs0"] - K * N + 1)), b"adv_dev overlaps obs_dev"),
        (dict(value=at(where["obs0"])), b"value_dev overlaps obs0_dev"), (dict(ret=at(where["term"] + 3)), b"ret_dev overlaps term_obs_dev"),
        (dict(adv=at(where["reward"])), b"adv_dev overlaps reward_dev"), (dict(value=at(where["done"])), b"value_dev overlaps done_dev"),
        (dict(ret=at(where["length"] + 1)), b"ret_dev overlaps length_dev"), (dict(adv=at(where["w"] + 1)), b"adv_dev overlaps value_w_dev"),
        (dict(ret=at(where["adv"] + K * N - 1)), b"ret_dev overlaps adv_dev"), (dict(value=at(where["adv"])), b"value_dev overlaps adv_dev"),
        (dict(value=at(where["ret"] + 1)), b"value_dev overlaps ret_dev")]
    edges = [dict(K=65535, S=1, P=1, obs=at(10 ** 6), term=at(2 * 10 ** 6), reward=at(3 * 10 ** 6), done=at(4 * 10 ** 6), adv=at(5 * 10 ** 6),
                  ret=at(6 * 10 ** 6), value=at(7 * 10 ** 6)),
             dict(gamma=0.0, lam=0.0), dict(gamma=1.0, lam=1.0), dict(gamma=5e-324), dict(term=None, length=None, ret=None),
             dict(term=None, ret=at(where["term"])), dict(ret=at(where["adv"] + K * N))]
    seen = _run_refusals("os2rv_gae", good, cases, edges, buf, fails_in_source=12)
    assert len(seen) == 10 + 4 + 7 + 10


def test_value_fit_refusals_come_through_ctypes_without_a_device():
    K, P, S, D = 3, 2, 2, 4
    N = S * P
    E = (D + 1) * (D + 2) // 2 + D + 1
    sizes = dict(obs=K * N * D, obs0=N * D, target=K * N, length=N, prev=(D + 1) * P, w=(D + 1) * P, lane_mom=E * N, mom=E * P, count=2 * N,
                 failed=P, steps=P, valid=P)
    buf, at, where = _refusal_rig(sizes, "w")
    nan, inf = float("nan"), float("inf")
    good = dict(lay=_lay(), K=K, P=P, S=S, obs=at(where["obs"]), obs0=at(where["obs0"]), target=at(where["target"]), length=at(where["length"]),
                prev=at(where["prev"]), ridge=1e-3, w=at(where["w"]), lane_mom=at(where["lane_mom"]), mom=at(where["mom"]),
                count=at(where["count"]), failed=at(where["failed"]), steps=at(where["steps"]), valid=at(where["valid"]))
    cases = SHAPE_CASES + [
        (dict(ridge=nan), b"ridge must be finite"), (dict(ridge=inf), b"ridge must be finite"), (dict(ridge=-inf), b"ridge must be finite"),
        (dict(ridge=-1e-300), b"ridge must be >= 0"), (dict(ridge=-1.0), b"ridge must be >= 0"),
        (dict(obs=None), b"null obs_dev"), (dict(obs0=None), b"null obs0_dev"), (dict(target=None), b"null target_dev"),
        (dict(w=None), b"null w_dev"), (dict(lane_mom=None), b"null lane_mom_dev"), (dict(mom=None), b"null mom_dev"),
        (dict(count=None), b"null lane_count_dev"),
        (dict(w=at(where["obs"] + sizes["obs"] - 1)), b"w_dev overlaps obs_dev"), (dict(w=at(where["obs0"] - sizes["w"] + 1)), b"w_dev overlaps obs_dev"),
        (dict(lane_mom=at(where["obs0"])), b"lane_mom_dev overlaps obs0_dev"), (dict(mom=at(where["target"])), b"mom_dev overlaps target_dev"),
        (dict(count=at(where["length"])), b"lane_count_dev overlaps length_dev"), (dict(w=at(where["prev"])), b"w_dev overlaps prev_w_dev"),
        (dict(failed=at(where["prev"] + 1)), b"failed_dev overlaps prev_w_dev"), (dict(steps=at(where["obs"])), b"steps_dev overlaps obs_dev"),
        (dict(valid=at(where["target"] + 2)), b"valid_dev overlaps target_dev"),
        (dict(lane_mom=at(where["w"] + sizes["w"] - 1)), b"lane_mom_dev overlaps w_dev"), (dict(mom=at(where["lane_mom"])), b"mom_dev overlaps lane_mom_dev"),
        (dict(count=at(where["mom"] + 1)), b"lane_count_dev overlaps mom_dev"), (dict(failed=at(where["count"])), b"failed_dev overlaps lane_count_dev"),
        (dict(steps=at(where["failed"])), b"steps_dev overlaps failed_dev"), (dict(valid=at(where["steps"])), b"valid_dev overlaps steps_dev")]
    edges = [dict(K=65535, S=1, P=1, obs=at(10 ** 6), target=at(3 * 10 ** 6)), dict(ridge=0.0), dict(ridge=5e-324), dict(ridge=1e308),
             dict(length=None, prev=None), dict(failed=None, steps=None, valid=None), dict(prev=None, w=at(where["prev"])),
             dict(lane_mom=at(where["w"] + sizes["w"]))]
    seen = _run_refusals("os2rv_value_fit", good, cases, edges, buf, fails_in_source=11)
    assert len(seen) == 10 + 2 + 7 + 14


# ---------------------------------------------------------------------------------------
# the Python layer, without a device
# ---------------------------------------------------------------------------------------
def test_python_argument_errors_need_no_device(monkeypatch):
    import torch
    from gym_os2r_amd import critic
    from gym_os2r_amd.sim import HipSim
    from test_pg_host import _bare
    assert all(callable(getattr(HipSim, m)) for m in ("gae", "gae_into", "value_fit", "value_fit_into"))
    assert critic.Os2rCriticLibraryMissing.__mro__[1] is ImportError and critic.LIB_PATH.endswith("libos2r_critic.so")

    def no_load():
        raise AssertionError("a refused call reached critic.load")
    monkeypatch.setattr(critic, "load", no_load)
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    s = _bare(f64)
    K, P, S, D = 3, 2, 2, 4
    N, E = S * P, critic.moments(4)
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    obs, obs0, rew, done, w = z(K, N, D), z(N, D), z(K, N), z(K, N, dtype=u8), z(D + 1, P)
    adv, val = z(K, N), z(K, N)

    def gae_into(*args, **kw):
        with pytest.raises(ValueError, match="^gae: "):
            s.gae_into(*args, **dict(dict(obs0=obs0, policies=P), **kw))

    def gae(*args, **kw):
        with pytest.raises(ValueError, match="^gae: "):
            s.gae(*args, **dict(dict(obs0=obs0, policies=P), **kw))
    full = (obs, rew, done, w, adv, val)
    for bad in (0, -1, 3, 2.0, True, None, "2"):
        gae_into(*full, policies=bad)
        gae(obs, rew, done, w.t(), policies=bad)
    for bad in (float("nan"), float("inf"), -0.1, 1.5, "x", None, True):
        gae_into(*full, gamma=bad)
        gae_into(*full, lam=bad)
        gae(obs, rew, done, w.t(), lam=bad)
    for i in range(len(full)):
        gae_into(*[None if j == i else t for j, t in enumerate(full)])
    gae_into(*full, obs0=None)
    gae(obs, rew, done, None)
    gae(obs, rew, done, z(D + 1, P + 1).t())
    for args in ((z(K, N), rew, done, w, adv, val), (z(K, N, D + 1), rew, done, w, adv, val), (obs.float(), rew, done, w, adv, val),
                 (obs, z(K, N + 1), done, w, adv, val), (obs, rew, z(K, N), w, adv, val), (obs, rew, done, z(P, D + 1), adv, val),
                 (obs, rew, done, w, z(N, K), val), (obs, rew, done, w, adv, z(K, N).float()), (obs, rew, done, w, adv, adv),
                 (obs, rew, done, w, rew, val), (obs, rew, done, w, adv, obs.reshape(-1)[:K * N].reshape(K, N))):
        gae_into(*args)
    for kw in (dict(obs0=z(N, D + 1)), dict(term_obs=z(K, N, D + 1)), dict(length=z(N)), dict(ret=z(K, N + 1)), dict(ret=adv), dict(ret=rew)):
        gae_into(*full, **kw)

    target, lane_mom, mom, count, wout = z(K, N), z(E, N), z(E, P), z(2, N, dtype=i32), z(D + 1, P)

    def fit_into(*args, **kw):
        with pytest.raises(ValueError, match="^value_fit: "):
            s.value_fit_into(*args, **dict(dict(obs0=obs0, policies=P), **kw))

    def fit(*args, **kw):
        with pytest.raises(ValueError, match="^value_fit: "):
            s.value_fit(*args, **dict(dict(obs0=obs0, policies=P), **kw))
    whole = (obs, target, wout, lane_mom, mom, count)
    for bad in (0, -1, 3, True, None):
        fit_into(*whole, policies=bad)
        fit(obs, target, policies=bad)
    for bad in (float("nan"), float("inf"), -0.1, "x", None, True):
        fit_into(*whole, ridge=bad)
    for i in range(len(whole)):
        fit_into(*[None if j == i else t for j, t in enumerate(whole)])
    fit_into(*whole, obs0=None)
    fit(obs, target, prev=z(P + 1, D + 1))
    for args in ((obs, z(K, N + 1), wout, lane_mom, mom, count), (obs, target, z(P, D + 1), lane_mom, mom, count),
                 (obs, target, wout, z(E + 1, N), mom, count), (obs, target, wout, lane_mom, z(P, E), count),
                 (obs, target, wout, lane_mom, mom, z(2, N)), (obs, target, wout, lane_mom, mom, z(4, N, dtype=i32)),
                 (obs, target, wout, lane_mom, lane_mom.reshape(-1)[:E * P].reshape(E, P), count)):
        fit_into(*args)
    for kw in (dict(prev=z(P, D + 1)), dict(prev=wout), dict(length=z(N + 1, dtype=i32)), dict(failed=z(P)), dict(steps=z(P + 1, dtype=i32)),
               dict(valid=count[0, :P]), dict(obs0=z(N, D).float())):
        fit_into(*whole, **kw)
    # what passes every check reaches the loader, and only then
    with pytest.raises(AttributeError):                                    # (the bare handle has no cfg to fill a layout from)
        s.gae_into(*full, obs0=obs0, policies=P)
    with pytest.raises(AttributeError):
        s.value_fit_into(*whole, obs0=obs0, policies=P)
