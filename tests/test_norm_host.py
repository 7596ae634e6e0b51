"""libos2r_norm.so (include/os2r_norm.h): the host side -- the numpy restatements of the three calls the GPU tests compare with
(`restate_stats`, `restate_fold`, `restate_unfold`), written from the header alone; the restatement of the statistics against an
independent statement (a float64 two-pass np.mean / np.var over the concatenation of three successive batches) in the regime
whitening is for, and against the unshifted float32 formula; merge and shard; the fold against the whitened policy in float64,
the identity and the floor; the unfold against torch autograd; the header against the one table of gym_os2r_amd/norm.py, the
exports of the library, the resources of the eight kernels in the built library; every refusal of the three entry points
through ctypes without a device; and the argument checks of HipSim.obs_stats / norm_fold / norm_unfold that need no device.
No GPU needed.

Measured on the CPU this test was written on (test_the_restatement_against_two_pass_statistics prints them), as the worst
|d mean| / std and the worst |d var| / var over every policy and component, var = m2 / count:
    float64 restatement against the two-pass statement     mean 3.608e-13   var 1.186e-15
    float32 restatement against its float64 self            mean 3.809e-06   var 5.546e-07
    unshifted float32 sums against the two-pass statement   var 1.167e-01 (the shifted float32 restatement: 5.545e-07)
(the mean's figure is in units of the component's deviation: at a mean of 50 and a deviation of 0.1 one unit in the last place
of the mean is 500 of them).  The bounds are MARGIN = 8 times the first two.  The fold, as the largest difference of an action
over the largest action: float64 3.083e-14, float32 4.926e-06."""
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

NAMES = ["os2rz_abi_version", "os2rz_last_error", "os2rz_obs_stats", "os2rz_fold", "os2rz_unfold"]
CHUNKS = 64
FLOOR = 1e-6
# |d mean| / std and |d var| / var: what a whitened observation moves by, in units of its own deviation, and what its scale is off by
MEASURED = {np.float64: dict(mean=3.608e-13, var=1.186e-15), np.float32: dict(mean=3.809e-06, var=5.546e-07)}
# the fold: the largest |W . [x; 1] - theta . [(x - mu) r; 1]| over the largest |action| of the reference
MEASURED_FOLD = {np.float64: 3.083e-14, np.float32: 4.926e-06}
MARGIN = 8
FORBIDDEN = ("os2rg_", "os2r_pg", "os2rv_", "os2r_critic", "os2ro_", "os2r_ppo", "os2rn_", "os2r_npg", "os2rx_", "os2r_cem", "os2ra_", "os2r_es",
             "os2ru_", "os2r_ukf", "os2re_", "os2r_ekf", "os2rp_", "os2r_pf", "os2rm_", "mppi", "os2rt_", "steer", "line_search")


# ---------------------------------------------------------------------------------------
# the restatements of include/os2r_norm.h (need no device)
# ---------------------------------------------------------------------------------------
def chunked(terms, fine):
    """Step 3: the sum over the valid lanes (fine [S, P] bool) of terms [S, P, ...] in 64 partials and the adjacent-pair tree;
    partial c walks s = c, c + 64, ... in ascending order."""
    S = fine.shape[0]
    parts = []
    for c in range(CHUNKS):
        acc = np.zeros(terms.shape[1:], terms.dtype)
        for s in range(c, S, CHUNKS):
            k = fine[s].reshape(fine[s].shape + (1,) * (acc.ndim - 1))
            acc = np.where(k, acc + terms[s], acc)
        parts.append(acc)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
    return parts[0]


def empty_state(P, D, dtype):
    return np.zeros(P, np.int64), np.zeros((P, D), dtype), np.zeros((P, D), dtype)


def restate_stats(obs, *, P, dtype, obs0=None, length=None, state=None):
    """include/os2r_norm.h, os2rz_obs_stats, steps 1-4, in numpy and in `dtype`.  obs [K, N, D], obs0 [N, D] | None, length [N] |
    None, state (count [P] int64, mean [P, D], m2 [P, D]) | None.
    -> dict(count, mean, m2, steps, valid, lane_sum [2 D, N], lane_count [2, N])."""
    obs = np.asarray(obs).astype(dtype)
    K, N, D = obs.shape
    S = N // P
    assert S * P == N
    zero = dtype(0)
    xs = obs if obs0 is None else np.concatenate([np.asarray(obs0).astype(dtype)[None], obs[:-1]])
    ln = np.full(N, K, np.int32) if length is None else np.clip(np.asarray(length, np.int64), 0, K).astype(np.int32)
    count_in, mean_in, m2_in = empty_state(P, D, dtype) if state is None else (np.asarray(state[0], np.int64), np.asarray(state[1]).astype(dtype),
                                                                               np.asarray(state[2]).astype(dtype))
    held = count_in > 0
    na = np.where(held, count_in, 0)
    with np.errstate(all="ignore"):
        x0 = xs[0, :P]                                                              # lane p is sample 0 of policy p
        fresh = np.where((ln[:P] > 0)[:, None] & np.isfinite(x0), x0, zero)            # step 1
        c = np.where(held[:, None], mean_in, fresh).astype(dtype)
        c_lane = np.tile(c, (S, 1))
        A, B = np.zeros((N, D), dtype), np.zeros((N, D), dtype)
        for k in range(K):                                                          # step 2
            m = (k < ln)[:, None]
            dk = np.where(m, xs[k], zero) - c_lane                                   # (a step at or beyond len is never read)
            A = np.where(m, A + dk, A)
            B = np.where(m, B + dk * dk, B)
        fine = np.isfinite(A).all(1) & np.isfinite(B).all(1)
        f = fine.reshape(S, P)
        At, Bt = chunked(A.reshape(S, P, D), f), chunked(B.reshape(S, P, D), f)      # step 3
        nb = chunked(ln.reshape(S, P), f).astype(np.int32)
        nv = chunked(fine.reshape(S, P).astype(np.int32), f).astype(np.int32)
        nbT, naT, ntT = nb.astype(dtype)[:, None], na.astype(dtype)[:, None], (na + nb).astype(dtype)[:, None]
        off = At / nbT                                                              # step 4
        diff = Bt - At * off
        m2b = np.where(diff < zero, zero, diff)
        w = nbT / ntT
        mean_kept, m2_kept = np.where(held[:, None], mean_in, zero), np.where(held[:, None], m2_in, zero)
        mean_new = np.where(held[:, None], mean_kept + off * w, c + off)
        m2_new = np.where(held[:, None], (m2_kept + m2b) + (off * off) * (naT * w), m2b)
        some = (nb > 0)[:, None]
        mean, m2 = np.where(some, mean_new, mean_kept), np.where(some, m2_new, m2_kept)
        count = na + nb.astype(np.int64)
    assert mean.dtype == dtype and m2.dtype == dtype and A.dtype == dtype and count.dtype == np.int64
    return dict(count=count, mean=mean, m2=m2, steps=nb, valid=nv, lane_sum=np.concatenate([A.T, B.T]),
                lane_count=np.stack([ln, fine.astype(np.int32)]))


def _scale(state, dtype, std_floor):
    """-> (scaled [P] bool, mu [P, D], r [P, D]) of os2rz_fold / os2rz_unfold."""
    count, mean, m2 = np.asarray(state[0], np.int64), np.asarray(state[1]).astype(dtype), np.asarray(state[2]).astype(dtype)
    floor = np.float64(std_floor).astype(dtype)
    with np.errstate(all="ignore"):
        sd = np.sqrt(m2 / count.astype(dtype)[:, None])
        sd = np.where(sd < floor, floor, sd)
        r = dtype(1) / sd
    assert r.dtype == dtype
    return count >= 2, mean, r


def restate_fold(theta, state, *, dtype, std_floor=FLOOR):
    """include/os2r_norm.h, os2rz_fold, in numpy and in `dtype`: theta [Q, rows, D+1] (Q a multiple of P; set q under policy
    q mod P) -> weights [Q, rows, D+1]."""
    theta = np.asarray(theta).astype(dtype)
    Q, rows, n = theta.shape
    D = n - 1
    scaled, mu, r = _scale(state, dtype, std_floor)
    p = np.arange(Q) % len(scaled)
    with np.errstate(all="ignore"):
        W = theta[:, :, :D] * r[p][:, None, :]
        s = W[:, :, 0] * mu[p][:, None, 0]
        for d in range(1, D):
            s = s + W[:, :, d] * mu[p][:, None, d]
        out = np.concatenate([W, (theta[:, :, D] - s)[:, :, None]], axis=2)
    out = np.where(scaled[p][:, None, None], out, theta)
    assert out.dtype == dtype
    return out


def restate_unfold(grad, state, *, dtype, std_floor=FLOOR):
    """include/os2r_norm.h, os2rz_unfold, in numpy and in `dtype`: grad [P, rows, D+1] -> grad_theta [P, rows, D+1]."""
    grad = np.asarray(grad).astype(dtype)
    D = grad.shape[2] - 1
    scaled, mu, r = _scale(state, dtype, std_floor)
    with np.errstate(all="ignore"):
        last = grad[:, :, D:]
        out = np.concatenate([(grad[:, :, :D] - last * mu[:, None, :]) * r[:, None, :], last], axis=2)
    out = np.where(scaled[:, None, None], out, grad)
    assert out.dtype == dtype
    return out


def crafted_obs(P, S, K, D, dtype, seed=0):
    """The inputs of the GPU tests, in `dtype`: observations in the regime whitening is for (a mean of up to 50 and a deviation
    between 0.1 and 5 per policy and component) and, by lane l = s P + p, where the shape reaches it:
      len: l % 7 == 2 -> 0, l % 7 == 3 -> -3, l % 7 == 4 -> K + 2, l % 7 == 5 -> ((l // 7) % K) + 1, else K
      s == 1: a NaN at step 0 of component 0 (inside every length > 0: lanes with len > 0 are invalid)
      s == 2: +inf at step 0 of component D - 1
      s == 3: a NaN and -inf at the last step, which is beyond len where len < K: not read there, the lane stays valid
      p == 1 (P > 1): sample 0 starts with a NaN in component 0 -- with an empty state that component's pivot is 0
      p == 2 (P > 2): every lane has len = K and is invalid (a NaN at step 0): the policy's state goes through
    -> dict(obs [K, N, D], obs0 [N, D], length [N] int32)"""
    rng = np.random.default_rng(seed + 1000 * P + 10 * S + K)
    N = S * P
    mu, sd = rng.uniform(-50, 50, (P, D)), rng.uniform(0.1, 5.0, (P, D))
    x = mu[None, None] + sd[None, None] * rng.normal(size=(K + 1, S, P, D))
    l = np.arange(N)
    length = np.select([l % 7 == 2, l % 7 == 3, l % 7 == 4, l % 7 == 5], [0, -3, K + 2, (l // 7) % K + 1], K).astype(np.int32)
    if S > 1:
        x[0:2, 1, :, 0] = np.nan
    if S > 2:
        x[0:2, 2, :, D - 1] = np.inf
    if S > 3:
        x[K - 1:, 3, :, 0] = np.nan
        x[K - 1:, 3, :, D - 1] = -np.inf
    if P > 1:
        x[0:2, 0, 1, 0] = np.nan
    if P > 2:
        x[0:2, :, 2, 0] = np.nan
        length[l % P == 2] = K
    x = x.reshape(K + 1, N, D).astype(dtype)
    return dict(obs=np.ascontiguousarray(x[1:]), obs0=np.ascontiguousarray(x[0]), length=length)


def _regime(P, S, K, D, batches, seed):
    """`batches` successive batches [K, S P, D] in float64 in the `no_norm` regime: component 0 of policy 0 has the mean 50 and
    the deviation 0.1, the others a mean of up to 50 and a deviation between 0.1 and 5."""
    rng = np.random.default_rng(seed)
    mu, sd = rng.uniform(-50, 50, (P, D)), rng.uniform(0.1, 5.0, (P, D))
    mu[0, 0], sd[0, 0] = 50.0, 0.1
    return [mu[None, None] + sd[None, None] * rng.normal(size=(K, S, P, D)) for _ in range(batches)]


def _merged(batches, P, dtype):
    state = None
    for b in batches:
        K, S, _, D = b.shape
        out = restate_stats(b.reshape(K, S * P, D), P=P, dtype=dtype, state=state)
        state = (out["count"], out["mean"], out["m2"])
    return state


def _distance(state, mean_ref, var_ref):
    count, mean, m2 = state
    var = m2.astype(np.float64) / count[:, None]
    return dict(mean=float(np.max(np.abs(mean.astype(np.float64) - mean_ref) / np.sqrt(var_ref))), var=float(np.max(np.abs(var - var_ref) / var_ref)))


def test_the_restatement_against_two_pass_statistics():
    """Three successive batches merged by the restatement against np.mean / np.var (float64, two passes) over their
    concatenation, means up to 50 and deviations from 0.1 to 5: float64 against that statement, float32 against the float64
    restatement on the same rounded inputs, eight times the measured distance each (the module's docstring has the figures).
    On the same data the unshifted float32 formula sum x^2 - (sum x)^2 / n is at least 100 times further off than the shifted
    float32 restatement: the data tests the pivot."""
    P, S, K, D = 3, 5, 40, 10
    batches = _regime(P, S, K, D, 3, seed=3)
    every = np.concatenate([b.reshape(K * S, P, D) for b in batches])
    mean_ref, var_ref = every.mean(0), every.var(0)
    assert np.abs(mean_ref).max() > 40 and np.sqrt(var_ref).min() < 0.12 and np.sqrt(var_ref).max() > 4
    s64 = _merged(batches, P, np.float64)
    assert s64[0].tolist() == [3 * K * S] * P
    d64 = _distance(s64, mean_ref, var_ref)
    rounded = [b.astype(np.float32) for b in batches]
    s32 = _merged(rounded, P, np.float32)
    self64 = _merged([b.astype(np.float64) for b in rounded], P, np.float64)
    d32 = _distance(s32, self64[1], self64[2] / self64[0][:, None])
    print(f"[norm restatement] float64 against two passes {d64}, float32 against its float64 self {d32}")
    for dtype, got in ((np.float64, d64), (np.float32, d32)):
        for name, v in got.items():
            assert v <= MARGIN * MEASURED[dtype][name], (dtype.__name__, name, v, MEASURED[dtype][name])
    assert all(v < 1e-12 for v in MEASURED[np.float64].values()) and all(v < 1e-5 for v in MEASURED[np.float32].values())
    # the unshifted formula in float32 on the same rounded data, against the two-pass statement of that data
    r = np.concatenate([b.reshape(K * S, P, D) for b in rounded])
    ref = r.astype(np.float64).var(0)
    n = np.float32(r.shape[0])
    s1, s2 = r.sum(0, dtype=np.float32), (r * r).sum(0, dtype=np.float32)
    plain = (s2 - s1 * s1 / n) / n
    assert plain.dtype == np.float32
    far_plain = float(np.max(np.abs(plain.astype(np.float64) - ref) / ref))
    far_shifted = float(np.max(np.abs(s32[2].astype(np.float64) / s32[0][:, None] - ref) / ref))
    print(f"[norm restatement] float32 variance: unshifted {far_plain:.3e}, shifted {far_shifted:.3e}")
    assert far_plain >= 100 * far_shifted and far_shifted < 1e-5


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_merge_and_shard(dtype):
    """Three batches merged one after the other stand within the same bound of one call over their concatenation along the
    steps; policies a .. a + M of a wide call equal a call over that slice, bit for bit, crafted lanes and a state included."""
    P, S, K, D = 3, 5, 40, 10
    batches = [b.astype(dtype) for b in _regime(P, S, K, D, 3, seed=4)]
    step = _merged(batches, P, dtype)
    whole = restate_stats(np.concatenate(batches).reshape(3 * K, S * P, D), P=P, dtype=dtype)
    assert np.array_equal(step[0], whole["count"])
    far = _distance(step, whole["mean"].astype(np.float64), whole["m2"].astype(np.float64) / whole["count"][:, None])
    print(f"[norm merge, {dtype.__name__}] three merges against one call: {far}")
    assert all(far[k] <= MARGIN * MEASURED[dtype][k] for k in far), far
    P, S, K, a, M = 6, 66, 7, 2, 3
    c = crafted_obs(P, S, K, D, dtype)
    rng = np.random.default_rng(1)
    state = (np.array([0, 5, 0, 9, 1, 0], np.int64), rng.normal(3, 1, (P, D)).astype(dtype), rng.uniform(1, 2, (P, D)).astype(dtype))
    wide = restate_stats(c["obs"], P=P, dtype=dtype, obs0=c["obs0"], length=c["length"], state=state)
    cut = lambda x, lead: np.ascontiguousarray(x.reshape(lead + (S, P) + x.shape[len(lead) + 1:])[(slice(None),) * (len(lead) + 1) + (slice(a, a + M),)]
                                               ).reshape(lead + (S * M,) + x.shape[len(lead) + 1:])
    part = restate_stats(cut(c["obs"], (K,)), P=M, dtype=dtype, obs0=cut(c["obs0"], ()), length=cut(c["length"], ()),
                         state=tuple(s[a:a + M] for s in state))
    for name in ("count", "mean", "m2", "steps", "valid"):
        assert np.array_equal(wide[name][a:a + M], part[name], equal_nan=True), name
    assert wide["valid"].min() == 0 and wide["valid"].max() > 0 and np.array_equal(wide["count"][2], state[0][2])


def test_the_crafted_observations_reach_every_branch():
    P, S, K, D = 5, 64, 7, 10
    c = crafted_obs(P, S, K, D, np.float64)
    out = restate_stats(c["obs"], P=P, dtype=np.float64, obs0=c["obs0"], length=c["length"])
    ln, fine = out["lane_count"]
    l = np.arange(S * P)
    assert set(ln.tolist()) == set(range(K + 1)) and (ln[(l % 7 == 3) & (l % P != 2)] == 0).all() and (ln[l % 7 == 4] == K).all() and ln[0] == ln[1] == K
    f = fine.reshape(S, P).astype(bool)
    lens = ln.reshape(S, P)
    assert not f[1][lens[1] > 0].any() and not f[2][lens[2] > 0].any() and f[1:3][lens[1:3] == 0].all() and (lens[1:3] == 0).any()   # NaN and inf inside the length
    assert f[3][lens[3] < K].all() and not f[3][lens[3] == K].any() and (lens[3] < K).any()              # the same beyond it: not read
    assert not f[:, 2].any() and out["count"][2] == 0 and (out["mean"][2] == 0).all() and out["valid"][2] == 0      # no valid lane
    assert out["steps"][2] == 0 and (out["valid"][[0, 1, 3, 4]] > 30).all() and np.isfinite(out["mean"]).all() and (out["m2"] >= 0).all()
    assert np.array_equal(out["count"], out["steps"].astype(np.int64))
    # policy 1: sample 0 starts with a NaN in component 0, so that component's pivot is 0 and the lane is invalid -- the mean is still right
    assert np.isnan(c["obs0"][1, 0]) and not f[0, 1] and abs(out["mean"][1, 0]) > 1
    # a non-empty state: the pivot is the running mean; a policy without a valid lane keeps its state bit for bit
    rng = np.random.default_rng(2)
    state = (np.array([4, 0, 7, 1, 0], np.int64), rng.normal(0, 30, (P, D)), rng.uniform(1, 2, (P, D)))
    held = restate_stats(c["obs"], P=P, dtype=np.float64, obs0=c["obs0"], length=c["length"], state=state)
    assert held["count"][2] == 7 and np.array_equal(held["mean"][2], state[1][2]) and np.array_equal(held["m2"][2], state[2][2])
    assert np.array_equal(held["count"], np.where(state[0] > 0, state[0], 0) + held["steps"]) and np.array_equal(held["mean"][1], out["mean"][1])
    # obs0 null: x_k = obs[k]
    knots = restate_stats(c["obs"], P=P, dtype=np.float64, length=c["length"])
    assert not np.array_equal(knots["mean"], out["mean"]) and np.array_equal(knots["steps"][[0, 3, 4]], out["steps"][[0, 3, 4]])
    # length null: every step counts, the values at the last step included
    full = restate_stats(c["obs"], P=P, dtype=np.float32, obs0=c["obs0"])
    assert (full["lane_count"][0] == K).all() and full["valid"][0] < out["valid"][0] + S


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_fold_is_the_whitened_policy(dtype):
    """restate_fold(theta) . [x; 1] against theta . [(x - mu) r; 1] in float64 on observations of the regime: eight times the
    measured distance.  count < 2 gives theta back bit for bit, and std_floor binds on a constant component."""
    P, S, K, D = 3, 5, 40, 10
    (batch,) = _regime(P, S, K, D, 1, seed=5)
    state = _merged([batch.astype(dtype)], P, dtype)
    rng = np.random.default_rng(6)
    theta = rng.normal(0, 0.5, (2 * P, 2, D + 1)).astype(dtype)                      # per lane: two sets a policy
    W = restate_fold(theta, state, dtype=dtype).astype(np.float64)
    count, mean, m2 = (a.astype(np.float64) for a in state)
    r = 1.0 / np.maximum(np.sqrt(m2 / count[:, None]), FLOOR)
    assert (r < 20).all()
    x = batch.astype(dtype).astype(np.float64).reshape(K * S, P, D)
    far, top = 0.0, 0.0
    for q in range(2 * P):
        p = q % P
        th = theta[q].astype(np.float64)
        want = ((x[:, p] - mean[p]) * r[p]) @ th[:, :D].T + th[:, D]
        got = x[:, p] @ W[q][:, :D].T + W[q][:, D]
        far, top = max(far, float(np.abs(got - want).max())), max(top, float(np.abs(want).max()))
    print(f"[norm fold, {dtype.__name__}] worst |d action| / max |action| = {far / top:.3e} (bound {MARGIN * MEASURED_FOLD[dtype]:.3e})")
    assert far / top <= MARGIN * MEASURED_FOLD[dtype] < (1e-11 if dtype is np.float64 else 1e-3)
    # a constant component has the deviation 0: the floor binds, W = theta / std_floor there and nowhere else
    batch[:, :, 1, 4] = 7.25
    flat = _merged([batch.astype(dtype)], P, dtype)
    assert flat[2][1, 4] == 0 and flat[1][1, 4] == dtype(7.25)
    Wf = restate_fold(theta, flat, dtype=dtype)
    assert np.array_equal(Wf[[1, 4], :, 4], theta[[1, 4], :, 4] * (dtype(1) / np.float64(FLOOR).astype(dtype)))
    assert np.array_equal(Wf[[0, 2, 3, 5]], W[[0, 2, 3, 5]].astype(dtype)) and np.abs(Wf[[1, 4]][:, :, [0, 1, 2, 3, 5]] / theta[[1, 4]][:, :, [0, 1, 2, 3, 5]]).max() < 20
    few = (np.array([1, 0, 5], np.int64), state[1], state[2])
    out = restate_fold(theta, few, dtype=dtype)
    assert np.array_equal(out[[0, 1, 3, 4]], theta[[0, 1, 3, 4]]) and not np.array_equal(out[2], theta[2])
    one = restate_fold(theta[:P, :1], state, dtype=dtype)                            # one row: value weights
    assert one.shape == (P, 1, D + 1) and np.array_equal(one, restate_fold(theta, state, dtype=dtype)[:P, :1])


def test_the_unfold_is_the_gradient_through_the_fold():
    """Against torch autograd in float64, through a torch statement of the fold, for a random scalar function of (W, b).  The
    bound: an entry is a product, a difference and a product, each rounded once -- 4 units in the last place of the largest
    intermediate, |g| (1 + |mu|) r."""
    import torch
    P, S, K, D = 3, 5, 40, 10
    (batch,) = _regime(P, S, K, D, 1, seed=7)
    state = _merged([batch], P, np.float64)
    count, mean, m2 = (torch.as_tensor(a, dtype=torch.float64) for a in state)
    r = 1.0 / torch.clamp(torch.sqrt(m2 / count[:, None]), min=FLOOR)
    gen = torch.Generator().manual_seed(8)
    theta = torch.randn(P, 2, D + 1, dtype=torch.float64, generator=gen, requires_grad=True)
    c1, c2 = torch.randn(P, 2, D + 1, dtype=torch.float64, generator=gen), torch.randn(P, 2, D + 1, dtype=torch.float64, generator=gen)
    W = theta[:, :, :D] * r[:, None, :]
    b = theta[:, :, D] - (W * mean[:, None, :]).sum(-1)
    folded = torch.cat([W, b[:, :, None]], dim=2)
    folded.retain_grad()
    f = (c1 * folded).sum() + torch.sin(c2 * folded).sum()
    f.backward()
    assert np.allclose(folded.detach().numpy(), restate_fold(theta.detach().numpy(), state, dtype=np.float64), rtol=1e-12, atol=1e-12)
    g = folded.grad.numpy()
    got = restate_unfold(g, state, dtype=np.float64)
    scale = np.abs(g).max() * (1 + np.abs(state[1]).max()) * float(r.max())
    far = float(np.abs(got - theta.grad.numpy()).max())
    print(f"[norm unfold] worst |d grad| = {far:.3e} (bound {4 * 2.0 ** -52 * scale:.3e})")
    assert far <= 4 * 2.0 ** -52 * scale
    few = (np.array([1, state[0][1], 0], np.int64), state[1], state[2])
    out = restate_unfold(g, few, dtype=np.float64)
    assert np.array_equal(out[[0, 2]], g[[0, 2]]) and np.array_equal(out[1], got[1])


# ---------------------------------------------------------------------------------------
# header, table, exports, resources
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import _lib, control, norm
    protos = _prototypes("os2r_norm.h", "os2rz")
    assert [p[0] for p in protos] == list(norm.ENTRY_POINTS) == NAMES
    lib = norm.load()
    for name, ret, args in protos:
        argtypes = norm.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2rz_last_error" else C.c_int)
    stats, fold, unfold = protos[2][2], protos[3][2], protos[4][2]
    assert stats[:5] == ["const Os2rControlLayout* layout", "int32_t nsteps", "int64_t npolicies", "int32_t nsamples", "uint32_t flags"]
    assert len(stats) == 19 and stats[-3:] == ["void* lane_sum_dev", "int32_t* lane_count_dev", "void* stream"]
    assert fold[:5] == ["const Os2rControlLayout* layout", "int64_t npolicies", "int64_t nlanes", "int32_t rows", "uint32_t flags"]
    assert len(fold) == 12 and fold[8] == "double std_floor" and len(unfold) == 11 and unfold[7] == "double std_floor"
    header = _header("os2r_norm.h")
    assert re.search(r"#define OS2R_NORM_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert len(re.findall(r"#include", header)) == 1
    assert lib.os2rz_abi_version() == norm.ABI_VERSION == 1
    for name, value in (("PER_LANE", 1), ("POLICY_FASTEST", 2), ("CHUNKS", CHUNKS), ("LANE_COUNTS", 2)):
        assert getattr(norm, name) == int(re.search(r"#define OS2RZ_%s (\d+)" % name, header).group(1)) == value, name
    assert norm.Os2rControlLayout is control.Os2rControlLayout and norm.layout is control.layout
    assert not set(norm.ENTRY_POINTS) & (set(_lib.ENTRY_POINTS) | set(_lib.RECORD_ENTRY_POINTS))
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", norm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "libos2r_norm.map")) as f:
        assert re.search(r"global:\s*os2rz_\*;\s*local:\s*\*;", f.read())
    # the header names no other companion library (their tests forbid it) and no other header declares anything of this one
    for word in FORBIDDEN:
        assert word not in header.lower(), word
    flat = " ".join(header.replace("\n *", " ").split())
    assert "adjacent-pair tree" in flat and "in ascending order onto 0" in flat and "no fused multiply-add" in flat
    for line in ("clipping of the whitened observation", "a forgetting factor", "a full covariance", "whitening of rewards or returns",
                 "MLP policies and scheduled policies", "a fit of the value function in whitened coordinates", "the caller swaps two buffers"):
        assert line in flat, line
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "os2r_norm.h":
            assert "os2rz_" not in _header(name).lower() and "os2r_norm.h" not in _header(name).lower(), name
    assert "since built as `libos2r_norm.so`" in " ".join(_header("os2r_es.h").replace("\n *", " ").split())
    # the sum over more than 64 samples of a policy is the score-function library's body, included and not copied; the one over
    # up to 64 is written once, and the header says why
    src = _csrc("os2r_norm.hpp")
    assert '#include "os2r_pg.hpp"' in src and "pg_wave_sum<T>" in src and "__shfl" not in src and "norm_push<T>" in src
    assert "side by side spill" in flat and "included unedited" in flat


KERNELS = ("norm_lane_kernel", "norm_sum_kernel", "norm_sum_few_kernel", "norm_fold_kernel")


def test_kernel_resources():
    """Exactly eight kernels, the four of os2r_norm.hpp in float and double, are in the built library and none uses scratch:
    private_segment_fixed_size 0, no VGPR or SGPR spill and no AGPRs in the code-object metadata.  The lane kernel uses LDS
    for a verdict per thread, the wave sum for the three totals its waves hand over.  The VGPR counts are printed; every kernel stays at four waves a SIMD or more."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import norm
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(norm.LIB_PATH)
    meta = kernel_meta.kernel_meta(norm.LIB_PATH)
    assert len(meta) == 8, sorted(meta)
    for kernel in KERNELS:
        for real in ("float", "double"):
            (name,) = [k for k in meta if f"{kernel}<{real}>" in k]
            m = meta[name]
            print(f"{kernel}<{real}>: {m['vgpr_count']} VGPRs")
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
            assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 128, (name, m)
            lds = {"norm_lane_kernel": (1024,), "norm_sum_kernel": (12, 16)}.get(kernel, (0,))    # the verdicts; B and the two counts
            assert m["group_segment_fixed_size"] in lds, (name, m)


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
    """Every case is refused with OS2R_ERR_INVALID and exactly its text; each cause has a text of its own; nothing is written."""
    seen = set()
    for kw, msg in cases:
        a = dict(good, **kw)
        rc = fn(*[a[k] for k in good], None)
        err = lib.os2rz_last_error()
        assert rc == abi.ERR_INVALID and err == prefix + msg, (list(kw), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases})
    assert not any(buf)
    return seen


def _source_checks(unit_function, seen, helper):
    """The source: no HIP call and every refusal of an argument before the device is asked for, and every text was met."""
    src = _csrc("os2r_norm_capi.hip")
    body = _function(src, "int " + unit_function)
    first_hip = min(body.index(t) for t in ("check_device(", "fold_launch(") if t in body)
    assert not re.search(HIP_CALL, body[:first_hip])
    fails = [m.start() for m in re.finditer(r"fail\(OS2R_ERR_INVALID", body)]
    assert fails and all(i < first_hip for i in fails)
    texts = re.findall(r'fail\(OS2R_ERR_INVALID, "([^"]+)"', body) + re.findall(r'return "([^"]+)";', _function(src, r"const char\* " + helper))
    assert len(texts) == len(set(texts)) and all(any(t.encode() in e for e in seen) for t in texts), [t for t in texts if not any(t.encode() in e for e in seen)]
    launch = _function(src, "int fold_launch")
    assert launch.index("check_device(") < launch.index("DeviceGuard") < launch.index("auto launch") and "fail(" not in launch


def test_obs_stats_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import norm
    lib = norm.load()
    Lay = _layouts()
    K, P, S, D = 3, 2, 3, 4
    N = S * P
    buf = (C.c_double * 4096)()
    base = C.addressof(buf)
    at = lambda i: C.c_void_p(base + 8 * i)
    size = dict(obs=K * N * D, obs0=N * D, length=N, count_in=P, mean_in=P * D, m2_in=P * D, count_out=P, mean_out=P * D, m2_out=P * D, steps=P,
                valid=P, lane_sum=2 * D * N, lane_count=2 * N)
    where, nxt = {}, 0
    for name, n in size.items():
        where[name] = nxt
        nxt += n
    assert nxt < 4000
    good = dict(lay=Lay(), K=K, P=P, S=S, flags=0, **{k: at(where[k]) for k in size})
    name = "os2rz_obs_stats"
    assert len(good) + 1 == len(norm.ENTRY_POINTS[name]) == 19
    assert lib.os2rz_obs_stats(*[None if _is_pointer(t) else 0 for t in norm.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rz_last_error() == b"os2rz_obs_stats: null layout"
    end = lambda n: where[n] + size[n] - 1
    part = b"count_in_dev, mean_in_dev and m2_in_dev must be all null or all given"
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"layout->dtype must be OS2R_F32 or OS2R_F64"),
             (dict(lay=Lay(nq=1)), b"layout->nq must be 2..5"), (dict(lay=Lay(obs_dim=0)), b"layout->obs_dim must be 1..12"),
             (dict(lay=Lay(obs_dim=13)), b"layout->obs_dim must be 1..12"),
             (dict(K=0), b"nsteps must be >= 1"), (dict(K=65536), b"nsteps must be <= 65535"), (dict(P=0), b"npolicies must be >= 1"),
             (dict(S=0), b"nsamples must be >= 1"), (dict(S=-2), b"nsamples must be >= 1"),
             (dict(P=2 ** 31, S=1), b"nsamples * npolicies exceeds 2^31 - 1"), (dict(P=2 ** 40), b"nsamples * npolicies exceeds 2^31 - 1"),
             (dict(S=2 ** 16, K=2 ** 15, P=1), b"nsamples * nsteps exceeds 2^31 - 1 (the steps of a policy are an int32)"),
             (dict(flags=1), b"unknown flag bits"), (dict(flags=0x80000000), b"unknown flag bits"),
             (dict(obs=None), b"null obs_dev"),
             (dict(count_in=None), part), (dict(mean_in=None), part), (dict(m2_in=None, count_in=None), part),
             (dict(count_out=None), b"null count_out_dev"), (dict(mean_out=None), b"null mean_out_dev"), (dict(m2_out=None), b"null m2_out_dev"),
             (dict(lane_sum=None), b"null lane_sum_dev (the second launch reads it)"),
             (dict(lane_count=None), b"null lane_count_dev (the second launch reads it)"),
             # an output over an input, from both sides; over another output; the optional ones too
             (dict(count_out=at(where["count_in"])), b"count_out_dev overlaps count_in_dev"),
             (dict(mean_out=at(end("mean_in"))), b"mean_out_dev overlaps mean_in_dev"), (dict(m2_out=at(where["m2_in"])), b"m2_out_dev overlaps m2_in_dev"),
             (dict(mean_out=at(end("obs"))), b"mean_out_dev overlaps obs_dev"), (dict(m2_out=at(where["obs0"])), b"m2_out_dev overlaps obs0_dev"),
             (dict(steps=at(where["length"])), b"steps_dev overlaps length_dev"), (dict(valid=at(where["steps"])), b"valid_dev overlaps steps_dev"),
             (dict(lane_sum=at(end("m2_out"))), b"lane_sum_dev overlaps m2_out_dev"), (dict(lane_count=at(end("lane_sum"))), b"lane_count_dev overlaps lane_sum_dev"),
             (dict(lane_count=at(where["count_out"])), b"lane_count_dev overlaps count_out_dev")]
    seen = _refused(lib, lib.os2rz_obs_stats, b"os2rz_obs_stats: ", good, cases, buf)
    # the edges are taken: nothing is left to refuse but the device, and no call is let through to one
    edges = [dict(K=65535, S=1, obs=C.c_void_p(2 ** 44)), dict(obs0=None), dict(length=None), dict(count_in=None, mean_in=None, m2_in=None), dict(steps=None, valid=None),
             dict(lay=Lay(abi.F32, device=1000)), dict(lane_count=at(where["lane_count"] + 1), steps=None, valid=None)]
    for kw in edges:                                  # (device 1000 is never there, with a GPU or without)
        a = dict(good, **dict(dict(lay=Lay(device=1000)), **kw))
        assert lib.os2rz_obs_stats(*[a[k] for k in good], None) == abi.ERR_NO_DEVICE and lib.os2rz_last_error().startswith(b"os2rz_obs_stats: "), kw
    assert not any(buf)
    _source_checks(name, seen, "shape_refusal")


def test_fold_and_unfold_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import norm
    lib = norm.load()
    Lay = _layouts()
    P, L, D = 2, 6, 4
    buf = (C.c_double * 4096)()
    base = C.addressof(buf)
    at = lambda i: C.c_void_p(base + 8 * i)
    nan, inf = float("nan"), float("inf")
    size = dict(count=P, mean=P * D, m2=P * D, theta=L * 2 * (D + 1), weights=L * 2 * (D + 1))
    where, nxt = {}, 0
    for name, n in size.items():
        where[name] = nxt
        nxt += n
    end = lambda n: where[n] + size[n] - 1
    part = b"count_dev, mean_dev and m2_dev must be all null or all given"
    common = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=7)), b"layout->dtype must be OS2R_F32 or OS2R_F64"),
              (dict(lay=Lay(nq=6)), b"layout->nq must be 2..5"), (dict(lay=Lay(obs_dim=0)), b"layout->obs_dim must be 1..12"),
              (dict(P=0), b"npolicies must be >= 1"), (dict(P=-1), b"npolicies must be >= 1"), (dict(P=2 ** 31), b"npolicies exceeds 2^31 - 1"),
              (dict(rows=0), b"rows must be 1 or 2"), (dict(rows=3), b"rows must be 1 or 2"),
              (dict(floor=nan), b"std_floor must be finite"), (dict(floor=inf), b"std_floor must be finite"), (dict(floor=0.0), b"std_floor must be > 0"),
              (dict(floor=-1e-6), b"std_floor must be > 0"), (dict(lay=Lay(abi.F32), floor=1e-60), b"std_floor rounds to 0 in the layout's dtype"),
              (dict(count=None), part), (dict(mean=None, m2=None), part), (dict(m2=None), part)]
    good = dict(lay=Lay(), P=P, L=L, rows=2, flags=norm.PER_LANE, **{k: at(where[k]) for k in ("count", "mean", "m2")}, floor=FLOOR,
                theta=at(where["theta"]), weights=at(where["weights"]))
    name = "os2rz_fold"
    assert len(good) + 1 == len(norm.ENTRY_POINTS[name]) == 12
    assert lib.os2rz_fold(*[None if _is_pointer(t) else 0 for t in norm.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rz_last_error() == b"os2rz_fold: null layout"
    cases = common + [(dict(flags=4), b"unknown flag bits"), (dict(flags=0x80000001), b"unknown flag bits"),
                      (dict(L=0), b"nlanes must be >= 1 with OS2RZ_PER_LANE"), (dict(L=2 ** 31), b"nlanes exceeds 2^31 - 1"),
                      (dict(L=5), b"nlanes must be a multiple of npolicies (lane l is under policy l mod npolicies)"),
                      (dict(theta=None), b"null theta_dev"), (dict(weights=None), b"null weights_dev"),
                      (dict(weights=at(end("theta"))), b"weights_dev overlaps theta_dev"), (dict(theta=at(end("weights"))), b"weights_dev overlaps theta_dev"),
                      (dict(weights=at(where["count"])), b"weights_dev overlaps count_dev"), (dict(weights=at(end("mean"))), b"weights_dev overlaps mean_dev"),
                      (dict(weights=at(where["m2"])), b"weights_dev overlaps m2_dev")]
    seen = _refused(lib, lib.os2rz_fold, b"os2rz_fold: ", good, cases, buf)
    edges = [dict(), dict(flags=0, L=-5), dict(flags=norm.POLICY_FASTEST, L=0), dict(flags=3, rows=1), dict(count=None, mean=None, m2=None),
             dict(floor=5e-324), dict(lay=Lay(abi.F32, device=1000), floor=1e-45), dict(flags=0, weights=at(where["theta"] + P * 2 * (D + 1)))]
    for kw in edges:
        a = dict(good, **dict(dict(lay=Lay(device=1000)), **kw))
        assert lib.os2rz_fold(*[a[k] for k in good], None) == abi.ERR_NO_DEVICE and lib.os2rz_last_error().startswith(b"os2rz_fold: "), kw
    assert not any(buf)
    _source_checks(name, seen, "sets_refusal")

    good = dict(lay=Lay(), P=P, rows=2, flags=norm.POLICY_FASTEST, **{k: at(where[k]) for k in ("count", "mean", "m2")}, floor=FLOOR,
                grad=at(where["theta"]), grad_theta=at(where["weights"]))
    name = "os2rz_unfold"
    assert len(good) + 1 == len(norm.ENTRY_POINTS[name]) == 11
    assert lib.os2rz_unfold(*[None if _is_pointer(t) else 0 for t in norm.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rz_last_error() == b"os2rz_unfold: null layout"
    cases = common + [(dict(flags=1), b"OS2RZ_PER_LANE is os2rz_fold's (a gradient is per policy)"), (dict(flags=3), b"OS2RZ_PER_LANE is os2rz_fold's (a gradient is per policy)"),
                      (dict(flags=4), b"unknown flag bits"), (dict(grad=None), b"null grad_dev"), (dict(grad_theta=None), b"null grad_theta_dev"),
                      (dict(grad_theta=at(where["theta"] + P * 2 * (D + 1) - 1)), b"grad_theta_dev overlaps grad_dev"),
                      (dict(grad_theta=at(end("count"))), b"grad_theta_dev overlaps count_dev"), (dict(grad_theta=at(where["mean"])), b"grad_theta_dev overlaps mean_dev"),
                      (dict(grad_theta=at(end("m2"))), b"grad_theta_dev overlaps m2_dev")]
    seen = _refused(lib, lib.os2rz_unfold, b"os2rz_unfold: ", good, cases, buf)
    edges = [dict(), dict(flags=0, rows=1), dict(count=None, mean=None, m2=None), dict(grad_theta=at(where["theta"] + P * 2 * (D + 1)))]
    for kw in edges:
        a = dict(good, **dict(dict(lay=Lay(device=1000)), **kw))
        assert lib.os2rz_unfold(*[a[k] for k in good], None) == abi.ERR_NO_DEVICE and lib.os2rz_last_error().startswith(b"os2rz_unfold: "), kw
    assert not any(buf)
    _source_checks(name, seen, "sets_refusal")


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
    from gym_os2r_amd import norm
    from gym_os2r_amd.sim import HipSim
    for method in ("obs_stats", "obs_stats_into", "norm_fold", "norm_fold_into", "norm_unfold", "norm_unfold_into"):
        assert callable(getattr(HipSim, method))
    assert "Chan's" in HipSim.obs_stats.__doc__ and "invariant" in HipSim.norm_unfold.__doc__

    def no_load():
        raise AssertionError("a refused call reached norm.load")
    monkeypatch.setattr(norm, "load", no_load)
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    s = _bare(f64)
    K, P, S, D = 3, 2, 3, 4
    N = S * P
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    obs, obs0, length = z(K, N, D), z(N, D), z(N, dtype=i32)
    state = (z(P, dtype=i64), z(P, D), z(P, D))
    outs = (z(P, dtype=i64), z(P, D), z(P, D), z(2 * D, N), z(2, N, dtype=i32))

    def stats_into(*args, **kw):
        with pytest.raises(ValueError, match="^obs_stats: "):
            s.obs_stats_into(*args, **dict(dict(policies=P), **kw))

    def stats(*args, **kw):
        with pytest.raises(ValueError, match="^obs_stats: "):
            s.obs_stats(*args, **dict(dict(policies=P), **kw))
    for kw in (dict(policies=0), dict(policies=True), dict(policies=2.0), dict(policies=4), dict(obs0=z(N, D + 1)), dict(obs0=obs0.float()),
               dict(length=z(N, dtype=i64)), dict(length=z(N + 1, dtype=i32)), dict(state=(state[0],)), dict(state="x"), dict(state=(state[0].int(), state[1], state[2])),
               dict(state=(state[0], state[1], None)), dict(state=(z(P + 1, dtype=i64), state[1], state[2])), dict(state=(state[0], z(P, D + 1), state[2])),
               dict(state=(state[0], state[1].to("meta"), state[2]))):
        stats_into(obs, *outs, **kw)
        stats(obs, **kw)
    for bad in (None, z(K, N), z(K, N, D + 1), obs.float(), obs.numpy(), z(0, N, D)):
        stats_into(bad, *outs)
        stats(bad)
    swap = lambda i, t: tuple(t if j == i else a for j, a in enumerate(outs))
    for args in (swap(0, None), swap(0, z(P, dtype=i32)), swap(1, z(P, D + 1)), swap(2, None), swap(2, z(P, D).float()), swap(3, z(2 * D, N + 1)),
                 swap(3, None), swap(4, z(2, N)), swap(4, z(3, N, dtype=i32)), swap(1, outs[2]), swap(1, z(D, P).t())):
        stats_into(obs, *args)
    stats_into(obs, *outs, steps=z(P))
    stats_into(obs, *outs, valid=z(P + 1, dtype=i32))
    stats_into(obs, *outs, state=(outs[0], state[1], state[2]))                      # an output over an input: the caller swaps
    stats_into(obs, *outs, state=(state[0], outs[1], state[2]))

    theta, weights = z(P, 2, D + 1), z(P, 2, D + 1)
    lanes, lw = z(N, 2, D + 1), z(N, 2, D + 1)

    def fold_into(*args, **kw):
        with pytest.raises(ValueError, match="^norm_fold: "):
            s.norm_fold_into(*args, **kw)

    def fold(*args, **kw):
        with pytest.raises(ValueError, match="^norm_fold: "):
            s.norm_fold(*args, **kw)

    def unfold_into(*args, **kw):
        with pytest.raises(ValueError, match="^norm_unfold: "):
            s.norm_unfold_into(*args, **kw)

    def unfold(*args, **kw):
        with pytest.raises(ValueError, match="^norm_unfold: "):
            s.norm_unfold(*args, **kw)
    for bad in (float("nan"), float("inf"), 0.0, -1e-6, "x", None, True):
        fold_into(theta, state, weights, std_floor=bad)
        fold(theta, state, std_floor=bad)
        unfold_into(theta, state, weights, std_floor=bad)
        unfold(theta, state, std_floor=bad)
    for bad in (None, "x", (state[0],), (state[0].int(), state[1], state[2]), (state[0], state[1].float(), state[2]), (state[0], state[1], z(P, D + 1)),
                (z(P, 1, dtype=i64), state[1], state[2])):
        fold_into(theta, bad, weights)
        fold(theta, bad)
        unfold_into(theta, bad, weights)
        unfold(theta, bad)
    for bad in (None, z(P, 3, D + 1), z(P, 2, D), z(P + 1, 2, D + 1), theta.float(), theta.numpy(), z(2, D + 1, P).permute(2, 0, 1)):
        fold_into(bad, state, weights)
        unfold_into(bad, state, weights)
    for bad in (None, z(P, 3, D + 1), z(P, 2, D), z(P + 1, 2, D + 1), theta.float(), theta.to("meta"), z(P), "x"):
        fold(bad, state)
        unfold(bad, state)
    for bad in (None, z(P, 1, D + 1), weights.float(), theta, z(2, D + 1, P)):
        fold_into(theta, state, bad)
        unfold_into(theta, state, bad)
    fold_into(z(2, D + 1, P), state, weights, policy_fastest=True)                  # both arrays in the one layout
    fold_into(theta, state, weights, policy_fastest=True)
    for bad in (0, -N, True, 2.0, N + 1):
        fold_into(lanes, state, lw, lanes=bad)
        fold(lanes, state, lanes=bad)
    fold_into(theta, state, weights, lanes=N)                                        # N sets, not P
    fold(theta, state, lanes=N)
    fold(lanes, state)
    f32 = _bare(torch.float32)
    with pytest.raises(ValueError, match="^norm_fold: std_floor"):
        f32.norm_fold_into(theta.float(), (state[0], state[1].float(), state[2].float()), weights.float(), std_floor=1e-60)
    # what passes every check reaches the loader, and only then (the bare handle has no cfg to fill a layout from)
    with pytest.raises(AttributeError):
        s.obs_stats_into(obs, *outs, policies=P, obs0=obs0, length=length, state=state, steps=z(P, dtype=i32), valid=z(P, dtype=i32))
    with pytest.raises(AttributeError):
        s.obs_stats_into(obs, *outs, policies=P)
    with pytest.raises(AttributeError):
        s.norm_fold_into(lanes, state, lw, lanes=N)
    with pytest.raises(AttributeError):
        s.norm_fold_into(z(1, D + 1, P), state, z(1, D + 1, P), policy_fastest=True)
    with pytest.raises(AttributeError):
        s.norm_unfold_into(z(2, D + 1, P), state, z(2, D + 1, P), policy_fastest=True)
    with pytest.raises(AttributeError):
        s.norm_fold(z(D + 1, P).t(), state)                                          # value weights as value_fit returns them
    with pytest.raises(AttributeError):
        s.norm_unfold(z(2, D + 1, P).permute(2, 0, 1), state)
