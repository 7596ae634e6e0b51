"""libos2r_pg.so (include/os2r_pg.h): the host side -- the numpy restatement of the policy gradient the GPU tests compare with
(`restate_pg`) against the textbook statement in float64 (the einsum of examples/reinforce_balancing.py, and a reverse loop for
the reward-to-go), the crafted inputs of the GPU tests (`crafted_pg`), the header against the one table of gym_os2r_amd/pg.py, the
exports of the library, the other libraries as they were, the resources of the six kernels in the built library, every refusal
of os2rg_policy_gradient through ctypes without a device, and the argument checks of HipSim.policy_gradient that need no device.
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
from header_check import HIP_CALL, _agrees, _csrc, _function, _header, _is_pointer, _prototypes  # noqa: E402

NAMES = ["os2rg_abi_version", "os2rg_last_error", "os2rg_policy_gradient"]
CHUNKS = 64
# K, P, S, D of the GPU tests (tests/test_gpu_pg.py): the smallest case; a partial with two terms beside partials with one;
# policies across a wave boundary and the largest D; several terms per partial with one policy; S = 1, the per-environment layout
SHAPES = [(1, 1, 1, 1), (7, 3, 65, 10), (5, 65, 2, 12), (33, 1, 200, 10), (4, 130, 1, 10)]
NONE_VALID = 2                          # the policy none of whose lanes is valid (where P > 2)
# The largest relative distance (the largest difference over the largest entry of the textbook result) of the restatement from
# the textbook statement in float64 over TEXTBOOK_SHAPES, measured on the CPU this test was written on
# (test_the_restatement_is_the_textbook_gradient prints them): the bound is 100 x that, the margin of tests/test_cem_host.py.
MEASURED = {np.float64: dict(grad=3.247e-15, lsig=1.856e-15, grad_rtg=2.151e-15, lsig_rtg=3.678e-15),
            np.float32: dict(grad=1.859e-7, lsig=8.565e-8, grad_rtg=2.240e-7, lsig_rtg=4.123e-7)}
MARGIN = 100
TEXTBOOK_SHAPES = [(7, 3, 65, 10), (33, 1, 200, 10), (50, 2, 300, 10)]


# ---------------------------------------------------------------------------------------
# the restatement of include/os2r_pg.h (needs no device)
# ---------------------------------------------------------------------------------------
def chunked_sum(x, fine):
    """Step 5: the sum of x [..., S, P] over the valid samples (fine [S, P] bool) in 64 partials, partial c adding its samples
    s = c, c + 64, ... in ascending order onto 0, then the adjacent-pair tree."""
    S = x.shape[-2]
    parts = []
    for c in range(CHUNKS):
        acc = np.zeros(x.shape[:-2] + x.shape[-1:], x.dtype)
        for s in range(c, S, CHUNKS):
            acc = np.where(fine[s], acc + x[..., s, :], acc)
        parts.append(acc)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
    return parts[0]


def restate_pg(obs, noise, sigma, *, P, dtype, obs0=None, action=None, tanh=False, length=None, adv=None, reward=None, done=None,
               gamma=1.0, baseline=None):
    """include/os2r_pg.h, steps 1-5, in numpy and in `dtype`.  obs [K, N, D], noise and action [K, N, 2], sigma [2] or [2, N].
    -> dict(grad [2, D+1, P], lane_grad [2, D+1, N], lsig_grad [2, P], lane_lsig [2, N], steps [P], clipped [2, P], valid [P],
    rtg [K, N] (zeros with adv), lane_count [4, N])."""
    f = lambda a: None if a is None else np.asarray(a).astype(dtype)
    obs, obs0, noise, action, adv, reward, baseline = (f(a) for a in (obs, obs0, noise, action, adv, reward, baseline))
    K, N, D = obs.shape
    S = N // P
    sig = np.broadcast_to(f(sigma).reshape(2, -1), (2, N))
    g = np.float64(gamma).astype(dtype)                                        # rounded once
    ln = np.full(N, K, np.int64) if length is None else np.clip(np.asarray(length, np.int64), 0, K)
    pol = np.arange(N) % P
    one = dtype(1)
    L, V, clip = np.zeros((2, D + 1, N), dtype), np.zeros((2, N), dtype), np.zeros((2, N), np.int32)
    G, rtg = np.zeros(N, dtype), np.zeros((K, N), dtype)
    with np.errstate(all="ignore"):
        sig_open = sig > 0                                                     # (a NaN is not)
        for k in range(K - 1, -1, -1):
            counted = k < ln
            if reward is not None:                                             # step 1
                G = np.where(counted, np.where(np.asarray(done[k]) != 0, reward[k], reward[k] + g * G), G)
                psi = G if baseline is None else G - baseline[k][pol]
                rtg[k] = np.where(counted, G, 0)
            else:
                psi = adv
            x = obs[k] if obs0 is None else (obs0 if k == 0 else obs[k - 1])
            for j in range(2):
                inside = np.ones(N, bool) if tanh else np.abs(action[k, :, j]) < 1   # step 2 (a NaN is not)
                clip[j] += counted & ~inside
                opened = counted & sig_open[j] & inside
                eps = noise[k, :, j]
                e = eps / sig[j]                                               # step 3
                c = psi * e
                for d in range(D):
                    L[j, d] = np.where(opened, L[j, d] + c * x[:, d], L[j, d])
                L[j, D] = np.where(opened, L[j, D] + c, L[j, D])
                V[j] = np.where(opened, V[j] + psi * (eps * eps - one), V[j])
        fine = np.isfinite(L).all((0, 1)) & np.isfinite(V).all(0)              # step 4
        shaped = fine.reshape(S, P)
        grad = chunked_sum(L.reshape(2, D + 1, S, P), shaped)                  # step 5
        lsig = chunked_sum(V.reshape(2, S, P), shaped)
    count = np.stack([ln.astype(np.int32), clip[0], clip[1], fine.astype(np.int32)])
    steps, clip0, clip1, valid = (chunked_sum(row.reshape(S, P), shaped) for row in count)
    assert all(a.dtype == dtype for a in (L, V, grad, lsig, rtg)) and all(a.dtype == np.int32 for a in (steps, clip0, valid))
    return dict(grad=grad, lane_grad=L, lsig_grad=lsig, lane_lsig=V, steps=steps, clipped=np.stack([clip0, clip1]), valid=valid, rtg=rtg,
                lane_count=count)


def textbook_pg(obs0, O, A, E, sigma, done, adv, P):
    """The five statements of examples/reinforce_balancing.py in float64, the policy as a batch dimension: the observation record
    shifted by one, the mask from a cumsum, the coefficient tensor, the einsum and the sum for the bias; beside them the
    gradient with respect to log sigma.  -> (grad [2, D+1, P], lsig [2, P])"""
    K, N, D = O.shape
    S = N // P
    prev = np.concatenate([obs0[None], O[:-1]])
    ended = (done != 0).astype(np.int64)
    alive = ((np.cumsum(ended, 0) - ended) == 0).astype(np.float64)
    inside = (np.abs(A) < 1.0).astype(np.float64)
    coef = inside * E / sigma * (alive * adv[None])[..., None]
    coef_p, prev_p = coef.reshape(K, S, P, 2), prev.reshape(K, S, P, D)
    grad = np.concatenate([np.einsum("kspj,kspd->jdp", coef_p, prev_p), coef_p.sum((0, 1)).T[:, None, :]], 1)
    lsig = (inside * (E * E - 1.0) * (alive * adv[None])[..., None]).reshape(K, S, P, 2).sum((0, 1)).T
    return grad, lsig


def textbook_rtg(obs0, O, A, E, sigma, done, length, reward, gamma, baseline, P):
    """The reward-to-go form in float64: a reverse loop for G, the rest as above.  -> (grad, lsig)"""
    K, N, D = O.shape
    S = N // P
    prev = np.concatenate([obs0[None], O[:-1]])
    counted = (np.arange(K)[:, None] < length[None]).astype(np.float64)
    G, psi = np.zeros(N), np.zeros((K, N))
    for k in range(K - 1, -1, -1):
        G = np.where(counted[k] > 0, np.where(done[k] != 0, reward[k], reward[k] + gamma * G), G)
        psi[k] = G - baseline[k][np.arange(N) % P]
    inside = (np.abs(A) < 1.0).astype(np.float64)
    w = (counted * psi)[..., None] * inside
    coef = (w * E / sigma).reshape(K, S, P, 2)
    grad = np.concatenate([np.einsum("kspj,kspd->jdp", coef, prev.reshape(K, S, P, D)), coef.sum((0, 1)).T[:, None, :]], 1)
    return grad, (w * (E * E - 1.0)).reshape(K, S, P, 2).sum((0, 1)).T


def plain_pg(K, P, S, D, dtype, seed=0):
    """A rollout as the example sees one, rounded to `dtype` and returned in float64: no lane is invalid, done ends the episode
    and length is what the rollout would report."""
    rng = np.random.default_rng(seed)
    N = S * P
    r = lambda a: a.astype(dtype).astype(np.float64)
    done = (rng.uniform(size=(K, N)) < 0.05).astype(np.uint8)
    first = np.where(done.any(0), done.argmax(0) + 1, K).astype(np.int32)
    A = np.clip(rng.normal(0.0, 0.7, (K, N, 2)), -1.0, 1.0)
    return dict(obs0=r(rng.normal(0, 1, (N, D))), obs=r(rng.normal(0, 1, (K, N, D))), action=r(A), noise=r(rng.normal(0, 1, (K, N, 2))),
                sigma=r(np.array([0.2, 0.3])), done=done, length=first, adv=r(rng.normal(0, 1, N)), reward=r(rng.uniform(0, 1, (K, N))),
                baseline=r(rng.uniform(0, 3, (K, P))))


def _far(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_is_the_textbook_gradient(dtype):
    """grad and lsig_grad within MARGIN x the distance measured when this was written: against the example's einsum statement
    fp64 3.2e-15 and 1.9e-15, fp32 1.9e-7 and 8.6e-8; with the reward-to-go against a float64 reverse loop fp64 2.2e-15 and
    3.7e-15, fp32 2.2e-7 and 4.1e-7 (relative to the largest entry).  steps, clipped and valid agree exactly."""
    worst = dict(grad=0.0, lsig=0.0, grad_rtg=0.0, lsig_rtg=0.0)
    for K, P, S, D in TEXTBOOK_SHAPES:
        c = plain_pg(K, P, S, D, dtype)
        common = dict(P=P, dtype=dtype, obs0=c["obs0"], action=c["action"], length=c["length"])
        got = restate_pg(c["obs"], c["noise"], c["sigma"], adv=c["adv"], **common)
        assert got["valid"].tolist() == [S] * P and np.isfinite(got["grad"]).all()
        assert np.array_equal(got["steps"], c["length"].reshape(S, P).sum(0))
        assert np.array_equal(got["clipped"].T, ((np.abs(c["action"]) >= 1) & (np.arange(K)[:, None, None] < c["length"][None, :, None]))
                              .reshape(K, S, P, 2).sum((0, 1)))
        grad, lsig = textbook_pg(c["obs0"], c["obs"], c["action"], c["noise"], c["sigma"], c["done"], c["adv"], P)
        worst["grad"], worst["lsig"] = max(worst["grad"], _far(got["grad"], grad)), max(worst["lsig"], _far(got["lsig_grad"], lsig))
        gamma = float(dtype(0.97))
        got = restate_pg(c["obs"], c["noise"], c["sigma"], reward=c["reward"], done=c["done"], gamma=gamma, baseline=c["baseline"], **common)
        assert got["valid"].tolist() == [S] * P
        grad, lsig = textbook_rtg(c["obs0"], c["obs"], c["action"], c["noise"], c["sigma"], c["done"], c["length"], c["reward"], gamma,
                                  c["baseline"], P)
        worst["grad_rtg"], worst["lsig_rtg"] = max(worst["grad_rtg"], _far(got["grad"], grad)), max(worst["lsig_rtg"], _far(got["lsig_grad"], lsig))
    print(f"restate_pg against the textbook, {dtype.__name__}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for name, value in worst.items():
        assert value <= MARGIN * MEASURED[dtype][name], (name, value)


def crafted_pg(K, P, S, D, dtype, seed=0):
    """The inputs of the GPU tests, in `dtype`.  By lane l = s P + p (where the shape reaches it):
      l % 11 == 1, 2, 3, 4   length 0, K, -3 and K + 5
      l % 7 == 6             NaNs in obs, noise, action and reward at every step k >= len: they change nothing
      l % 5 == 0             actions of exactly +1 and -1 and the nearest values below 1 in magnitude, in turn over the steps
      l % 9 == 1, 3          in the per-lane sigma, component 0 is 0, component 1 is NaN
      s % 8 == 5 (S >= 6)    an invalid lane: a NaN reward at step 0 and an infinite adv, the length K, the components open
      p == 2 (P > 2)         the same in every lane of the policy: none of its lanes is valid
    done bytes (any non-zero value) fall in mid-window with probability 0.1.
    -> dict(obs, obs0, noise, action, sigma [2], lane_sigma [2, N], length, adv, reward, done, baseline)"""
    rng = np.random.default_rng(seed)
    N = S * P
    l = np.arange(N)
    s, p = l // P, l % P
    obs, obs0 = rng.normal(0, 1, (K, N, D)), rng.normal(0, 1, (N, D))
    noise = rng.normal(0, 1, (K, N, 2))
    action = np.clip(rng.normal(0, 0.7, (K, N, 2)), -1, 1).astype(dtype)
    below = np.nextafter(dtype(1), dtype(0))
    edge = np.array([1, -1, below, -below], dtype)
    action[:, l % 5 == 0, :] = edge[np.arange(K) % 4][:, None, None]
    lane_sigma = rng.uniform(0.1, 0.4, (2, N))
    lane_sigma[0, l % 9 == 1], lane_sigma[1, l % 9 == 3] = 0.0, np.nan
    length = rng.integers(1, K + 1, N).astype(np.int32)
    for rest, value in ((1, 0), (2, K), (3, -3), (4, K + 5)):
        length[l % 11 == rest] = value
    adv, reward = rng.normal(0, 1, N), rng.uniform(0, 1, (K, N))
    done = (rng.uniform(size=(K, N)) < 0.1) * rng.integers(1, 256, (K, N))
    broken = ((s % 8 == 5) & (S >= 6)) | ((p == NONE_VALID) & (P > 2))
    length[broken] = K
    adv[broken], reward[0, broken] = np.inf, np.nan
    action[0, broken, :] = 0.5
    lane_sigma[:, broken] = 0.25
    beyond = (np.arange(K)[:, None] >= np.clip(length, 0, K)[None]) & (l % 7 == 6)[None]
    obs[beyond], noise[beyond], action[beyond], reward[beyond] = np.nan, np.nan, np.nan, np.nan
    f = lambda a: np.ascontiguousarray(a.astype(dtype))
    return dict(obs=f(obs), obs0=f(obs0), noise=f(noise), action=f(action), sigma=f(np.array([0.3, 0.25])), lane_sigma=f(lane_sigma),
                length=length, adv=f(adv), reward=f(reward), done=np.ascontiguousarray(done.astype(np.uint8)),
                baseline=f(rng.uniform(0, 2, (K, P))))


def at_most_a_quarter_invalid(out, P, S):
    """Of the restatement `out`: the policy NONE_VALID (P > 2) has no valid lane and zeros for sums; of every other policy at most
    a quarter of the lanes is invalid."""
    fine = out["lane_count"][3].reshape(S, P)
    for p in range(P):
        if P > 2 and p == NONE_VALID:
            assert fine[:, p].sum() == 0 == out["valid"][p] == out["steps"][p] and (out["clipped"][:, p] == 0).all()
            assert (out["grad"][:, :, p] == 0).all() and (out["lsig_grad"][:, p] == 0).all()
        else:
            assert 4 * (S - fine[:, p].sum()) <= S and out["valid"][p] == fine[:, p].sum(), (p, S, fine[:, p].sum())
    return True


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_on_crafted_inputs_that_reach_every_branch(dtype):
    from gym_os2r_amd import pg
    assert CHUNKS == pg.CHUNKS == int(re.search(r"#define OS2RG_CHUNKS (\d+)", _header("os2r_pg.h")).group(1))
    K, P, S, D = 7, 3, 65, 10
    c = crafted_pg(K, P, S, D, dtype)
    N, l = S * P, np.arange(S * P)
    common = dict(P=P, dtype=dtype, obs0=c["obs0"], action=c["action"], length=c["length"])
    adv = restate_pg(c["obs"], c["noise"], c["lane_sigma"], adv=c["adv"], **common)
    rtg = restate_pg(c["obs"], c["noise"], c["lane_sigma"], reward=c["reward"], done=c["done"], gamma=0.97, baseline=c["baseline"], **common)
    for out in (adv, rtg):
        assert at_most_a_quarter_invalid(out, P, S)
        ln, clip0, clip1, fine = out["lane_count"]
        # the four lengths; a lane of length 0 has zeros for sums and is valid
        assert set(c["length"][[1, 2, 3, 4]]) == {0, K, -3, K + 5} and ln[1] == 0 == ln[3] and ln[2] == K == ln[4]
        assert (out["lane_grad"][:, :, 1] == 0).all() and fine[1] == 1
        # the broken lanes: not finite, not valid, left out of steps and clipped
        broken = ~fine.astype(bool)
        assert broken.sum() == S + (S // 8) * (P - 1) and not np.isfinite(out["lane_grad"][:, :, broken]).all()
        assert np.array_equal(out["steps"], np.where(broken, 0, ln).reshape(S, P).sum(0))
        assert np.array_equal(out["clipped"][0], np.where(broken, 0, clip0).reshape(S, P).sum(0))
        # NaNs beyond len change nothing: every lane that holds some is valid (unless broken), its sums are finite
        held = (l % 7 == 6) & (np.clip(c["length"], 0, K) < K)
        assert held.any() and np.isnan(c["obs"][-1, held]).all() and np.isfinite(out["lane_grad"][:, :, held & ~broken]).all()
        # actions of exactly +-1 are clipped, the nearest values below are not
        five = np.flatnonzero((l % 5 == 0) & ~broken & (ln == K))[0]
        assert clip0[five] == clip1[five] == len([k for k in range(K) if k % 4 < 2]) and (np.abs(c["action"][2, five]) < 1).all()
        # sigma 0 and NaN: the row of that motor is 0, the other is not
        zero, nan = np.flatnonzero((l % 9 == 1) & ~broken & (ln > 1))[0], np.flatnonzero((l % 9 == 3) & ~broken & (ln > 1))[0]
        assert (out["lane_grad"][0, :, zero] == 0).all() and (out["lane_grad"][1, :, zero] != 0).any() and out["lane_lsig"][0, zero] == 0
        assert (out["lane_grad"][1, :, nan] == 0).all() and (out["lane_grad"][0, :, nan] != 0).any() and fine[nan] == 1
        # a partial with two terms (s = 0 and 64) beside partials with one
        assert S == CHUNKS + 1
    # the reward-to-go: cut by a done byte in mid-window, 0 behind len, gamma = 0 leaves the rewards
    K2 = np.clip(c["length"], 0, K)
    mid = np.argwhere((c["done"][1:K - 1] != 0) & (K2[None] == K) & np.isfinite(c["reward"]).all(0)[None])[0]
    k, lane = mid[0] + 1, mid[1]
    assert rtg["rtg"][k, lane] == c["reward"][k, lane] and rtg["rtg"][k - 1, lane] != c["reward"][k - 1, lane]
    assert (rtg["rtg"][np.arange(K)[:, None] >= K2[None]] == 0).all()
    zero = restate_pg(c["obs"], c["noise"], c["lane_sigma"], reward=c["reward"], done=c["done"], gamma=0.0, **common)
    counted = np.arange(K)[:, None] < K2[None]
    assert np.array_equal(zero["rtg"][counted], c["reward"][counted], equal_nan=True)
    # tanh: no clip counts, the actions are not read
    th = restate_pg(c["obs"], c["noise"], c["sigma"], adv=c["adv"], tanh=True, P=P, dtype=dtype, length=c["length"])
    assert (th["clipped"] == 0).all() and not np.array_equal(th["grad"], adv["grad"])
    # obs0 null: obs[k] itself is what step k saw
    same = restate_pg(np.concatenate([c["obs0"][None], c["obs"][:-1]]), c["noise"], c["lane_sigma"], adv=c["adv"], P=P, dtype=dtype,
                      action=c["action"], length=c["length"])
    assert np.array_equal(same["lane_grad"], adv["lane_grad"], equal_nan=True) and np.array_equal(same["grad"], adv["grad"])
    for shape in SHAPES:
        c = crafted_pg(*shape, dtype)
        out = restate_pg(c["obs"], c["noise"], c["lane_sigma"], adv=c["adv"], P=shape[1], dtype=dtype, obs0=c["obs0"], action=c["action"],
                         length=c["length"])
        assert at_most_a_quarter_invalid(out, shape[1], shape[2]) and np.isfinite(out["grad"]).all()


# ---------------------------------------------------------------------------------------
# header, table, exports
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import control, pg
    protos = _prototypes("os2r_pg.h", "os2rg")
    assert [p[0] for p in protos] == list(pg.ENTRY_POINTS) == NAMES
    lib = pg.load()
    for name, ret, args in protos:
        argtypes = pg.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2rg_last_error" else C.c_int)
    args = protos[2][2]
    assert args[0] == "const Os2rControlLayout* layout" and args[4] == "uint32_t flags" and args[-1] == "void* stream" and len(args) == 26
    assert args[14] == "double gamma" and pg.ENTRY_POINTS["os2rg_policy_gradient"][14] is C.c_double
    assert pg.ENTRY_POINTS["os2rg_policy_gradient"][2] is C.c_int64
    header = _header("os2r_pg.h")
    assert re.search(r"#define OS2R_PG_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert lib.os2rg_abi_version() == pg.ABI_VERSION == 1
    assert pg.TANH == int(re.search(r"#define OS2RG_TANH (\d)u", header).group(1)) == 1
    assert pg.SIGMA_PER_LANE == int(re.search(r"#define OS2RG_SIGMA_PER_LANE (\d)u", header).group(1)) == 2
    assert pg.Os2rControlLayout is control.Os2rControlLayout and pg.layout is control.layout
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", pg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)


def test_the_other_libraries_are_as_they_were():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib, cem, control, ekf, mppi, pf, pg, search, steer, ukf
    loaders = (control, search, steer, mppi, pf, ekf, ukf, cem)
    others = set(_lib.ENTRY_POINTS) | set(_lib.RECORD_ENTRY_POINTS) | set().union(*(set(mod.ENTRY_POINTS) for mod in loaders))
    assert not set(pg.ENTRY_POINTS) & others and not any(name.startswith("os2rg_") for name in others)
    prefixes = {name.split("_")[0] + "_" for name in others}
    assert not any(name.startswith(tuple(prefixes - {"os2r_"})) for name in pg.ENTRY_POINTS)
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "os2r_pg.h":
            assert "os2rg_" not in _header(name) and "os2r_pg" not in _header(name).lower(), name
    assert len(_lib.ENTRY_POINTS) == 35 and len(_lib.RECORD_ENTRY_POINTS) == 3
    assert [len(mod.ENTRY_POINTS) for mod in loaders] == [3, 3, 4, 3, 3, 3, 4, 3]
    exports = {_lib.LIB_PATH: set(_lib.ENTRY_POINTS), _lib.RECORD_LIB_PATH: set(_lib.RECORD_ENTRY_POINTS)}
    exports.update({mod.LIB_PATH: set(mod.ENTRY_POINTS) for mod in loaders})
    assert len(exports) == 10
    for path, table in exports.items():
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == table, path
        kernels = kernel_meta.kernel_meta(path)
        assert kernels and not any("policy_gradient" in k for k in kernels), path


def test_kernel_resources():
    """Exactly six kernels, the lane kernel and the two sums in float and double, are in the built library and none uses scratch:
    private_segment_fixed_size 0, no VGPR or SGPR spill, no AGPRs and no LDS in the code-object metadata.  The lane kernel keeps four
    steps of loads in flight: 112 VGPRs in float, 150 in double; the sum over up to 64 samples holds its 64 terms: 71 and 133; the
    sum of a wave 55 in both."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import pg
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(pg.LIB_PATH)
    meta = kernel_meta.kernel_meta(pg.LIB_PATH)
    assert len(meta) == 6, sorted(meta)
    for kernel in ("policy_gradient_lane_kernel", "policy_gradient_sum_kernel", "policy_gradient_sum_few_kernel"):
        for real in ("float", "double"):
            (name,) = [k for k in meta if f"{kernel}<{real}>" in k]
            m = meta[name]
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
            assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 256 and m["group_segment_fixed_size"] == 0, (name, m)


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def test_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import control, pg
    lib = pg.load()
    K, P, S, D = 3, 2, 2, 4
    N = S * P
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
    size = dict(obs=K * N * D, obs0=N * D, noise=K * N * 2, act=K * N * 2, sigma=2, length=N, adv=N, reward=K * N, done=K * N,
                baseline=K * P, grad=2 * (D + 1) * P, lane_grad=2 * (D + 1) * N, lsig=2 * P, lane_lsig=2 * N, steps=P, clipped=2 * P,
                valid=P, rtg=K * N, count=4 * N)
    where, nxt = {}, 0
    for name, n in size.items():
        if name == "grad":
            nxt = 4096
        where[name] = nxt
        nxt += (n + 1) & ~1                               # every array starts at a pair
    assert where["baseline"] + size["baseline"] < 4096 and nxt < 8000
    good = dict(lay=Lay(), K=K, P=P, S=S, flags=0, obs=at(where["obs"]), obs0=at(where["obs0"]), noise=at(where["noise"]), act=at(where["act"]),
                sigma=at(where["sigma"]), length=at(where["length"]), adv=at(where["adv"]), reward=None, done=None, gamma=1.0, baseline=None,
                grad=at(where["grad"]), lane_grad=at(where["lane_grad"]), lsig=at(where["lsig"]), lane_lsig=at(where["lane_lsig"]),
                steps=at(where["steps"]), clipped=at(where["clipped"]), valid=at(where["valid"]), rtg=None, count=at(where["count"]))
    rew = dict(adv=None, reward=at(where["reward"]), done=at(where["done"]))
    name = "os2rg_policy_gradient"
    assert len(good) + 1 == len(pg.ENTRY_POINTS[name])

    def call(**kw):
        a = dict(good, **kw)
        return lib.os2rg_policy_gradient(*[a[k] for k in good], None)
    assert lib.os2rg_policy_gradient(*[None if _is_pointer(t) else 0 for t in pg.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rg_last_error() == b"os2rg_policy_gradient: null layout"
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(nq=1)), b"nq must be 2..5"),
             (dict(lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"), (dict(lay=Lay(obs_dim=13)), b"obs_dim must be 1..12"),
             (dict(K=0), b"nsteps must be >= 1"), (dict(K=-2), b"nsteps must be >= 1"), (dict(K=65536), b"nsteps must be <= 65535"),
             (dict(P=0), b"npolicies must be >= 1"), (dict(P=-1), b"npolicies must be >= 1"), (dict(S=0), b"nsamples must be >= 1"),
             (dict(S=-4), b"nsamples must be >= 1"), (dict(P=2 ** 62), b"nsamples * npolicies exceeds 2^31 - 1"),
             (dict(P=2 ** 30, S=2), b"nsamples * npolicies exceeds 2^31 - 1"), (dict(P=1, S=2 ** 30, K=2), b"nsamples * nsteps exceeds 2^31 - 1"),
             (dict(flags=4), b"unknown flag bits"), (dict(flags=0x80000001), b"unknown flag bits"),
             (dict(gamma=nan), b"gamma must be finite"), (dict(gamma=inf), b"gamma must be finite"), (dict(gamma=-inf), b"gamma must be finite"),
             (dict(gamma=-1e-300), b"gamma must be in [0, 1]"), (dict(gamma=1.0000001), b"gamma must be in [0, 1]"),
             (dict(rew, gamma=nan), b"gamma must be finite"), (dict(rew, gamma=2.0), b"gamma must be in [0, 1]"),
             (dict(obs=None), b"null obs_dev"), (dict(noise=None), b"null noise_dev"), (dict(sigma=None), b"null sigma_dev"),
             (dict(grad=None), b"null grad_dev"), (dict(lane_grad=None), b"null lane_grad_dev"), (dict(count=None), b"null lane_count_dev"),
             (dict(act=None), b"null action_dev without OS2RG_TANH"),
             (dict(reward=at(where["reward"]), done=at(where["done"])), b"adv_dev and reward_dev are both given"),
             (dict(adv=None), b"neither adv_dev nor reward_dev is given"), (dict(rew, done=None), b"reward_dev needs done_dev"),
             (dict(baseline=at(where["baseline"])), b"baseline_dev needs reward_dev"), (dict(rtg=at(where["rtg"])), b"rtg_dev needs reward_dev"),
             (dict(lane_lsig=None), b"lsig_grad_dev needs lane_lsig_dev"), (dict(lsig=None), b"lane_lsig_dev needs lsig_grad_dev"),
             (dict(noise=at(where["noise"] + 1)), b"noise_dev must be aligned to a pair"),
             (dict(act=at(where["act"] + 1)), b"action_dev must be aligned to a pair"),
             (dict(lay=Lay(abi.F32), noise=C.c_void_p(base + 4)), b"noise_dev must be aligned to a pair"),
             # an output over an input, from both sides; over another output; the optional ones too
             (dict(grad=at(where["obs"] + size["obs"] - 1)), b"grad_dev overlaps obs_dev"),
             (dict(grad=at(where["obs0"] - size["grad"] + 1)), b"grad_dev overlaps obs_dev"),
             (dict(lane_grad=at(where["noise"])), b"lane_grad_dev overlaps noise_dev"), (dict(count=at(where["act"])), b"lane_count_dev overlaps action_dev"),
             (dict(steps=at(where["sigma"] + 1)), b"steps_dev overlaps sigma_dev"), (dict(valid=at(where["length"])), b"valid_dev overlaps length_dev"),
             (dict(clipped=at(where["adv"] + N - 1)), b"clipped_dev overlaps adv_dev"),
             (dict(rew, rtg=at(where["reward"] + K * N - 1)), b"rtg_dev overlaps reward_dev"),
             (dict(rew, lsig=at(where["done"])), b"lsig_grad_dev overlaps done_dev"),
             (dict(rew, baseline=at(where["baseline"]), lane_lsig=at(where["baseline"] + K * P - 1)), b"lane_lsig_dev overlaps baseline_dev"),
             (dict(lane_grad=at(where["grad"] + size["grad"] - 1)), b"lane_grad_dev overlaps grad_dev"),
             (dict(lsig=at(where["lane_grad"])), b"lsig_grad_dev overlaps lane_grad_dev"), (dict(lane_lsig=at(where["lsig"] + 1)), b"lane_lsig_dev overlaps lsig_grad_dev"),
             (dict(steps=at(where["lane_lsig"])), b"steps_dev overlaps lane_lsig_dev"), (dict(clipped=at(where["steps"])), b"clipped_dev overlaps steps_dev"),
             (dict(valid=at(where["clipped"])), b"valid_dev overlaps clipped_dev"), (dict(rew, rtg=at(where["valid"])), b"rtg_dev overlaps valid_dev"),
             (dict(rew, rtg=at(where["rtg"]), count=at(where["rtg"] + K * N - 1)), b"lane_count_dev overlaps rtg_dev")]
    seen = set()
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.os2rg_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(b"os2rg_policy_gradient: "), (kw.keys(), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases}) == 46              # each cause has a text of its own
    assert not any(buf)                                                   # a refused call wrote nothing
    # the edges are taken: nothing is left to refuse but the device, and no call is let through to one
    flat = at(where["sigma"])
    edges = [dict(K=65535, S=1, P=1, obs=at(10 ** 6), noise=at(2 * 10 ** 6), act=at(3 * 10 ** 6)), dict(gamma=0.0), dict(gamma=1.0), dict(rew, gamma=5e-324), dict(flags=3, act=None, sigma=flat),
             dict(flags=1, act=at(where["act"] + 1)), dict(lsig=None, lane_lsig=None), dict(steps=None, clipped=None, valid=None),
             dict(rew, baseline=at(where["baseline"]), rtg=at(where["rtg"])), dict(obs0=None, length=None),
             dict(valid=at(where["rtg"])), dict(lane_grad=at(where["grad"] + size["grad"])), dict(flags=1, act=at(where["act"]), grad=at(where["act"])),
             dict(done=at(where["grad"]))]                                # (done_dev is not read with adv_dev)
    for kw in edges:                                  # (device 1000 is never there, with a GPU or without)
        kw = dict(kw, lay=Lay(device=1000))
        assert call(**kw) == abi.ERR_NO_DEVICE and lib.os2rg_last_error().startswith(b"os2rg_policy_gradient: "), kw
    assert not any(buf)
    # the source: no HIP call and every refusal of an argument before check_device
    body = _function(_csrc("os2r_pg_capi.hip"), "int " + name)
    first_hip = body.index("check_device(")
    assert not re.search(HIP_CALL, body[:first_hip]) and body.index("DeviceGuard") > first_hip and body.index("auto launch") > first_hip
    fails = [m.start() for m in re.finditer(r"fail\(OS2R_ERR_INVALID", body)]
    assert len(fails) == 28 and all(i < first_hip for i in fails)
    texts = re.findall(r'fail\(OS2R_ERR_INVALID, "([^"]+)"', body)
    assert len(texts) == len(set(texts)) == 26 and all(any(t.encode() in e for e in seen) for t in texts)


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
    from gym_os2r_amd import pg
    from gym_os2r_amd.sim import HipSim
    assert callable(HipSim.policy_gradient) and callable(HipSim.policy_gradient_into)

    def no_load():
        raise AssertionError("a refused call reached pg.load")
    monkeypatch.setattr(pg, "load", no_load)
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    s = _bare(f64)
    K, P, S, D = 3, 2, 2, 4
    N = S * P
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    obs, noise, act, sig = z(K, N, D), z(K, N, 2), z(K, N, 2), z(2)
    grad, lane, count = z(2, D + 1, P), z(2, D + 1, N), z(4, N, dtype=i32)
    ok = dict(policies=P, actions=act, adv=z(N))
    rew = dict(policies=P, actions=act, rewards=z(K, N), done=z(K, N, dtype=u8))

    def into(*args, raw=None, **kw):                  # raw: the keywords as they are; else `ok` with `kw` over it
        with pytest.raises(ValueError, match="^policy_gradient: "):
            s.policy_gradient_into(*args, **(dict(ok, **kw) if raw is None else raw))

    def whole(*args, raw=None, **kw):
        with pytest.raises(ValueError, match="^policy_gradient: "):
            s.policy_gradient(*args, **(dict(ok, **kw) if raw is None else raw))
    full = (obs, noise, sig, grad, lane, count)
    surface = (obs, noise, sig)
    for bad in (0, -1, 3, 2.0, True, None, "2"):
        into(*full, policies=bad)
        whole(*surface, policies=bad)
    for bad in (float("nan"), float("inf"), -0.1, 1.5, "x", None, True):
        into(*full, gamma=bad)
        whole(*surface, gamma=bad)
        into(*full, raw=dict(rew, gamma=bad))
    for kw in (dict(policies=P, actions=act), dict(rew, adv=z(N)), dict(policies=P, actions=act, rewards=z(K, N)),
               dict(ok, baseline=z(K, P)), dict(ok, done=z(K, N, dtype=u8), baseline=z(K, P))):
        into(*full, raw=kw)
        whole(*surface, raw=kw)
    into(*full, rtg=z(K, N))
    whole(*surface, want_rtg=True)
    into(*full, actions=None)
    whole(*surface, actions=None)
    into(*full, lsig_grad=z(2, P))
    into(*full, lane_lsig=z(2, N))
    for i in range(len(full)):
        into(*[None if j == i else t for j, t in enumerate(full)])
    for args in ((z(K, N), noise, sig, grad, lane, count), (z(0, N, D), noise, sig, grad, lane, count), (obs.numpy(), noise, sig, grad, lane, count),
                 (z(K, N + 1, D), noise, sig, grad, lane, count), (z(K, N, D + 1), noise, sig, grad, lane, count),
                 (obs.float(), noise, sig, grad, lane, count), (z(N, K, D).permute(1, 0, 2), noise, sig, grad, lane, count),
                 (obs, z(K, N, 3), sig, grad, lane, count), (obs, noise.float(), sig, grad, lane, count), (obs, noise, z(3), grad, lane, count),
                 (obs, noise, z(N, 2), grad, lane, count), (obs, noise, z(2, N + 1), grad, lane, count), (obs, noise, sig, z(P, 2, D + 1), lane, count),
                 (obs, noise, sig, grad, z(N, 2, D + 1), count), (obs, noise, sig, grad, lane, z(4, N)), (obs, noise, sig, grad, lane, z(3, N, dtype=i32)),
                 (obs, z(K, N + 1, 2).reshape(-1)[1:1 + K * N * 2].reshape(K, N, 2), sig, grad, lane, count),
                 (obs, noise, sig, obs.reshape(-1)[:2 * (D + 1) * P].reshape(2, D + 1, P), lane, count),
                 (obs, noise, sig, grad, z(0), count)):
        into(*args)
    misaligned = z(K * N * 2 + 1)[1:].reshape(K, N, 2)
    into(*full, actions=misaligned)
    pool = z(4096)
    into(obs, noise, sig, pool[:2 * (D + 1) * P].reshape(2, D + 1, P), pool[5:5 + 2 * (D + 1) * N].reshape(2, D + 1, N), count)
    for kw in (dict(obs0=z(N, D + 1)), dict(obs0=z(N, D).float()), dict(length=z(N)), dict(length=z(N + 1, dtype=i32)), dict(steps=z(P)),
               dict(steps=z(P + 1, dtype=i32)), dict(clipped=z(P, 3, dtype=i32)), dict(valid=z(P, dtype=torch.int64)),
               dict(lsig_grad=z(P, 3), lane_lsig=z(2, N)), dict(lsig_grad=z(2, P), lane_lsig=z(N, 2)), dict(adv=z(N + 1)),
               dict(actions=z(K, N, 3)), dict(steps=count[0, :P])):
        into(*full, **kw)
    for kw in (dict(done=z(K, N)), dict(baseline=z(P, K)), dict(rtg=z(N, K)), dict(rewards=z(K, N + 1)), dict(rtg=rew["rewards"])):
        into(*full, raw=dict(rew, **kw))
    for args in ((None, noise, sig), (obs, None, sig), (obs, noise, None), (obs, noise, True), (obs, noise, z(N + 1, 2)), (obs, noise, "wide"),
                 (obs, z(K, N), sig), (z(K, N + 1, D), noise, sig), (obs, noise, z(2).float())):
        whole(*args)
    for kw in (dict(obs0=z(N)), dict(length=z(N)), dict(adv=z(N).float())):
        whole(*surface, **kw)
    # what passes every check reaches the loader, and only then
    with pytest.raises(AttributeError):                                    # (the bare handle has no cfg to fill a layout from)
        s.policy_gradient_into(*full, **ok)
