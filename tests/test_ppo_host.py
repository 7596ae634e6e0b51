"""libos2r_ppo.so (include/os2r_ppo.h): the host side -- the numpy restatement of the clipped-surrogate gradient the GPU tests
compare with (`restate_ppo`), the crafted inputs of the GPU tests (`crafted_ppo`) and the branches they reach, the first-epoch
identity against `restate_pg` of tests/test_pg_host.py, the restatement against torch autograd in float64, the header against
the one table of gym_os2r_amd/ppo.py, the exports of the library, the resources of the six kernels in the built library, every
refusal of os2ro_ppo_gradient through ctypes without a device, and the argument checks of HipSim.ppo_gradient that need no
device.  No GPU needed."""
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
from test_pg_host import CHUNKS, NONE_VALID, SHAPES, chunked_sum, crafted_pg, plain_pg, restate_pg  # noqa: E402

NAMES = ["os2ro_abi_version", "os2ro_last_error", "os2ro_ppo_gradient"]
CLIP = 0.2
SAME = 1                                # the policy whose weights are weights_old (where P > 1)
# The largest relative distance (the largest difference over the largest entry of the reference) of the restatement from torch
# autograd in float64 over AUTOGRAD_SHAPES, measured on the CPU this test was written on
# (test_the_restatement_is_the_autograd_gradient prints them): the bound is MARGIN x that, the margin of tests/test_pg_host.py.
MEASURED = {np.float64: dict(grad=1.523e-15, lsig=2.172e-15, surr=6.216e-16),
            np.float32: dict(grad=4.405e-7, lsig=5.871e-7, surr=1.156e-7)}
MARGIN = 100
AUTOGRAD_SHAPES = [((7, 3, 65, 10), 0), ((33, 1, 200, 10), 2)]     # with the seed at which no rho lies at a bound, in either dtype
FORBIDDEN = ("os2rg_", "os2r_pg", "os2rv_", "os2r_critic", "os2rx_", "os2r_cem", "os2ru_", "os2r_ukf", "os2re_", "os2r_ekf", "os2rp_",
             "os2r_pf", "os2rm_", "mppi", "os2rt_", "steer", "line_search")


# ---------------------------------------------------------------------------------------
# the restatement of include/os2r_ppo.h (needs no device)
# ---------------------------------------------------------------------------------------
def restate_ppo(obs, noise, sigma, weight, weight_old, adv, *, P, dtype, clip=CLIP, obs0=None, action=None, tanh=False, length=None,
                sigma_new=None, ratio=None):
    """include/os2r_ppo.h, steps 1-17, in numpy and in `dtype`.  obs [K, N, D], noise and action [K, N, 2], sigma [2] or [2, N],
    sigma_new [2, P] or None, weight and weight_old [2, D+1, P], adv [K, N].  `ratio` [K, N]: rho as the device formed it (read
    where k < len); None: rho is formed with np.exp.
    -> dict(grad [2, D+1, P], lane_grad [2, D+1, N], lsig_grad [2, P], lane_lsig [2, N], stat [3, P], lane_stat [3, N], steps [P],
    clipped [2, P], gated [P], valid [P], ratio [K, N], lane_count [5, N]) and, for the test of rho, h [K, N] and rprod [K, N]
    (r'_0 r'_1), both 0 where k >= len."""
    f = lambda a: None if a is None else np.asarray(a).astype(dtype)
    obs, obs0, noise, action, adv, weight, weight_old, sigma_new, ratio = (
        f(a) for a in (obs, obs0, noise, action, adv, weight, weight_old, sigma_new, ratio))
    K, N, D = obs.shape
    S = N // P
    sig = np.broadcast_to(f(sigma).reshape(2, -1), (2, N))
    lo, hi = dtype(np.float64(1) - np.float64(clip)), dtype(np.float64(1) + np.float64(clip))       # formed in double, rounded once
    ln = np.full(N, K, np.int64) if length is None else np.clip(np.asarray(length, np.int64), 0, K)
    pol = np.arange(N) % P
    one, half = dtype(1), dtype(0.5)
    L, V, stat = np.zeros((2, D + 1, N), dtype), np.zeros((2, N), dtype), np.zeros((3, N), dtype)
    clipc, gated = np.zeros((2, N), np.int32), np.zeros(N, np.int32)
    rho_out, h_out, rprod_out = np.zeros((K, N), dtype), np.zeros((K, N), dtype), np.zeros((K, N), dtype)
    with np.errstate(all="ignore"):
        dW = (weight - weight_old)[:, :, pol]                                  # once per lane
        if sigma_new is None:
            r, snew = np.ones((2, N), dtype), sig
        else:
            snew = sigma_new[:, pol]
            r = sig / snew
        enabled = (sig > 0) & (snew > 0)                                       # (a NaN is not positive)
        for k in range(K - 1, -1, -1):
            counted = k < ln
            psi = adv[k]                                                       # step 1
            x = obs[k] if obs0 is None else (obs0 if k == 0 else obs[k - 1])
            z, t, rp, opened = [None, None], [None, None], [None, None], [None, None]
            for j in range(2):
                inside = np.ones(N, bool) if tanh else np.abs(action[k, :, j]) < 1   # step 2 (a NaN is not)
                clipc[j] += counted & ~inside
                opened[j] = enabled[j] & inside
                q = []
                for g in range(4):                                             # step 3
                    acc = np.zeros(N, dtype)
                    for d in range(3 * g, min(3 * g + 3, D)):
                        acc = acc + dW[j, d] * x[:, d]
                    q.append(acc)
                dmu = ((q[0] + q[1]) + (q[2] + q[3])) + dW[j, D]
                eps = noise[k, :, j]
                z[j] = (eps - dmu / sig[j]) * r[j]                             # steps 4 and 5
                t[j] = np.where(opened[j], eps * eps - z[j] * z[j], dtype(0))
                rp[j] = np.where(opened[j], r[j], one)
            h = half * (t[0] + t[1])                                           # step 6
            rprod = rp[0] * rp[1]
            rho = np.exp(h) * rprod if ratio is None else ratio[k]             # steps 7 to 9
            rho_out[k], h_out[k], rprod_out[k] = np.where(counted, rho, 0), np.where(counted, h, 0), np.where(counted, rprod, 0)
            up, down = (psi > 0) & (rho > hi), (psi < 0) & (rho < lo)          # step 10 (a NaN closes nothing)
            closed = up | down
            gated += counted & closed
            stat[0] = np.where(counted, stat[0] + np.where(up, psi * hi, np.where(down, psi * lo, rho * psi)), stat[0])   # steps 11 to 13
            stat[1] = np.where(counted, stat[1] + (rho - one), stat[1])
            stat[2] = np.where(counted, stat[2] + h, stat[2])
            w = psi * rho                                                      # step 14
            for j in range(2):
                go = counted & opened[j] & ~closed
                c = w * (z[j] / snew[j])
                for d in range(D):
                    L[j, d] = np.where(go, L[j, d] + c * x[:, d], L[j, d])
                L[j, D] = np.where(go, L[j, D] + c, L[j, D])
                V[j] = np.where(go, V[j] + w * (z[j] * z[j] - one), V[j])
        fine = np.isfinite(L).all((0, 1)) & np.isfinite(V).all(0) & np.isfinite(stat).all(0)     # step 15
        shaped = fine.reshape(S, P)
        grad = chunked_sum(L.reshape(2, D + 1, S, P), shaped)                  # steps 16 and 17
        lsig = chunked_sum(V.reshape(2, S, P), shaped)
        tot = chunked_sum(stat.reshape(3, S, P), shaped)
    count = np.stack([ln.astype(np.int32), clipc[0], clipc[1], gated, fine.astype(np.int32)])
    steps, clip0, clip1, gate, valid = (chunked_sum(row.reshape(S, P), shaped) for row in count)
    assert all(a.dtype == dtype for a in (L, V, stat, grad, lsig, tot, rho_out)) and all(a.dtype == np.int32 for a in (steps, gate, valid))
    return dict(grad=grad, lane_grad=L, lsig_grad=lsig, lane_lsig=V, stat=tot, lane_stat=stat, steps=steps, clipped=np.stack([clip0, clip1]),
                gated=gate, valid=valid, ratio=rho_out, lane_count=count, h=h_out, rprod=rprod_out)


def crafted_ppo(K, P, S, D, dtype, seed=0):
    """The inputs of the GPU tests, in `dtype`: obs, obs0, noise, action, sigma, lane_sigma and length are crafted_pg's, with its
    lengths of 0, K, -3 and K + 5 (l % 11 == 1, 2, 3, 4), its NaNs beyond len (l % 7 == 6; here in adv too), its actions of
    exactly +-1 (l % 5 == 0) and its per-lane sigma of 0 and NaN (l % 9 == 1, 3).  Beside them, by lane l = s P + p (where the shape
    reaches it):
      weight_old, weight     N(0, 0.3) and a step of 0.05 N(0, 1) from it: both gate directions, and open gates beside them
      p == SAME (P > 1)      weight == weight_old: every rho is 1 where sigma_new is null
      l % 13 == 5            psi = 0 at the even steps
      s % 8 == 5 (S >= 6)    the observation is 3 dW_0 / |dW_0| at every step, eps_0 = 2000, the length K: where sigma_new is null and
                             the policy is not SAME rho overflows and the lane is invalid
      p == 2 (P > 2)         an infinite adv at step 0 of every lane of the policy: none of its lanes is valid
      sigma_new              [0.25, 0.25] in policy SAME, else (0.3, 0.25) U(0.95, 1.05); 0 on motor 0 where p % 4 == 0 and P > 1, NaN
                             on motor 1 where p % 4 == 2
      s == 3, 4 of SAME (S >= 5)   eps = 0, the length K, the per-lane sigma (hi / 4, 1 / 4) with adv = 1 and (lo / 4, 1 / 4)
                             with adv = -1: with per-lane sigma and sigma_new, rho is exactly hi and exactly lo, and the gate is open
    -> dict(obs, obs0, noise, action, sigma [2], lane_sigma [2, N], length, adv [K, N], weight, weight_old, sigma_new [2, P])"""
    c = crafted_pg(K, P, S, D, dtype, seed)
    rng = np.random.default_rng(seed + 1000)
    N = S * P
    l = np.arange(N)
    s, p = l // P, l % P
    obs, obs0, noise, action = (c[k].astype(np.float64) for k in ("obs", "obs0", "noise", "action"))
    lane_sigma, length = c["lane_sigma"].astype(np.float64), c["length"].copy()
    weight_old = rng.normal(0, 0.3, (2, D + 1, P)).astype(dtype).astype(np.float64)
    weight = (weight_old + 0.05 * rng.normal(0, 1, (2, D + 1, P))).astype(dtype).astype(np.float64)
    if P > 1:
        weight[:, :, SAME] = weight_old[:, :, SAME]
    adv = rng.normal(0, 1, (K, N))
    adv[0::2, l % 13 == 5] = 0.0
    sigma_new = np.array([0.3, 0.25])[:, None] * rng.uniform(0.95, 1.05, (2, P))
    if P > 1:
        sigma_new[0, np.arange(P) % 4 == 0] = 0.0
        sigma_new[:, SAME] = 0.25
    sigma_new[1, np.arange(P) % 4 == 2] = np.nan
    # the overflowing lanes (crafted_pg has set their length to K, their sigma to 0.25 and left them free of NaNs)
    over = (s % 8 == 5) & (S >= 6)
    dW0 = (weight - weight_old)[0, :D, :]
    norm = np.sqrt((dW0 * dW0).sum(0))
    v = 3.0 * dW0 / np.where(norm > 0, norm, 1.0)                              # [D, P]
    obs[:, over, :], obs0[over, :] = v.T[p[over]][None], v.T[p[over]]
    noise[:, over, 0], action[:, over, :] = 2000.0, 0.5
    # the policy none of whose lanes is valid
    none = (p == NONE_VALID) & (P > 2)
    adv[0, none] = np.inf
    # rho exactly hi and exactly lo
    lo, hi = float(dtype(1.0 - CLIP)), float(dtype(1.0 + CLIP))
    if P > 1 and S >= 5:
        for sample, bound, sign in ((3, hi, 1.0), (4, lo, -1.0)):
            lane = sample * P + SAME
            length[lane] = K
            obs[:, lane, :], noise[:, lane, :], action[:, lane, :] = rng.normal(0, 1, (K, D)), 0.0, 0.5
            lane_sigma[:, lane] = (bound * 0.25, 0.25)
            adv[:, lane] = sign
    beyond = (np.arange(K)[:, None] >= np.clip(length, 0, K)[None]) & (l % 7 == 6)[None]
    adv[beyond] = np.nan
    f = lambda a: np.ascontiguousarray(a.astype(dtype))
    return dict(obs=f(obs), obs0=f(obs0), noise=f(noise), action=f(action), sigma=c["sigma"], lane_sigma=f(lane_sigma), length=length,
                adv=f(adv), weight=f(weight), weight_old=f(weight_old), sigma_new=f(sigma_new))


def ppo_kwargs(c, P, dtype, *, obs0=True, per_lane=False, sigma_new=False, tanh=False):
    """The arguments of restate_ppo for one configuration of the crafted inputs `c` -> (positional, keywords)."""
    return ((c["obs"], c["noise"], c["lane_sigma"] if per_lane else c["sigma"], c["weight"], c["weight_old"], c["adv"]),
            dict(P=P, dtype=dtype, obs0=c["obs0"] if obs0 else None, action=None if tanh else c["action"], tanh=tanh, length=c["length"],
                 sigma_new=c["sigma_new"] if sigma_new else None))


def at_most_a_quarter_invalid(out, P, S):
    """Of the restatement `out`: the policy NONE_VALID (P > 2) has no valid lane and zeros for sums; of every other policy at most
    a quarter of the lanes is invalid (the cap of tests/test_pg_host.py)."""
    fine = out["lane_count"][4].reshape(S, P)
    for p in range(P):
        if P > 2 and p == NONE_VALID:
            assert fine[:, p].sum() == 0 == out["valid"][p] == out["steps"][p] == out["gated"][p] and (out["clipped"][:, p] == 0).all()
            assert (out["grad"][:, :, p] == 0).all() and (out["lsig_grad"][:, p] == 0).all() and (out["stat"][:, p] == 0).all()
        else:
            assert 4 * (S - fine[:, p].sum()) <= S and out["valid"][p] == fine[:, p].sum(), (p, S, fine[:, p].sum())
    return True


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_on_crafted_inputs_that_reach_every_branch(dtype):
    from gym_os2r_amd import pg, ppo
    assert CHUNKS == ppo.CHUNKS == pg.CHUNKS == int(re.search(r"#define OS2RO_CHUNKS (\d+)", _header("os2r_ppo.h")).group(1))
    K, P, S, D = 7, 3, 65, 10
    c = crafted_ppo(K, P, S, D, dtype)
    N, l = S * P, np.arange(S * P)
    s, p = l // P, l % P
    lo, hi = dtype(1.0 - CLIP), dtype(1.0 + CLIP)
    args, kw = ppo_kwargs(c, P, dtype)
    out = restate_ppo(*args, **kw)
    assert at_most_a_quarter_invalid(out, P, S)
    ln, clip0, clip1, gated, fine = out["lane_count"]
    counted = np.arange(K)[:, None] < ln[None]
    rho, adv = out["ratio"], c["adv"]
    # the gated share of the counted steps of the valid lanes, and the same from the totals
    share = gated[fine == 1].sum() / ln[fine == 1].sum()
    print(f"gated share at {(K, P, S, D)} {dtype.__name__}: {share:.3f}")
    assert 0.10 <= share <= 0.60 and out["gated"].sum() == gated[fine == 1].sum() and out["steps"].sum() == ln[fine == 1].sum()
    # both gate directions, and an open gate beside each, in valid lanes of policy 0
    good = counted & ((p == 0) & (fine == 1))[None]
    with np.errstate(invalid="ignore"):
        assert (good & (adv > 0) & (rho > hi)).any() and (good & (adv > 0) & (rho <= hi) & (rho != 1)).any()
        assert (good & (adv < 0) & (rho < lo)).any() and (good & (adv < 0) & (rho >= lo) & (rho != 1)).any()
        # the opposite signs close nothing, and psi = 0 closes nothing: the lane's count is that of the two closing cases
        assert (good & (adv > 0) & (rho < lo)).any() and (good & (adv < 0) & (rho > hi)).any()
        assert np.array_equal(gated, (counted & (((adv > 0) & (rho > hi)) | ((adv < 0) & (rho < lo)))).sum(0))
    zero = np.flatnonzero((l % 13 == 5) & (ln == K) & (fine == 1) & (p == 0))[0]
    assert (c["adv"][0::2, zero] == 0).all() and (rho[0::2, zero] != 1).all()
    # the policy whose weights are the old ones: every rho is 1, nothing is gated, dev and logr are 0
    same = p == SAME
    assert np.array_equal(c["weight"][:, :, SAME], c["weight_old"][:, :, SAME]) and (rho[:, same][counted[:, same]] == 1).all()
    assert out["gated"][SAME] == 0 and (out["stat"][1:, SAME] == 0).all() and out["stat"][0, SAME] != 0 and (out["grad"][:, :, SAME] != 0).all()
    # an overflowing rho makes its lane invalid: the lanes s % 8 == 5 of policy 0 (those of SAME are valid: rho is 1 there)
    over = (s % 8 == 5) & (p == 0)
    assert over.sum() == S // 8 and np.isinf(rho[:, over]).all() and (fine[over] == 0).all() and (fine[(s % 8 == 5) & same] == 1).all()
    assert not np.isfinite(out["lane_stat"][1, over]).any() and np.isfinite(out["stat"]).all() and np.isfinite(out["grad"]).all()
    # the policy with no valid lane, and the count of the invalid lanes; they are left out of the integer sums
    broken = fine == 0
    assert broken.sum() == S + S // 8 and (fine[p == NONE_VALID] == 0).all()
    for name, row in (("steps", ln), ("gated", gated)):
        assert np.array_equal(out[name], np.where(broken, 0, row).reshape(S, P).sum(0))
    assert np.array_equal(out["clipped"][1], np.where(broken, 0, clip1).reshape(S, P).sum(0))
    # the four lengths; a lane of length 0 has zeros for sums and is valid
    assert set(c["length"][[1, 2, 3, 4]]) == {0, K, -3, K + 5} and ln[1] == 0 == ln[3] and ln[2] == K == ln[4]
    assert (out["lane_grad"][:, :, 1] == 0).all() and (out["lane_stat"][:, 1] == 0).all() and fine[1] == 1 and (rho[:, 1] == 0).all()
    # NaNs beyond len change nothing: every lane that holds some is valid (unless broken), its sums are finite, rho is 0 there
    held = (l % 7 == 6) & (ln < K)
    assert held.any() and np.isnan(c["obs"][-1, held]).all() and np.isnan(c["adv"][-1, held]).all()
    assert np.isfinite(out["lane_grad"][:, :, held & ~broken]).all() and (rho[~counted] == 0).all()
    # actions of exactly +-1 are clipped, whatever the widths; the nearest values below are not
    five = np.flatnonzero((l % 5 == 0) & ~broken & (ln == K) & (p == 0))[0]
    assert clip0[five] == clip1[five] == len([k for k in range(K) if k % 4 < 2]) and (np.abs(c["action"][2, five]) < 1).all()
    assert (out["h"][0, five] == 0) and rho[0, five] == 1 and out["h"][2, five] != 0
    # tanh: no clip counts, the actions are not read
    th = restate_ppo(*args, **dict(kw, tanh=True, action=None))
    assert (th["clipped"] == 0).all() and not np.array_equal(th["grad"], out["grad"])
    # obs0 null: obs[k] itself is what step k saw
    shifted = dict(c, obs=np.concatenate([c["obs0"][None], c["obs"][:-1]]))
    a2, k2 = ppo_kwargs(shifted, P, dtype, obs0=False)
    moved = restate_ppo(*a2, **k2)
    assert np.array_equal(moved["lane_grad"], out["lane_grad"], equal_nan=True) and np.array_equal(moved["grad"], out["grad"])
    # a per-lane sigma of 0 and NaN: the row of that motor is 0, the other is not, and the ratio is that of the other motor alone
    args_l, kw_l = ppo_kwargs(c, P, dtype, per_lane=True)
    lane = restate_ppo(*args_l, **kw_l)
    assert at_most_a_quarter_invalid(lane, P, S)
    fine_l, ln_l = lane["lane_count"][4], lane["lane_count"][0]
    z0, nan = (np.flatnonzero((l % 9 == m) & (l % 5 != 0) & (fine_l == 1) & (ln_l > 1))[0] for m in (1, 3))
    assert (lane["lane_grad"][0, :, z0] == 0).all() and (lane["lane_grad"][1, :, z0] != 0).any() and lane["lane_lsig"][0, z0] == 0
    assert (lane["lane_grad"][1, :, nan] == 0).all() and (lane["lane_grad"][0, :, nan] != 0).any()
    # sigma_new: 0 on motor 0 of policy 0 and NaN on motor 1 of policy 2 disable that motor, in the gradient and in the ratio; in
    # policy SAME rho is exactly hi in sample 3 and exactly lo in sample 4, and both gates are open
    args_n, kw_n = ppo_kwargs(c, P, dtype, per_lane=True, sigma_new=True)
    new = restate_ppo(*args_n, **kw_n)
    assert at_most_a_quarter_invalid(new, P, S)
    assert c["sigma_new"][0, 0] == 0 and np.isnan(c["sigma_new"][1, 2]) and (c["sigma_new"][:, SAME] == 0.25).all()
    assert (new["lane_grad"][0][:, p == 0] == 0).all() and (new["grad"][1, :, 0] != 0).all() and (new["lane_lsig"][0, p == 0] == 0).all()
    assert (new["lane_grad"][1][:, p == 2] == 0).all() and (new["lane_count"][4][p == 2] == 0).all()
    at_hi, at_lo = 3 * P + SAME, 4 * P + SAME
    assert (new["ratio"][:, at_hi] == hi).all() and (new["ratio"][:, at_lo] == lo).all() and (new["h"][:, [at_hi, at_lo]] == 0).all()
    assert (c["adv"][:, at_hi] == 1).all() and (c["adv"][:, at_lo] == -1).all() and new["lane_count"][3][[at_hi, at_lo]].tolist() == [0, 0]
    assert new["lane_stat"][0, at_hi] != 0 and new["gated"][SAME] > 0 and new["lane_count"][4][[at_hi, at_lo]].tolist() == [1, 1]
    # a partial with two terms (s = 0 and 64) beside partials with one
    assert S == CHUNKS + 1
    for shape in SHAPES:
        c = crafted_ppo(*shape, dtype)
        for config in (dict(), dict(per_lane=True, sigma_new=True)):
            a, k = ppo_kwargs(c, shape[1], dtype, **config)
            o = restate_ppo(*a, **k)
            assert at_most_a_quarter_invalid(o, shape[1], shape[2]) and np.isfinite(o["grad"]).all() and np.isfinite(o["stat"]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_first_epoch_is_the_score_function_gradient_bit_for_bit(dtype):
    """With weights == weights_old and sigma_new null the restatement equals restate_pg(reward=adv, gamma=0.0) in grad, lane_grad,
    lsig_grad, lane_lsig, steps, clipped and valid bit for bit, on every shape, with shared and per-lane sigma and with tanh;
    every rho is 1 and no gate closes.  (done is all ones: the reward-to-go of a step is then its reward alone, whatever stands
    behind it -- the infinite adv of the policy none of whose lanes is valid would else turn 0 x inf into a NaN.)"""
    for shape in SHAPES:
        K, P, S, D = shape
        c = crafted_ppo(K, P, S, D, dtype)
        for per_lane, tanh in ((False, False), (True, False), (False, True)):
            args, kw = ppo_kwargs(c, P, dtype, per_lane=per_lane, tanh=tanh)
            got = restate_ppo(args[0], args[1], args[2], c["weight"], c["weight"], args[5], **kw)
            want = restate_pg(args[0], args[1], args[2], P=P, dtype=dtype, obs0=c["obs0"], action=kw["action"], tanh=tanh, length=c["length"],
                              reward=c["adv"], done=np.ones((K, S * P), np.uint8), gamma=0.0)
            for name in ("grad", "lane_grad", "lsig_grad", "lane_lsig", "steps", "clipped", "valid"):
                assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name], equal_nan=True), (shape, per_lane, tanh, name)
            assert np.array_equal(got["lane_count"][[0, 1, 2, 4]], want["lane_count"]) and (got["lane_count"][3] == 0).all()
            ln = got["lane_count"][0]
            assert (got["ratio"][np.arange(K)[:, None] < ln[None]] == 1).all() and (got["lane_stat"][1:] == 0).all()
            if P > 2:
                assert got["valid"][NONE_VALID] == 0                         # (the identity holds on invalid lanes too)


def autograd_ppo(c, P, clip, sigma_new):
    """The reference: torch autograd in float64 on the CPU.  The objective is the sum of min(rho A, clamp(rho, 1 - c, 1 + c) A)
    over the counted steps, rho from the Gaussian log-densities of the pre-squash sample u = mu_old + sigma eps under the new
    and the old policy over the components on which the clip did not bind.  -> (grad [2, D+1, P], lsig [2, P], surr [P], rho [K, N])"""
    import torch
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    O, E, A, adv = t(c["obs"]), t(c["noise"]), t(c["action"]), t(c["adv"])
    K, N, D = O.shape
    pol = torch.arange(N) % P
    prev = torch.cat([t(c["obs0"])[None], O[:-1]])
    ones = torch.ones(K, N, 1, dtype=torch.float64)
    X = torch.cat([prev, ones], 2)                                             # [K, N, D+1]
    W_old = t(c["weight_old"])
    W = t(c["weight"]).clone().requires_grad_(True)                            # [2, D+1, P]
    sig = t(c["sigma"])                                                        # [2]
    logs = torch.log(t(sigma_new)).clone().requires_grad_(True)                # [2, P]
    mu_old = torch.einsum("knd,jdn->knj", X, W_old[:, :, pol])
    mu = torch.einsum("knd,jdn->knj", X, W[:, :, pol])
    u = mu_old + sig * E
    s_new = torch.exp(logs)[:, pol].T                                          # [N, 2]
    logp_new = -torch.log(s_new) - (u - mu) ** 2 / (2 * s_new ** 2)
    logp_old = -torch.log(sig) - (u - mu_old) ** 2 / (2 * sig ** 2)
    inside = (A.abs() < 1.0).to(torch.float64)
    rho = torch.exp(((logp_new - logp_old) * inside).sum(2))
    counted = (torch.arange(K)[:, None] < t(c["length"])[None]).to(torch.float64)
    term = torch.minimum(rho * adv, torch.clamp(rho, 1 - clip, 1 + clip) * adv) * counted
    surr = term.reshape(K, N // P, P).sum((0, 1))
    surr.sum().backward()
    return W.grad.numpy(), logs.grad.numpy(), surr.detach().numpy(), rho.detach().numpy()


def plain_ppo(K, P, S, D, dtype, seed):
    """plain_pg's rollout (no lane is invalid) with adv [K, N], weights a step of 0.05 N(0, 1) apart and a new width within 5 % of the
    old, rounded to `dtype` and returned in float64."""
    c = plain_pg(K, P, S, D, dtype, seed)
    rng = np.random.default_rng(seed + 77)
    r = lambda a: a.astype(dtype).astype(np.float64)
    c["adv"] = r(rng.normal(0, 1, (K, S * P)))
    c["weight_old"] = r(rng.normal(0, 0.3, (2, D + 1, P)))
    c["weight"] = r(c["weight_old"] + 0.05 * rng.normal(0, 1, (2, D + 1, P)))
    c["sigma_new"] = r(c["sigma"][:, None] * rng.uniform(0.95, 1.05, (2, P)))
    return c


def _far(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_is_the_autograd_gradient(dtype):
    """grad, lsig_grad and surr within MARGIN x the distance measured when this was written (relative to the largest entry):
    fp64 1.5e-15, 2.2e-15 and 6.2e-16, fp32 4.4e-7, 5.9e-7 and 1.2e-7, with the new width given and null.  No step's
    float64 rho lies within 1e-4 (relative) of lo or hi, so both sides gate the same steps: gated is that count exactly."""
    worst = dict(grad=0.0, lsig=0.0, surr=0.0)
    for (K, P, S, D), seed in AUTOGRAD_SHAPES:
        c = plain_ppo(K, P, S, D, dtype, seed)
        for new_width in (True, False):
            s_new = c["sigma_new"] if new_width else np.repeat(c["sigma"][:, None], P, 1)
            grad, lsig, surr, rho = autograd_ppo(c, P, CLIP, s_new)
            counted = np.arange(K)[:, None] < c["length"][None]
            for bound in (1 - CLIP, 1 + CLIP):
                assert (np.abs(rho[counted] / bound - 1) > 1e-4).all(), "a rho at a bound: take another seed"
            got = restate_ppo(c["obs"], c["noise"], c["sigma"], c["weight"], c["weight_old"], c["adv"], P=P, dtype=dtype, obs0=c["obs0"],
                              action=c["action"], length=c["length"], sigma_new=c["sigma_new"] if new_width else None)
            assert got["valid"].tolist() == [S] * P and np.array_equal(got["steps"], c["length"].reshape(S, P).sum(0))
            closed = counted & (((c["adv"] > 0) & (rho > 1 + CLIP)) | ((c["adv"] < 0) & (rho < 1 - CLIP)))
            assert np.array_equal(got["gated"], closed.reshape(K, S, P).sum((0, 1))) and 0.1 < closed.sum() / counted.sum() < 0.6
            worst["grad"], worst["surr"] = max(worst["grad"], _far(got["grad"], grad)), max(worst["surr"], _far(got["stat"][0], surr))
            worst["lsig"] = max(worst["lsig"], _far(got["lsig_grad"], lsig))
    print(f"restate_ppo against autograd, {dtype.__name__}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for name, value in worst.items():
        assert value <= MARGIN * MEASURED[dtype][name], (name, value)


# ---------------------------------------------------------------------------------------
# header, table, exports, resources
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import _lib, control, pg, ppo
    protos = _prototypes("os2r_ppo.h", "os2ro")
    assert [p[0] for p in protos] == list(ppo.ENTRY_POINTS) == NAMES
    lib = ppo.load()
    for name, ret, args in protos:
        argtypes = ppo.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2ro_last_error" else C.c_int)
    args = protos[2][2]
    assert args[:5] == ["const Os2rControlLayout* layout", "int32_t nsteps", "int64_t npolicies", "int32_t nsamples", "uint32_t flags"]
    assert len(args) == 29 and args[15] == "double clip" and ppo.ENTRY_POINTS["os2ro_ppo_gradient"][15] is C.c_double
    assert args[-1] == "void* stream" and args[-2] == "int32_t* lane_count_dev" and ppo.ENTRY_POINTS["os2ro_ppo_gradient"][2] is C.c_int64
    header = _header("os2r_ppo.h")
    assert re.search(r"#define OS2R_PPO_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert len(re.findall(r"#include", header)) == 1
    assert lib.os2ro_abi_version() == ppo.ABI_VERSION == 1
    assert ppo.TANH == int(re.search(r"#define OS2RO_TANH (\d)u", header).group(1)) == 1
    assert ppo.SIGMA_PER_LANE == int(re.search(r"#define OS2RO_SIGMA_PER_LANE (\d)u", header).group(1)) == 2
    assert ppo.CHUNKS == int(re.search(r"#define OS2RO_CHUNKS (\d+)", header).group(1)) == pg.CHUNKS == 64
    assert ppo.LANE_COUNTS == int(re.search(r"#define OS2RO_LANE_COUNTS (\d+)", header).group(1)) == 5
    assert ppo.STATS == int(re.search(r"#define OS2RO_STATS (\d+)", header).group(1)) == 3
    assert ppo.Os2rControlLayout is control.Os2rControlLayout and ppo.layout is control.layout
    assert not set(ppo.ENTRY_POINTS) & (set(_lib.ENTRY_POINTS) | set(_lib.RECORD_ENTRY_POINTS)) and len(_lib.ENTRY_POINTS) == 35
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", ppo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "libos2r_ppo.map")) as f:
        assert re.search(r"global:\s*os2ro_\*;\s*local:\s*\*;", f.read())
    # the header names no other companion library (their tests forbid it), and no other header speaks of this one; the sums over
    # the samples are said in words, and are the included bodies
    for word in FORBIDDEN:
        assert word not in header.lower(), word
    assert "adjacent-pair tree" in header and "in ascending order onto 0" in header
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "os2r_ppo.h":
            assert "os2ro_" not in _header(name).lower() and "os2r_ppo" not in _header(name).lower(), name
    assert '#include "os2r_pg.hpp"' in _csrc("os2r_ppo.hpp") and "pg_wave_sum<T>" in _csrc("os2r_ppo.hpp") and "pg_few_sum<T>" in _csrc("os2r_ppo.hpp")


KERNELS = ("ppo_lane_kernel", "ppo_sum_kernel", "ppo_sum_few_kernel")


def test_kernel_resources():
    """Exactly six kernels, the lane kernel and the two sums in float and double, are in the built library and none uses scratch or
    LDS: private_segment_fixed_size 0, no VGPR or SGPR spill, no AGPRs and group_segment_fixed_size 0 in the code-object metadata.
    The lane kernel keeps four steps of loads in flight: 108 VGPRs in float, 154 in double (the score-function lane kernel
    stands at 112 and 150); the sum over up to 64 samples holds its 64 terms: 71 and 133; the sum of a wave 55 in both."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import ppo
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(ppo.LIB_PATH)
    meta = kernel_meta.kernel_meta(ppo.LIB_PATH)
    assert len(meta) == 6, sorted(meta)
    for kernel in KERNELS:
        for real in ("float", "double"):
            (name,) = [k for k in meta if f"{kernel}<{real}>" in k]
            m = meta[name]
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
            assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 256 and m["group_segment_fixed_size"] == 0, (name, m)


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def test_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import control, ppo
    lib = ppo.load()
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
    size = dict(obs=K * N * D, obs0=N * D, noise=K * N * 2, act=K * N * 2, sigma=2, sigma_new=2 * P, weight=2 * (D + 1) * P,
                weight_old=2 * (D + 1) * P, length=N, adv=K * N, grad=2 * (D + 1) * P, lane_grad=2 * (D + 1) * N, lsig=2 * P, lane_lsig=2 * N,
                stat=3 * P, lane_stat=3 * N, steps=P, clipped=2 * P, gated=P, valid=P, ratio=K * N, count=5 * N)
    where, nxt = {}, 0
    for name, n in size.items():
        if name == "grad":
            assert nxt < 4096
            nxt = 4096
        where[name] = nxt
        nxt += (n + 1) & ~1                               # every array starts at a pair
    assert nxt < 8000
    good = dict(lay=Lay(), K=K, P=P, S=S, flags=0, obs=at(where["obs"]), obs0=at(where["obs0"]), noise=at(where["noise"]), act=at(where["act"]),
                sigma=at(where["sigma"]), sigma_new=at(where["sigma_new"]), weight=at(where["weight"]), weight_old=at(where["weight_old"]),
                length=at(where["length"]), adv=at(where["adv"]), clip=0.2, grad=at(where["grad"]), lane_grad=at(where["lane_grad"]),
                lsig=at(where["lsig"]), lane_lsig=at(where["lane_lsig"]), stat=at(where["stat"]), lane_stat=at(where["lane_stat"]),
                steps=at(where["steps"]), clipped=at(where["clipped"]), gated=at(where["gated"]), valid=at(where["valid"]),
                ratio=at(where["ratio"]), count=at(where["count"]))
    name = "os2ro_ppo_gradient"
    assert len(good) + 1 == len(ppo.ENTRY_POINTS[name])

    def call(**kw):
        a = dict(good, **kw)
        return lib.os2ro_ppo_gradient(*[a[k] for k in good], None)
    assert lib.os2ro_ppo_gradient(*[None if _is_pointer(t) else 0 for t in ppo.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2ro_last_error() == b"os2ro_ppo_gradient: null layout"
    end = lambda n: where[n] + size[n] - 1
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(nq=1)), b"nq must be 2..5"),
             (dict(lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"), (dict(lay=Lay(obs_dim=13)), b"obs_dim must be 1..12"),
             (dict(K=0), b"nsteps must be >= 1"), (dict(K=-2), b"nsteps must be >= 1"), (dict(K=65536), b"nsteps must be <= 65535"),
             (dict(P=0), b"npolicies must be >= 1"), (dict(P=-1), b"npolicies must be >= 1"), (dict(S=0), b"nsamples must be >= 1"),
             (dict(S=-4), b"nsamples must be >= 1"), (dict(P=2 ** 62), b"nsamples * npolicies exceeds 2^31 - 1"),
             (dict(P=2 ** 30, S=2), b"nsamples * npolicies exceeds 2^31 - 1"), (dict(P=1, S=2 ** 30, K=2), b"nsamples * nsteps exceeds 2^31 - 1"),
             (dict(flags=4), b"unknown flag bits"), (dict(flags=0x80000001), b"unknown flag bits"),
             (dict(clip=nan), b"clip must be finite"), (dict(clip=inf), b"clip must be finite"), (dict(clip=-inf), b"clip must be finite"),
             (dict(clip=0.0), b"clip must be in (0, 1)"), (dict(clip=-0.2), b"clip must be in (0, 1)"), (dict(clip=1.0), b"clip must be in (0, 1)"),
             (dict(clip=1.5), b"clip must be in (0, 1)"),
             (dict(obs=None), b"null obs_dev"), (dict(noise=None), b"null noise_dev"), (dict(sigma=None), b"null sigma_dev"),
             (dict(weight=None), b"null weight_dev"), (dict(weight_old=None), b"null weight_old_dev"), (dict(adv=None), b"null adv_dev"),
             (dict(grad=None), b"null grad_dev"), (dict(lane_grad=None), b"null lane_grad_dev"), (dict(lane_stat=None), b"null lane_stat_dev"),
             (dict(count=None), b"null lane_count_dev"), (dict(act=None), b"null action_dev without OS2RO_TANH"),
             (dict(lane_lsig=None), b"lsig_grad_dev needs lane_lsig_dev"), (dict(lsig=None), b"lane_lsig_dev needs lsig_grad_dev"),
             (dict(noise=at(where["noise"] + 1)), b"noise_dev must be aligned to a pair"),
             (dict(act=at(where["act"] + 1)), b"action_dev must be aligned to a pair"),
             (dict(lay=Lay(abi.F32), noise=C.c_void_p(base + 4)), b"noise_dev must be aligned to a pair"),
             # an output over an input, from both sides; over another output; the optional ones too
             (dict(grad=at(end("obs"))), b"grad_dev overlaps obs_dev"),
             (dict(grad=at(where["obs0"] - size["grad"] + 1)), b"grad_dev overlaps obs_dev"),
             (dict(lane_grad=at(where["noise"])), b"lane_grad_dev overlaps noise_dev"), (dict(count=at(where["act"])), b"lane_count_dev overlaps action_dev"),
             (dict(steps=at(where["sigma"] + 1)), b"steps_dev overlaps sigma_dev"), (dict(gated=at(end("sigma_new"))), b"gated_dev overlaps sigma_new_dev"),
             (dict(stat=at(where["weight"])), b"stat_dev overlaps weight_dev"), (dict(lane_stat=at(end("weight_old"))), b"lane_stat_dev overlaps weight_old_dev"),
             (dict(valid=at(where["length"])), b"valid_dev overlaps length_dev"), (dict(clipped=at(end("adv"))), b"clipped_dev overlaps adv_dev"),
             (dict(ratio=at(end("adv"))), b"ratio_dev overlaps adv_dev"), (dict(lsig=at(where["obs0"])), b"lsig_grad_dev overlaps obs0_dev"),
             (dict(lane_grad=at(end("grad"))), b"lane_grad_dev overlaps grad_dev"),
             (dict(lsig=at(where["lane_grad"])), b"lsig_grad_dev overlaps lane_grad_dev"), (dict(lane_lsig=at(where["lsig"] + 1)), b"lane_lsig_dev overlaps lsig_grad_dev"),
             (dict(stat=at(where["lane_lsig"])), b"stat_dev overlaps lane_lsig_dev"), (dict(lane_stat=at(end("stat"))), b"lane_stat_dev overlaps stat_dev"),
             (dict(steps=at(where["lane_stat"])), b"steps_dev overlaps lane_stat_dev"), (dict(clipped=at(where["steps"])), b"clipped_dev overlaps steps_dev"),
             (dict(gated=at(where["clipped"] + 1)), b"gated_dev overlaps clipped_dev"), (dict(valid=at(where["gated"])), b"valid_dev overlaps gated_dev"),
             (dict(ratio=at(where["valid"])), b"ratio_dev overlaps valid_dev"), (dict(count=at(end("ratio"))), b"lane_count_dev overlaps ratio_dev")]
    seen = set()
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.os2ro_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(b"os2ro_ppo_gradient: "), (kw.keys(), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases}) == 50              # each cause has a text of its own
    assert not any(buf)                                                   # a refused call wrote nothing
    # the edges are taken: nothing is left to refuse but the device, and no call is let through to one
    edges = [dict(K=65535, S=1, P=1, obs=at(10 ** 6), noise=at(2 * 10 ** 6), act=at(3 * 10 ** 6), adv=at(4 * 10 ** 6), ratio=at(5 * 10 ** 6)),
             dict(clip=5e-324), dict(clip=0.9999999999999999), dict(flags=3, act=None, sigma=at(where["obs"])),
             dict(flags=1, act=at(where["act"] + 1)), dict(lsig=None, lane_lsig=None),
             dict(stat=None, steps=None, clipped=None, gated=None, valid=None, ratio=None), dict(obs0=None, length=None, sigma_new=None),
             dict(weight=at(where["weight_old"])),                         # (two inputs may be one array: the first epoch)
             dict(lane_grad=at(where["grad"] + size["grad"])), dict(flags=1, act=at(where["act"]), grad=at(where["act"]))]
    for kw in edges:                                  # (device 1000 is never there, with a GPU or without)
        kw = dict(kw, lay=Lay(device=1000))
        assert call(**kw) == abi.ERR_NO_DEVICE and lib.os2ro_last_error().startswith(b"os2ro_ppo_gradient: "), kw
    assert not any(buf)
    # the source: no HIP call and every refusal of an argument before check_device
    body = _function(_csrc("os2r_ppo_capi.hip"), "int " + name)
    first_hip = body.index("check_device(")
    assert not re.search(HIP_CALL, body[:first_hip]) and body.index("DeviceGuard") > first_hip and body.index("auto launch") > first_hip
    fails = [m.start() for m in re.finditer(r"fail\(OS2R_ERR_INVALID", body)]
    assert len(fails) == 27 and all(i < first_hip for i in fails)
    texts = re.findall(r'fail\(OS2R_ERR_INVALID, "([^"]+)"', body)
    assert len(texts) == len(set(texts)) == 25 and all(any(t.encode() in e for e in seen) for t in texts)


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
    from gym_os2r_amd import ppo
    from gym_os2r_amd.sim import HipSim
    assert callable(HipSim.ppo_gradient) and callable(HipSim.ppo_gradient_into)
    assert "(dev - logr) / steps" in HipSim.ppo_gradient.__doc__ and "k3" in HipSim.ppo_gradient.__doc__

    def no_load():
        raise AssertionError("a refused call reached ppo.load")
    monkeypatch.setattr(ppo, "load", no_load)
    f64, i32 = torch.float64, torch.int32
    s = _bare(f64)
    K, P, S, D = 3, 2, 2, 4
    N = S * P
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    obs, noise, act, sig, w, w_old, adv = z(K, N, D), z(K, N, 2), z(K, N, 2), z(2), z(2, D + 1, P), z(2, D + 1, P), z(K, N)
    grad, lane, lane_stat, count = z(2, D + 1, P), z(2, D + 1, N), z(3, N), z(5, N, dtype=i32)
    ok = dict(policies=P, actions=act)

    def into(*args, **kw):
        with pytest.raises(ValueError, match="^ppo_gradient: "):
            s.ppo_gradient_into(*args, **dict(ok, **kw))

    def whole(*args, **kw):
        with pytest.raises(ValueError, match="^ppo_gradient: "):
            s.ppo_gradient(*args, **dict(ok, **kw))
    full = (obs, noise, sig, w, w_old, adv, grad, lane, lane_stat, count)
    wv, wv_old = z(P, 2, D + 1), z(P, 2, D + 1)
    surface = (obs, noise, sig, wv, wv_old, adv)
    for bad in (0, -1, 3, 2.0, True, None, "2"):
        into(*full, policies=bad)
        whole(*surface, policies=bad)
    for bad in (float("nan"), float("inf"), 0.0, -0.1, 1.0, 1.5, "x", None, True):
        into(*full, clip=bad)
        whole(*surface, clip=bad)
    into(*full, actions=None)
    whole(*surface, actions=None)
    into(*full, lsig_grad=z(2, P))
    into(*full, lane_lsig=z(2, N))
    for i in range(len(full)):
        into(*[None if j == i else t for j, t in enumerate(full)])
    swap = lambda i, t: tuple(t if j == i else a for j, a in enumerate(full))
    for args in (swap(0, z(K, N)), swap(0, z(0, N, D)), swap(0, obs.numpy()), swap(0, z(K, N + 1, D)), swap(0, z(K, N, D + 1)), swap(0, obs.float()),
                 swap(0, z(N, K, D).permute(1, 0, 2)), swap(1, z(K, N, 3)), swap(1, noise.float()), swap(2, z(3)), swap(2, z(N, 2)),
                 swap(2, z(2, N + 1)), swap(3, z(P, 2, D + 1)), swap(3, w.float()), swap(4, z(2, D, P)), swap(4, z(2, D + 1, P + 1)),
                 swap(5, z(N)), swap(5, z(K, N + 1)), swap(5, z(N, K).t()), swap(6, z(P, 2, D + 1)), swap(7, z(N, 2, D + 1)), swap(8, z(2, N)),
                 swap(8, z(3, N).float()), swap(9, z(5, N)), swap(9, z(4, N, dtype=i32)),
                 swap(1, z(K, N + 1, 2).reshape(-1)[1:1 + K * N * 2].reshape(K, N, 2)),
                 swap(6, obs.reshape(-1)[:2 * (D + 1) * P].reshape(2, D + 1, P)), swap(6, w), swap(8, adv.reshape(-1)[:3 * N].reshape(3, N)),
                 swap(7, z(0))):
        into(*args)
    misaligned = z(K * N * 2 + 1)[1:].reshape(K, N, 2)
    into(*full, actions=misaligned)
    pool = z(4096)
    into(*swap(6, pool[:2 * (D + 1) * P].reshape(2, D + 1, P))[:7], pool[5:5 + 2 * (D + 1) * N].reshape(2, D + 1, N), lane_stat, count)
    for kw in (dict(obs0=z(N, D + 1)), dict(obs0=z(N, D).float()), dict(length=z(N)), dict(length=z(N + 1, dtype=i32)), dict(steps=z(P)),
               dict(steps=z(P + 1, dtype=i32)), dict(clipped=z(P, 3, dtype=i32)), dict(valid=z(P, dtype=torch.int64)), dict(gated=z(P)),
               dict(gated=z(2, P, dtype=i32)), dict(stat=z(P, 3)), dict(stat=z(3, P).float()), dict(ratio=z(N, K)), dict(ratio=adv),
               dict(sigma_new=z(P, 3)), dict(sigma_new=z(2, P + 1)), dict(sigma_new=z(2, P).float()),
               dict(lsig_grad=z(P, 3), lane_lsig=z(2, N)), dict(lsig_grad=z(2, P), lane_lsig=z(N, 2)),
               dict(actions=z(K, N, 3)), dict(steps=count[0, :P]), dict(stat=lane_stat[:, :P])):
        into(*full, **kw)
    for args in ((None, noise, sig, wv, wv_old, adv), (obs, None, sig, wv, wv_old, adv), (obs, noise, None, wv, wv_old, adv),
                 (obs, noise, True, wv, wv_old, adv), (obs, noise, z(N + 1, 2), wv, wv_old, adv), (obs, noise, "wide", wv, wv_old, adv),
                 (obs, z(K, N), sig, wv, wv_old, adv), (z(K, N + 1, D), noise, sig, wv, wv_old, adv), (obs, noise, z(2).float(), wv, wv_old, adv),
                 (obs, noise, sig, None, wv_old, adv), (obs, noise, sig, wv, None, adv), (obs, noise, sig, z(2, D + 1, P + 1), wv_old, adv),
                 (obs, noise, sig, wv, z(P, 2, D), adv), (obs, noise, sig, wv, wv_old, None), (obs, noise, sig, wv, wv_old, z(K, N).float())):
        whole(*args)
    for kw in (dict(obs0=z(N)), dict(length=z(N)), dict(sigma_new=z(P, 3)), dict(sigma_new=z(2, P + 1))):
        whole(*surface, **kw)
    # what passes every check reaches the loader, and only then
    with pytest.raises(AttributeError):                                    # (the bare handle has no cfg to fill a layout from)
        s.ppo_gradient_into(*full, **ok)
    with pytest.raises(AttributeError):
        s.ppo_gradient_into(obs, noise, sig, w, w, adv, grad, lane, lane_stat, count, **ok)      # (the first epoch: one array for both weights)
