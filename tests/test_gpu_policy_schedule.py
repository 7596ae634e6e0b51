"""os2r_rollout_policy_scheduled (include/os2r.h) on the MI355X: closed-loop rollouts whose linear policy is a table of weight
sets indexed by a clock.  The reference is a loop of os2r_step calls on a twin handle whose actions torch computes (the `_policy`
order of test_gpu_policy_rollout.py) from the returned observations with the weights of slot s, s computed in Python from the
window's step index or from episode_info() read before each step.  Every comparison is torch.equal."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from helpers import make_config
from gym_os2r_amd import abi
from test_gpu_policy_rollout import _assert_same_handle, _everything, _policy, _sums

pytestmark = pytest.mark.gpu

N, K, LIMIT = 200, 24, 13          # three waves and a tail of 8; TimeLimit 13


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def HipSim(torch_mod):
    from gym_os2r_amd.sim import HipSim
    return HipSim


def _make(torch, HipSim, mode, dtype, seed=5):
    """Randomised resets and parameters, TimeLimit 13, robots on the ground after 150 random steps, then episode steps = e mod 13:
    the lanes of one wave sit at different slots of the episode clock.  -> (handle, the observation its last step returned)"""
    cfg, _, _ = make_config(mode, "BalancingV2", True, reset_mode=abi.RESET_RANDOM, randomize_params=True, num_envs=N,
                            contact=True, seed=seed, max_episode_steps=LIMIT, dtype=dtype)
    sim = HipSim(cfg)
    for _ in range(150):
        obs = sim.step(None)[0]
    sim.set_episode_info(steps=torch.arange(N, dtype=torch.int32, device=sim.device) % LIMIT)
    return sim, obs


def _table(torch, sim, T, per_env, seed=0, scale=0.6):
    g = torch.Generator().manual_seed(seed)
    shape = (sim.N, T, 2, sim.D + 1) if per_env else (T, 2, sim.D + 1)
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64)).to(sim.device, sim.dtype)


def _slot(torch, sim, k, T, clock, wrap, first_slot):
    """[N] int64: the slot of every environment at the top of env-step k of the window."""
    if clock == "episode":
        t = first_slot + sim.episode_info()[0].to(torch.int64)
    else:
        t = torch.full((sim.N,), first_slot + k, dtype=torch.int64, device=sim.device)
    return t % T if wrap else torch.clamp(t, max=T - 1)


def _schedule_loop(torch, sim, obs, W, clock, wrap=False, first_slot=0, steps=K):
    """`steps` calls of os2r_step with the scheduled policy computed in torch; -> (per-step outputs, actions [K, N, 2], slots)"""
    T = W.shape[-3]
    sim.done_reasons(True)
    out, acts, slots = [], [], []
    ar = torch.arange(sim.N, device=sim.device)
    for k in range(steps):
        s = _slot(torch, sim, k, T, clock, wrap, first_slot)
        Wk = W[ar, s] if W.dim() == 4 else W[s]                  # [N, 2, D+1]
        a = _policy(torch, obs, Wk, False)
        o, r, d, t = sim.step(a)
        out.append((o, r, d, t, sim.reasons.clone()))
        acts.append(a)
        slots.append(s)
        obs = o
    sim.done_reasons(False)
    return out, torch.stack(acts), torch.stack(slots)


def _check_against_loop(torch, a, b, obs_b, W, clock, wrap=False, first_slot=0):
    ret, length, (O, R, Dn, Tm, Wy), (A, E) = a.rollout_schedule(K, W, clock=clock, wrap=wrap, first_slot=first_slot,
                                                                 want_outputs=True, want_terminal=True, want_reasons=True,
                                                                 want_actions=True)
    assert E is None
    per, acts, slots = _schedule_loop(torch, b, obs_b, W, clock, wrap, first_slot)
    T = W.shape[-3]
    # the setting is what the test is about: lanes of the first wave at different slots in the first env-step (episode clock),
    # every slot used, t beyond the table (hold) or a wrap inside the window, episodes ending inside the window
    if clock == "episode":
        assert len(set(slots[0, :64].tolist())) > 1
    assert int(slots.max()) == T - 1 and len(set(slots.flatten().tolist())) >= T - 1
    assert first_slot + K - 1 > T - 1
    assert int((Dn != 0).sum()) > 0 and int((Dn[:K - 1] != 0).sum()) > 0
    for k in range(K):
        for x, y in zip(per[k], (O[k], R[k], Dn[k], Tm[k], Wy[k])):
            assert torch.equal(x, y), k
    assert torch.equal(A, acts)
    r_ref, l_ref = _sums(torch, per, first_episode=False)
    assert torch.equal(ret, r_ref) and torch.equal(length, l_ref) and bool((length == K).all())
    _assert_same_handle(torch, a, b, clock)


@pytest.mark.parametrize("clock", ["window", "episode"])
@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("mode,dtype", [("free_hip", abi.F64), ("free_hip", abi.F32), ("fixed_hip_simple", abi.F64)])
def test_fused_schedule_equals_a_loop_of_steps(HipSim, torch_mod, mode, dtype, per_env, clock):
    """The fused kernel, T = 5 held at its last slot: per-step outputs, returns, lengths, recorded actions and the handle."""
    torch = torch_mod
    (a, _), (b, obs_b) = _make(torch, HipSim, mode, dtype), _make(torch, HipSim, mode, dtype)
    _check_against_loop(torch, a, b, obs_b, _table(torch, a, 5, per_env), clock)
    a.close(); b.close()


@pytest.mark.parametrize("clock", ["window", "episode"])
@pytest.mark.parametrize("per_env", [False, True])
def test_schedule_wraps(HipSim, torch_mod, per_env, clock):
    """T = 4 with OS2R_POLICY_SCHEDULE_WRAP, from first_slot 3: s = t mod 4."""
    torch = torch_mod
    (a, _), (b, obs_b) = _make(torch, HipSim, "free_hip", abi.F64), _make(torch, HipSim, "free_hip", abi.F64)
    _check_against_loop(torch, a, b, obs_b, _table(torch, a, 4, per_env, seed=1), clock, wrap=True, first_slot=3)
    a.close(); b.close()


@pytest.mark.parametrize("wrap,T", [(False, 16), (True, 7)])
@pytest.mark.parametrize("per_env", [False, True])
def test_a_window_may_be_split(HipSim, torch_mod, per_env, wrap, T):
    """Window clock: one window of 24 env-steps equals windows of 10 and 14, the second with first_slot = 10."""
    torch = torch_mod
    (a, _), (b, _) = _make(torch, HipSim, "free_hip", abi.F64), _make(torch, HipSim, "free_hip", abi.F64)
    W = _table(torch, a, T, per_env, seed=2)
    kw = dict(wrap=wrap, want_outputs=True, want_terminal=True, want_reasons=True, want_actions=True)
    _, _, out, (A, _) = a.rollout_schedule(K, W, **kw)
    _, _, out1, (A1, _) = b.rollout_schedule(10, W, **kw)
    _, _, out2, (A2, _) = b.rollout_schedule(14, W, first_slot=10, **kw)
    for x, x1, x2 in zip(out + (A,), out1 + (A1,), out2 + (A2,)):
        assert torch.equal(x, torch.cat([x1, x2]))
    assert int((out[2] != 0).sum()) > 0
    _assert_same_handle(torch, a, b, "split")
    a.close(); b.close()


@pytest.mark.parametrize("clock", ["window", "episode"])
@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_launch_loop_equals_a_loop_of_steps(HipSim, torch_mod, dtype, per_env, clock):
    """fixed_hip_torque has no fused rollout: the policy kernel, the step launch and the sums per env-step."""
    torch = torch_mod
    (a, _), (b, obs_b) = _make(torch, HipSim, "fixed_hip_torque", dtype), _make(torch, HipSim, "fixed_hip_torque", dtype)
    _check_against_loop(torch, a, b, obs_b, _table(torch, a, 5, per_env, seed=3), clock, first_slot=1)
    a.close(); b.close()


@pytest.mark.parametrize("clock", ["window", "episode"])
@pytest.mark.parametrize("per_env", [False, True])
def test_launch_loop_equals_fused_schedule(HipSim, torch_mod, per_env, clock):
    """Work counters on: the library takes its launch loop on a configuration that also has the fused kernel; same results."""
    torch = torch_mod
    (a, _), (b, _) = _make(torch, HipSim, "free_hip", abi.F64), _make(torch, HipSim, "free_hip", abi.F64)
    W = _table(torch, a, 5, per_env, seed=4)
    a.count_work(True)
    for wrap in (False, True):
        kw = dict(clock=clock, wrap=wrap, first_slot=2, want_outputs=True, want_terminal=True, want_reasons=True, want_actions=True)
        ra, la, oa, (aa, _) = a.rollout_schedule(K, W, **kw)
        rb, lb, ob, (ab, _) = b.rollout_schedule(K, W, **kw)
        assert torch.equal(ra, rb) and torch.equal(la, lb) and torch.equal(aa, ab)
        for x, y in zip(oa, ob):
            assert torch.equal(x, y)
        _assert_same_handle(torch, a, b, "free_hip")
    assert a.work_counters()["wave_iterations"] > 0          # the counting step kernel ran: the launch loop
    a.count_work(False)
    a.close(); b.close()


@pytest.mark.parametrize("clock", ["window", "episode"])
@pytest.mark.parametrize("per_env", [False, True])
def test_a_schedule_of_one_slot_is_rollout_policy(HipSim, torch_mod, per_env, clock):
    torch = torch_mod
    (a, _), (b, _) = _make(torch, HipSim, "free_hip", abi.F64), _make(torch, HipSim, "free_hip", abi.F64)
    W = _table(torch, a, 1, per_env, seed=5)
    for first in (False, True):
        ra, la, oa, (act, eps) = a.rollout_schedule(K, W, clock=clock, first_slot=3, first_episode=first, want_outputs=True,
                                                    want_terminal=True, want_reasons=True)
        assert act is None and eps is None
        rb, lb, ob = b.rollout_policy(K, W[:, 0] if per_env else W[0], first_episode=first, want_outputs=True, want_terminal=True,
                                      want_reasons=True)
        assert torch.equal(ra, rb) and torch.equal(la, lb)
        for x, y in zip(oa, ob):
            assert torch.equal(x, y)
        _assert_same_handle(torch, a, b, "T = 1")
    a.close(); b.close()


def test_noise_is_that_of_rollout_policy_and_the_actions_replay(HipSim, torch_mod):
    """sigma = 0.3, salt = 9.  T = 1: actions and noise of rollout_policy(..., sigma, salt).  T = 5: rollout(K, actions) on a twin
    replays the window bit for bit."""
    torch = torch_mod
    (a, _), (b, _) = _make(torch, HipSim, "free_hip", abi.F64), _make(torch, HipSim, "free_hip", abi.F64)
    W1 = _table(torch, a, 1, False, seed=6)
    ra, la, _, (A, E) = a.rollout_schedule(K, W1, sigma=0.3, salt=9, want_actions=True, want_noise=True)
    rb, lb, _, (Ab, Eb) = b.rollout_policy(K, W1[0], sigma=0.3, salt=9, want_actions=True, want_noise=True)
    assert torch.equal(A, Ab) and torch.equal(E, Eb) and torch.equal(ra, rb) and torch.equal(la, lb)
    assert float(E.abs().max()) > 1.0
    _assert_same_handle(torch, a, b, "noisy T = 1")
    for clock in ("window", "episode"):
        W5 = _table(torch, a, 5, True, seed=7)
        _, _, oa, (A, E) = a.rollout_schedule(K, W5, clock=clock, sigma=0.3, salt=9, want_outputs=True, want_terminal=True,
                                              want_reasons=True, want_actions=True, want_noise=True)
        ob = b.rollout(K, A, want_terminal=True, want_reasons=True)
        for x, y in zip(oa, ob):
            assert torch.equal(x, y)
        _assert_same_handle(torch, a, b, "noisy T = 5")
    a.close(); b.close()


def test_errors_behind_a_valid_handle(HipSim, torch_mod):
    torch = torch_mod
    a, _ = _make(torch, HipSim, "free_hip", abi.F64)
    from gym_os2r_amd.sim import _ptr
    lib, h, st = a._lib, a._h, a._stream()
    W = _table(torch, a, 5, False)
    sg = torch.full((2,), 0.3, dtype=a.dtype, device=a.device)
    buf, buf2 = (torch.zeros(K, N, 2, dtype=a.dtype, device=a.device) for _ in range(2))
    before, count = _everything(a), a.step_count

    def call(nsteps=K, w=W, period=5, first=0, flags=0, sigma=None, salt=0, act=None, eps=None):
        return lib.os2r_rollout_policy_scheduled(h, nsteps, _ptr(w), period, first, flags, _ptr(sigma), salt, None, None, None, None,
                                                 None, None, None, _ptr(act), _ptr(eps), st)

    for kw, word in ((dict(nsteps=0), "nsteps"), (dict(period=0), "period"), (dict(first=-1), "first_slot"), (dict(w=None), "weights"),
                     (dict(flags=64), "flag"), (dict(eps=buf), "noise_dev"), (dict(salt=9), "salt")):
        assert call(**kw) == abi.ERR_INVALID, kw
        msg = lib.os2r_last_error(h).decode()
        assert "os2r_rollout_policy_scheduled" in msg and word in msg, (kw, msg)
    for bit in (abi.POLICY_CLOCK_EPISODE, abi.POLICY_SCHEDULE_WRAP):
        assert lib.os2r_rollout_policy(h, K, _ptr(W), bit, None, None, None, None, None, None, None, st) == abi.ERR_INVALID
        assert "unknown flag" in lib.os2r_last_error(h).decode()
        assert lib.os2r_rollout_policy_noisy(h, K, _ptr(W), bit, _ptr(sg), 0, None, None, None, None, None, None, None, None, None,
                                             st) == abi.ERR_INVALID
        assert "unknown flag" in lib.os2r_last_error(h).decode()
    torch.cuda.synchronize()
    for x, y in zip(before, _everything(a)):
        assert torch.equal(x, y)
    assert a.step_count == count
    # the Python layer's own checks
    for bad in (dict(weights=W[0]), dict(weights=W.to(torch.float32)), dict(weights=W.cpu()), dict(weights=W, clock="step"),
                dict(weights=W, first_slot=-1), dict(weights=W, salt=3), dict(weights=W, want_noise=True)):
        with pytest.raises(ValueError):
            a.rollout_schedule(K, **bad)
    # what is legal: the sigma-only arguments with sigma, the recorded actions without
    assert call(sigma=sg, salt=9, act=buf, eps=buf2) == abi.OK and call(act=buf) == abi.OK
    torch.cuda.synchronize()
    assert a.step_count == count + 2 * K
    a.close()


def test_tvlqr_example_runs():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tvlqr_tracking.py"), "--envs", "64", "--steps", "20"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "tracking" in r.stdout, r.stdout
