"""os2r_rollout_policy_noisy (include/os2r.h) on the MI355X: closed-loop rollouts with Gaussian exploration noise on the linear
policy's pre-squash output.  Checked by composition: a noisy rollout equals the open-loop os2r_rollout of the actions it reports,
bit for bit; the actions equal the documented formula evaluated in torch, bit for bit; the noise is Philox stream 5 of the CPU
oracle through Box-Muller, keyed by (seed, global environment index, step counter, salt)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import make_config
from gym_os2r_amd import abi

pytestmark = pytest.mark.gpu

# the configurations of tests/test_gpu_policy_rollout.py: the fused f64 and f32 kernels, the launch loop (fixed_hip_torque) in both
CASES = [("free_hip", abi.F64), ("fixed_hip_simple", abi.F64), ("free_hip", abi.F32), ("fixed_hip_torque", abi.F64),
         ("fixed_hip_torque", abi.F32)]
N, K = 1000, 24
SALT = 0x9E3779B9


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def HipSim(torch_mod):
    from gym_os2r_amd.sim import HipSim
    return HipSim


def _make(HipSim, mode, dtype, seed=5, n=N, env_offset=0, binding=None):
    """Randomised resets and parameters, TimeLimit 13, robots on the ground after 150 random steps (step counter 150);
    -> (handle, the observation its last step returned)."""
    cfg, _, _ = make_config(mode, "BalancingV2", True, reset_mode=abi.RESET_RANDOM, randomize_params=True, num_envs=n,
                            contact=True, seed=seed, max_episode_steps=13, dtype=dtype, env_offset=env_offset)
    sim = HipSim(cfg, binding=binding)
    for _ in range(150):
        obs = sim.step(None)[0]
    return sim, obs


def _weights(torch, sim, per_env, seed=0, scale=0.6):
    g = torch.Generator().manual_seed(seed)
    shape = (sim.N, 2, sim.D + 1) if per_env else (2, sim.D + 1)
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64)).to(sim.device, sim.dtype)


def _sigma(torch, sim, per_env):
    """About 0.3: with weights of scale 0.6 both clipped and unclipped actions occur."""
    if not per_env:
        return torch.tensor([0.3, 0.25], dtype=sim.dtype, device=sim.device)
    g = torch.Generator().manual_seed(11)
    return (0.2 + 0.2 * torch.rand((sim.N, 2), generator=g, dtype=torch.float64)).to(sim.device, sim.dtype)


def _presquash(torch, obs, W, sigma, eps):
    """The documented order: z_j = (((b_j + W_j0*o_0) + W_j1*o_1) + ...), y_j = z_j + (sigma_j * eps_j): one tensor operation
    per product and per sum."""
    D = obs.shape[1]
    Wn = W.unsqueeze(0).expand(obs.shape[0], 2, D + 1) if W.dim() == 2 else W
    z = Wn[:, :, D].clone()
    for d in range(D):
        z = z + Wn[:, :, d] * obs[:, d:d + 1]
    if sigma is None:
        return z
    sg = sigma.unsqueeze(0).expand(obs.shape[0], 2) if sigma.dim() == 1 else sigma
    p = sg * eps
    return z + p


def _sums(torch, R, Dn, first_episode):
    ret = torch.zeros_like(R[0])
    length = torch.zeros(ret.shape, dtype=torch.int32, device=ret.device)
    live = torch.ones(ret.shape, dtype=torch.bool, device=ret.device)
    for k in range(R.shape[0]):
        ret = torch.where(live, ret + R[k], ret)
        length = length + live.to(torch.int32)
        if first_episode:
            live = live & (Dn[k] == 0)
    return ret, length


def _everything(sim):
    return (sim.get_state() + sim.get_solver_state() + sim.episode_info() + (sim.get_action_history(0), sim.get_action_history(1)))


def _assert_same_handle(torch, a, b, what):
    for x, y in zip(_everything(a), _everything(b)):
        assert torch.equal(x, y), what
    assert a.step_count == b.step_count, what


ALL = dict(want_outputs=True, want_terminal=True, want_reasons=True, want_actions=True, want_noise=True)


@pytest.mark.parametrize("per_env_sigma", [False, True])
@pytest.mark.parametrize("mode,dtype", CASES)
def test_noisy_rollout_equals_the_open_loop_rollout_of_its_actions(HipSim, torch_mod, mode, dtype, per_env_sigma):
    """Replay: os2r_rollout on a twin handle with the actions the noisy rollout reports gives every per-step output and the same
    handle afterwards, bit for bit, through randomised resets and TimeLimit truncations, on a batch with a tail wave; the returns
    and lengths are the step-ordered sums of the rewards, over the window and over the first episode."""
    torch = torch_mod
    (a, _), (b, _) = _make(HipSim, mode, dtype), _make(HipSim, mode, dtype)
    W, sg = _weights(torch, a, per_env_sigma), _sigma(torch, a, per_env_sigma)
    ck = a.checkpoint()
    ret, length, (O, R, Dn, Tm, Wy), (A, E) = a.rollout_policy(K, W, sigma=sg, salt=SALT, **ALL)
    assert A.shape == (K, N, 2) and E.shape == (K, N, 2) and A.dtype == a.dtype and E.dtype == a.dtype
    Ob, Rb, Db, Tb, Wb = b.rollout(K, actions=A, want_terminal=True, want_reasons=True)
    for name, x, y in (("obs", O, Ob), ("reward", R, Rb), ("done", Dn, Db), ("terminal", Tm, Tb), ("reasons", Wy, Wb)):
        assert torch.equal(x, y), (mode, name)
    _assert_same_handle(torch, a, b, mode)
    assert int((Dn != 0).sum()) > 0                          # episodes ended (and were reset) inside the window
    clipped = int((A.abs() == 1.0).sum())
    assert 0 < clipped < A.numel(), clipped                  # both clipped and unclipped actions occur
    assert float(A.abs().max()) <= 1.0
    r_ref, l_ref = _sums(torch, R, Dn, first_episode=False)
    assert torch.equal(ret, r_ref) and bool((length == K).all()) and torch.equal(length, l_ref)
    a.restore(ck)
    ret1, length1, out1, (A1, E1) = a.rollout_policy(K, W, sigma=sg, salt=SALT, first_episode=True, **ALL)
    assert torch.equal(A1, A) and torch.equal(E1, E) and torch.equal(out1[1], R) and torch.equal(out1[2], Dn)
    r_ref, l_ref = _sums(torch, R, Dn, first_episode=True)
    assert torch.equal(ret1, r_ref) and torch.equal(length1, l_ref)
    assert int((length1 < K).sum()) > 0 and int(length1.min()) >= 1
    _assert_same_handle(torch, a, b, mode)
    a.close(); b.close()


@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("mode,dtype", CASES)
def test_actions_equal_the_documented_formula(HipSim, torch_mod, mode, dtype, per_env):
    """Clip squash: A[k] == clamp(z(O_prev[k], W) + sigma * E[k], -1, 1) evaluated in torch, one operation per product and sum,
    bit for bit; O_prev[k] is the observation before step k (post-reset after an auto-reset)."""
    torch = torch_mod
    a, obs0 = _make(HipSim, mode, dtype)
    W, sg = _weights(torch, a, per_env, seed=4), _sigma(torch, a, per_env)
    _, _, (O, _, _, _, _), (A, E) = a.rollout_policy(K, W, sigma=sg, salt=3, want_outputs=True, want_actions=True, want_noise=True)
    for k in range(K):
        prev = obs0 if k == 0 else O[k - 1]
        ref = torch.clamp(_presquash(torch, prev, W, sg, E[k]), -1.0, 1.0)
        assert torch.equal(A[k], ref), (mode, k, float((A[k] - ref).abs().max()))
    a.close()


def test_tanh_squash_within_8_ulp(HipSim, torch_mod):
    """tanh squash: the kernel's tanh and torch's agree within 8 ulp (the allowance of test_policy_rollout_tanh_squash for the same
    two routines) on the same pre-squash value."""
    torch = torch_mod
    a, obs0 = _make(HipSim, "free_hip", abi.F64)
    W, sg = _weights(torch, a, True, seed=1), _sigma(torch, a, True)
    _, _, _, (A, E) = a.rollout_policy(1, W, sigma=sg, tanh=True, want_actions=True, want_noise=True)
    ref = torch.tanh(_presquash(torch, obs0, W, sg, E[0]))
    ulp = torch.finfo(torch.float64).eps * ref.abs().clamp_min(2.0 ** -1022)
    worst = float(((A[0] - ref).abs() / ulp).max())
    print(f"[noisy tanh] max |A - tanh(y)| = {worst:.2f} ulp")
    assert worst <= 8.0, worst
    a.close()


def _box_muller(oracle, seed, genv, c, salt):
    """eps of os2r_rollout_policy_noisy for global environment indices `genv` at step counter c: Philox counter
    words c0 = low 32 bits of c, c1 = (c >> 32) ^ salt, stream 5; Box-Muller in numpy."""
    c0, c1 = c & 0xFFFFFFFF, ((c >> 32) ^ salt) & 0xFFFFFFFF
    u = np.array([oracle.uniform2(seed, int(g), abi.STREAM_POLICY_NOISE, c0, c1) for g in genv])
    r = np.sqrt(-2.0 * np.log(1.0 - u[:, 0]))
    th = 6.283185307179586476925286766559 * u[:, 1]
    return np.stack([r * np.cos(th), r * np.sin(th)], axis=1)


# Device libm and numpy differ in the last bits of log, sin and cos.  Measured on the MI355X: max |dE| / max(|E|, 1) = 2.454e-16 over
# the 3 x 1000 x 2 values below; the bound is 8 x that (anything above 1e-12 would be a wrong stream or a float evaluation).
NOISE_STREAM_TOL = 8 * 2.454e-16


def test_noise_is_stream_5_of_the_counter_rng(HipSim, torch_mod, oracle):
    """f64: E[k, e] against Box-Muller on the oracle's uniform2(seed, env_offset + e, 5, c0, c1) for all e at three step
    counters -- the first and last step of a window, and one above 2^32 set through the step_count setter -- with a non-zero
    env_offset and salt.  f32: the same noise rounded once to float, bit for bit."""
    torch = torch_mod
    seed, off = 5, 777
    a, _ = _make(HipSim, "free_hip", abi.F64, seed=seed, env_offset=off)
    f, _ = _make(HipSim, "free_hip", abi.F32, seed=seed, env_offset=off)
    W, Wf = _weights(torch, a, False), _weights(torch, f, False)
    genv = off + np.arange(N)
    worst = 0.0
    assert a.step_count == 150 and f.step_count == 150
    E = a.rollout_policy(K, W, sigma=0.3, salt=SALT, want_noise=True)[3][1]
    Ef = f.rollout_policy(K, Wf, sigma=0.3, salt=SALT, want_noise=True)[3][1]
    assert Ef.dtype == torch.float32 and torch.equal(Ef, E.to(torch.float32))
    for k in (0, K - 1):
        ref = _box_muller(oracle, seed, genv, 150 + k, SALT)
        worst = max(worst, float(np.max(np.abs(E[k].cpu().numpy() - ref) / np.maximum(np.abs(ref), 1.0))))
    big = 3 * 2 ** 32 + 17
    a.step_count = big
    f.step_count = big
    E = a.rollout_policy(2, W, sigma=0.3, salt=SALT, want_noise=True)[3][1]
    Ef = f.rollout_policy(2, Wf, sigma=0.3, salt=SALT, want_noise=True)[3][1]
    assert torch.equal(Ef, E.to(torch.float32))
    assert a.step_count == big + 2
    ref = _box_muller(oracle, seed, genv, big + 1, SALT)
    worst = max(worst, float(np.max(np.abs(E[1].cpu().numpy() - ref) / np.maximum(np.abs(ref), 1.0))))
    # (the high word matters: without it the counter words would be those of step 18)
    assert np.max(np.abs(_box_muller(oracle, seed, genv, 18, SALT) - ref)) > 1.0
    print(f"[noise stream] max |dE| / max(|E|, 1) = {worst:.3e} (bound {NOISE_STREAM_TOL:.3e})")
    assert worst <= NOISE_STREAM_TOL <= 1e-12, worst
    a.close(); f.close()


@pytest.mark.parametrize("mode,dtype", [("free_hip", abi.F64), ("free_hip", abi.F32), ("fixed_hip_torque", abi.F64)])
def test_sigma_zero_is_the_deterministic_policy(HipSim, torch_mod, mode, dtype):
    """sigma = 0 (a float, a shared pair, per-env zeros) gives the actions, outputs, returns and final handle of rollout_policy
    without sigma, bit for bit, and still reports the noise it drew; sigma=None returns today's 3-tuple."""
    torch = torch_mod
    (a, obs0), (b, _) = _make(HipSim, mode, dtype), _make(HipSim, mode, dtype)
    W = _weights(torch, a, True, seed=6)
    ck = a.checkpoint()
    E_ref = a.rollout_policy(K, W, sigma=0.3, want_noise=True)[3][1]
    det = b.rollout_policy(K, W, want_outputs=True, want_terminal=True, want_reasons=True)
    assert isinstance(det, tuple) and len(det) == 3 and len(det[2]) == 5
    assert b.rollout_policy(1, W)[2] is None and len(b.rollout_policy(1, W, sigma=None)) == 3
    for sg in (0.0, torch.zeros(2, dtype=a.dtype, device=a.device), torch.zeros(N, 2, dtype=a.dtype, device=a.device)):
        a.restore(ck)
        ret, length, out, (A, E) = a.rollout_policy(K, W, sigma=sg, **ALL)
        assert torch.equal(ret, det[0]) and torch.equal(length, det[1])
        for x, y in zip(out, det[2]):
            assert torch.equal(x, y), mode
        assert torch.equal(E, E_ref) and float(E.abs().max()) > 3.0
        for k in range(K):
            prev = obs0 if k == 0 else out[0][k - 1]
            assert torch.equal(A[k], torch.clamp(_presquash(torch, prev, W, None, None), -1.0, 1.0)), k
    a.rollout_policy(2, W, sigma=0.0)
    _assert_same_handle(torch, a, b, mode)
    a.close(); b.close()


def test_noise_is_keyed_by_global_index_counter_and_salt(HipSim, torch_mod):
    torch = torch_mod
    mode, dtype = "free_hip", abi.F64
    a, _ = _make(HipSim, mode, dtype)
    W, sg = _weights(torch, a, True, seed=7), _sigma(torch, a, True)
    ck = a.checkpoint()
    ret, length, out, (A, E) = a.rollout_policy(K, W, sigma=sg, salt=SALT, **ALL)
    # two shards of 500 environments reproduce the 1000-environment handle, slice for slice
    for off in (0, 500):
        s, _ = _make(HipSim, mode, dtype, n=500, env_offset=off)
        sl = slice(off, off + 500)
        r2, l2, out2, (A2, E2) = s.rollout_policy(K, W[sl].contiguous(), sigma=sg[sl].contiguous(), salt=SALT, **ALL)
        assert torch.equal(A2, A[:, sl]) and torch.equal(E2, E[:, sl]), off
        assert torch.equal(r2, ret[sl]) and torch.equal(l2, length[sl])
        for x, y in zip(out2, out):
            assert torch.equal(x, y[:, sl]), off
        s.close()
    # a restored checkpoint and the same call reproduce the window
    end = a.checkpoint()
    a.restore(ck)
    _, _, _, (A3, E3) = a.rollout_policy(K, W, sigma=sg, salt=SALT, want_actions=True, want_noise=True)
    assert torch.equal(A3, A) and torch.equal(E3, E)
    # another salt: independent noise at the same step counters -- no element of 48 000 doubles is equal
    a.restore(ck)
    _, _, _, (_, E4) = a.rollout_policy(K, W, sigma=sg, salt=SALT + 1, want_noise=True)
    assert E4.numel() == 48000 and int((E4 == E).sum()) == 0
    a.restore(ck)
    _, _, _, (_, E5) = a.rollout_policy(K, W, sigma=sg, want_noise=True)          # salt 0
    assert int((E5 == E).sum()) == 0 and int((E5 == E4).sum()) == 0
    # two consecutive windows of K / 2 steps equal one window of K
    a.restore(ck)
    h = K // 2
    _, _, o1, (A6, E6) = a.rollout_policy(h, W, sigma=sg, salt=SALT, **ALL)
    _, _, o2, (A7, E7) = a.rollout_policy(K - h, W, sigma=sg, salt=SALT, **ALL)
    assert torch.equal(torch.cat([A6, A7]), A) and torch.equal(torch.cat([E6, E7]), E)
    for x, y, z in zip(o1, o2, out):
        assert torch.equal(torch.cat([x, y]), z)
    for x, y in zip((end["q"], end["qd"], end["solver_lambda"], end["hist0"], end["hist1"], end["steps"], end["episode"]),
                    a.get_state() + (a.get_solver_state()[0], a.get_action_history(0), a.get_action_history(1)) + a.episode_info()[:2]):
        assert torch.equal(x, y)
    a.close()


def test_noise_distribution(HipSim, torch_mod):
    """409 600 values (N = 4096, K = 50, f64, seed 5, env_offset 0, salt 0, step counter 150): moments, cross products and the
    Kolmogorov distance to Phi, each within five standard errors of the statistic under N(0, 1) (Kolmogorov: the 1e-6 quantile,
    2.63 / sqrt(n)).  Derived bounds; the specified generator on the CPU sits well inside all of them (mean -1.5e-5, var - 1
    -2.1e-3, third 2.7e-3, fourth - 3 2.7e-3, cross products -5.8e-4, 8.7e-5, 5.6e-4, Kolmogorov 9.4e-4)."""
    torch = torch_mod
    n_env, k_steps = 4096, 50
    a, _ = _make(HipSim, "free_hip", abi.F64, seed=5, n=n_env)
    assert a.step_count == 150
    E = a.rollout_policy(k_steps, _weights(torch, a, False), sigma=0.3, want_noise=True)[3][1]
    x = E.flatten()
    n = x.numel()
    assert n == 409600
    stats = {"mean": (float(x.mean()), 5 / math.sqrt(n)),
             "var - 1": (float((x * x).mean() - x.mean() ** 2) - 1.0, 5 * math.sqrt(2 / n)),
             "third moment": (float((x ** 3).mean()), 5 * math.sqrt(15 / n)),
             "fourth moment - 3": (float((x ** 4).mean()) - 3.0, 5 * math.sqrt(96 / n)),
             "hip x knee": (float((E[..., 0] * E[..., 1]).mean()), 5 / math.sqrt(n / 2)),
             "step k x step k+1": (float((E[:-1] * E[1:]).mean()), 5 / math.sqrt(n / 2)),
             "env e x env e+1": (float((E[:, :-1] * E[:, 1:]).mean()), 5 / math.sqrt(n / 2))}
    xs = torch.sort(x).values
    F = 0.5 * (1.0 + torch.erf(xs / math.sqrt(2.0)))
    i = torch.arange(1, n + 1, dtype=torch.float64, device=x.device)
    stats["Kolmogorov distance"] = (float(torch.maximum((i / n - F).max(), (F - (i - 1) / n).max())), 2.63 / math.sqrt(n))
    for name, (v, bound) in stats.items():
        print(f"[noise distribution] {name:<20} {v:+.3e}  (bound {bound:.3e})")
    print(f"[noise distribution] max |eps| {float(x.abs().max()):.3f}, beyond 3 sigma {100 * float((x.abs() > 3).double().mean()):.5f} %")
    for name, (v, bound) in stats.items():
        assert abs(v) <= bound, (name, v, bound)
    a.close()


def test_noisy_actions_are_never_counted_as_violations(HipSim, torch_mod):
    torch = torch_mod
    a, _ = _make(HipSim, "free_hip", abi.F64)
    b, _ = _make(HipSim, "fixed_hip_torque", abi.F64)          # the launch loop hands the actions to a step launch
    for sim in (a, b):
        before = torch.zeros(1, dtype=torch.int32, device=sim.device)
        after = torch.full((1,), -1, dtype=torch.int32, device=sim.device)
        sim.action_violations_into(before, clear=False)
        _, _, _, (A, _) = sim.rollout_policy(K, _weights(torch, sim, False), sigma=2.0, want_actions=True)
        sim.action_violations_into(after, clear=False)
        torch.cuda.synchronize()
        assert int(after) == int(before)
        assert float(A.abs().max()) == 1.0 and int((A.abs() == 1.0).sum()) > A.numel() // 4
        sim.close()


def test_argument_checks(HipSim, torch_mod):
    """HipSim raises ValueError before the library is called; the library itself refuses what the binding would have let through."""
    torch = torch_mod
    a, _ = _make(HipSim, "free_hip", abi.F64)
    W = _weights(torch, a, False)
    ck = a.checkpoint()
    count = a.step_count
    bad = [dict(sigma=torch.zeros(3, dtype=a.dtype, device=a.device)),
           dict(sigma=torch.zeros(2, N, dtype=a.dtype, device=a.device)),
           dict(sigma=torch.zeros(N - 1, 2, dtype=a.dtype, device=a.device)),
           dict(sigma=torch.zeros(2, dtype=torch.float32, device=a.device)),
           dict(sigma=torch.zeros(2, dtype=a.dtype)),                      # on the host
           dict(sigma=[0.1, 0.1]),
           dict(sigma=0.1, salt=-1), dict(sigma=0.1, salt=2 ** 32),
           dict(want_actions=True), dict(want_noise=True), dict(salt=5)]
    for kw in bad:
        with pytest.raises(ValueError):
            a.rollout_policy(K, W, **kw)
    for n in (-1, 0):
        with pytest.raises(ValueError):
            a.rollout_policy(n, W, sigma=0.1)
    # the C-ABI behind it: null sigma, nsteps < 1, null weights, an unknown flag bit; os2r_rollout_policy refuses the new bit
    lib, h, vp = a._lib, a._h, ctypes.c_void_p
    w, sg = vp(W.data_ptr()), vp(torch.zeros(2, dtype=a.dtype, device=a.device).data_ptr())
    rest = (None,) * 9 + (a._stream(),)
    for args, msg in (((h, 1, w, 0, None, 0), "null sigma"), ((h, 0, w, 0, sg, 0), "nsteps"), ((h, 1, None, 0, sg, 0), "null weights"),
                      ((h, 1, w, 16, sg, 0), "unknown flag")):
        assert lib.os2r_rollout_policy_noisy(*args, *rest) == abi.ERR_INVALID
        assert msg in lib.os2r_last_error(h).decode()
    assert lib.os2r_rollout_policy(h, 1, w, abi.POLICY_SIGMA_PER_ENV, None, None, None, None, None, None, None,
                                   a._stream()) == abi.ERR_INVALID
    assert "unknown flag" in lib.os2r_last_error(h).decode()
    assert a.step_count == count
    for x, y in zip((ck["q"], ck["qd"]), a.get_state()):
        assert torch.equal(x, y)                                           # nothing ran
    a.close()


def test_both_bindings_and_both_paths_agree(HipSim, torch_mod):
    """The pybind11 binding gives what ctypes gives; with work counters on the library takes its launch loop on a configuration
    that has the fused kernel: same results, bit for bit."""
    torch = torch_mod
    (a, _), (b, _), (c, _) = (_make(HipSim, "free_hip", abi.F64), _make(HipSim, "free_hip", abi.F64, binding="pybind11"),
                              _make(HipSim, "free_hip", abi.F64))
    W, sg = _weights(torch, a, True, seed=3), _sigma(torch, a, True)
    c.count_work(True)
    ra = a.rollout_policy(K, W, sigma=sg, salt=SALT, first_episode=True, **ALL)
    for other in (b, c):
        ro = other.rollout_policy(K, W, sigma=sg, salt=SALT, first_episode=True, **ALL)
        assert torch.equal(ra[0], ro[0]) and torch.equal(ra[1], ro[1])
        for x, y in zip(ra[2] + ra[3], ro[2] + ro[3]):
            assert torch.equal(x, y)
        _assert_same_handle(torch, a, other, other.binding)
    assert c.work_counters()["wave_iterations"] > 0           # the counting step kernel ran: the launch loop
    c.count_work(False)
    a.close(); b.close(); c.close()


def test_reinforce_example_runs():
    """examples/reinforce_balancing.py, small: a few hundred environments, two iterations.  Nothing about learning progress."""
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "reinforce_balancing.py"), "--envs", "256", "--iters", "2",
                        "--horizon", "50"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "iteration 1" in r.stdout, r.stdout
