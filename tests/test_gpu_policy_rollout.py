"""os2r_rollout_policy (include/os2r.h) on the MI355X: closed-loop rollouts with an on-device linear policy against a loop of
os2r_step calls whose actions torch computes from the returned observations, against the launch loop, against the CPU oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import make_config
from gym_os2r_amd import abi

pytestmark = pytest.mark.gpu

# the configurations of test_rollout_equals_step_by_step: fused where os2r_rollout is fused, the launch loop for fixed_hip_torque
# (in f32 too: the f32 policy kernel)
CASES = [("free_hip", abi.F64), ("fixed_hip_simple", abi.F64), ("free_hip", abi.F32), ("fixed_hip_torque", abi.F64),
         ("fixed_hip_torque", abi.F32)]
N, K = 1000, 24


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def HipSim(torch_mod):
    from gym_os2r_amd.sim import HipSim
    return HipSim


def _make(HipSim, mode, dtype, seed=5):
    """Randomised resets and parameters, TimeLimit 13, robots on the ground after 150 random steps; -> (handle, the observation
    its last step returned)."""
    cfg, _, _ = make_config(mode, "BalancingV2", True, reset_mode=abi.RESET_RANDOM, randomize_params=True, num_envs=N,
                            contact=True, seed=seed, max_episode_steps=13, dtype=dtype)
    sim = HipSim(cfg)
    for _ in range(150):
        obs = sim.step(None)[0]
    return sim, obs


def _weights(torch, sim, per_env, seed=0, scale=0.6):
    g = torch.Generator().manual_seed(seed)
    shape = (sim.N, 2, sim.D + 1) if per_env else (2, sim.D + 1)
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64)).to(sim.device, sim.dtype)


def _policy(torch, obs, W, tanh):
    """The documented order: z_j = (((b_j + W_j0*o_0) + W_j1*o_1) + ...), one tensor operation per product and per sum."""
    D = obs.shape[1]
    Wn = W.unsqueeze(0).expand(obs.shape[0], 2, D + 1) if W.dim() == 2 else W
    z = Wn[:, :, D].clone()
    for d in range(D):
        z = z + Wn[:, :, d] * obs[:, d:d + 1]
    return torch.tanh(z) if tanh else torch.clamp(z, -1.0, 1.0)


def _step_loop(torch, sim, obs, W, tanh, steps=K):
    """K calls of os2r_step with the policy computed in torch from the handle's last returned observation."""
    sim.done_reasons(True)
    out = []
    for _ in range(steps):
        o, r, d, t = sim.step(_policy(torch, obs, W, tanh))
        out.append((o, r, d, t, sim.reasons.clone()))
        obs = o
    sim.done_reasons(False)
    return out


def _sums(torch, per, first_episode):
    ret = torch.zeros_like(per[0][1])
    length = torch.zeros(ret.shape, dtype=torch.int32, device=ret.device)
    live = torch.ones(ret.shape, dtype=torch.bool, device=ret.device)
    for _, r, d, _, _ in per:
        ret = torch.where(live, ret + r, ret)
        length = length + live.to(torch.int32)
        if first_episode:
            live = live & (d == 0)
    return ret, length


def _everything(sim):
    return (sim.get_state() + sim.get_solver_state() + sim.episode_info() + (sim.get_action_history(0), sim.get_action_history(1)))


def _assert_same_handle(torch, a, b, what):
    for x, y in zip(_everything(a), _everything(b)):
        assert torch.equal(x, y), what
    assert a.step_count == b.step_count, what


@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("mode,dtype", CASES)
def test_policy_rollout_equals_a_loop_of_steps(HipSim, torch_mod, mode, dtype, per_env):
    """Clip squash: every per-step output, the returns and lengths, and the handle afterwards are those of K os2r_step calls
    whose actions torch computes from the returned observations in the documented order -- bit for bit, through randomised
    resets and TimeLimit truncations, on a batch with a tail wave."""
    torch = torch_mod
    (a, _), (b, obs_b) = _make(HipSim, mode, dtype), _make(HipSim, mode, dtype)
    W = _weights(torch, a, per_env)
    ret, length, (O, R, Dn, Tm, Wy) = a.rollout_policy(K, W, want_outputs=True, want_terminal=True, want_reasons=True)
    per = _step_loop(torch, b, obs_b, W, tanh=False)
    for k in range(K):
        for x, y in zip(per[k], (O[k], R[k], Dn[k], Tm[k], Wy[k])):
            assert torch.equal(x, y), (mode, k)
    assert int((Dn != 0).sum()) > 0                   # episodes ended (and were reset) inside the window
    r_ref, l_ref = _sums(torch, per, first_episode=False)
    assert torch.equal(ret, r_ref) and bool((length == K).all()) and torch.equal(length, l_ref)
    _assert_same_handle(torch, a, b, mode)
    hist = a.get_action_history(0)
    assert float(hist.abs().max()) <= 1.0             # policy actions are in range: nothing was clamped or counted
    a.close(); b.close()


def test_policy_rollout_tanh_squash(HipSim, torch_mod):
    """tanh squash: the kernel's tanh and torch's agree within a few ulp, the trajectories within 1e-12 over K = 24."""
    torch = torch_mod
    (a, _), (b, obs_b) = _make(HipSim, "free_hip", abi.F64), _make(HipSim, "free_hip", abi.F64)
    W = _weights(torch, a, True, seed=1)
    a.rollout_policy(1, W, tanh=True)
    per = _step_loop(torch, b, obs_b, W, tanh=True, steps=1)
    ha, hb = a.get_action_history(0), b.get_action_history(0)
    ulp = torch.finfo(torch.float64).eps * hb.abs().clamp_min(2.0 ** -1022)
    assert bool(((ha - hb).abs() <= 8 * ulp).all()), float(((ha - hb).abs() / ulp).max())
    _, _, (O, R, Dn, _, _) = a.rollout_policy(K - 1, W, tanh=True, want_outputs=True)
    per = _step_loop(torch, b, per[-1][0], W, tanh=True, steps=K - 1)
    for k in range(K - 1):
        o, r, d = per[k][:3]
        assert float(((O[k] - o).abs() / o.abs().clamp_min(1.0)).max()) < 1e-12, k
        assert torch.equal(Dn[k], d), k
    for x, y in zip(a.get_state(), b.get_state()):
        assert float(((x - y).abs() / y.abs().clamp_min(1.0)).max()) < 1e-12
    a.close(); b.close()


@pytest.mark.parametrize("mode", ["free_hip", "fixed_hip_torque"])
def test_policy_rollout_returns_without_outputs(HipSim, torch_mod, mode):
    """With every per-step output off, the returns and lengths are the sequential sums of the loop's rewards, over the whole
    window and over the first episode only; per-env weights that repeat one set give what the shared set gives, bit for bit."""
    torch = torch_mod
    (a, _), (b, obs_b) = _make(HipSim, mode, abi.F64), _make(HipSim, mode, abi.F64)
    W = _weights(torch, a, False, seed=2)
    per = _step_loop(torch, b, obs_b, W, tanh=False)
    ck = a.checkpoint()
    for first in (False, True):
        r_ref, l_ref = _sums(torch, per, first)
        a.restore(ck)
        ret, length, out = a.rollout_policy(K, W, first_episode=first)
        assert out is None
        assert torch.equal(ret, r_ref) and torch.equal(length, l_ref), (mode, first)
        if first:
            assert int((length < K).sum()) > 0 and int(length.min()) >= 1
        _assert_same_handle(torch, a, b, mode)
        a.restore(ck)
        ret2, length2, _ = a.rollout_policy(K, W.unsqueeze(0).repeat(a.N, 1, 1), first_episode=first)
        assert torch.equal(ret2, ret) and torch.equal(length2, length)
        _assert_same_handle(torch, a, b, mode)
    a.close(); b.close()


@pytest.mark.parametrize("per_env", [False, True])
def test_launch_loop_equals_fused_rollout(HipSim, torch_mod, per_env):
    """Work counters on (os2r_set_work_counters): the library takes its launch loop -- policy kernel, step launch, sums -- on a
    configuration that also has the fused kernel; both give the same results, bit for bit."""
    torch = torch_mod
    (a, _), (b, _) = _make(HipSim, "free_hip", abi.F64), _make(HipSim, "free_hip", abi.F64)
    W = _weights(torch, a, per_env, seed=3)
    a.count_work(True)
    for first in (False, True):
        ra, la, oa = a.rollout_policy(K, W, first_episode=first, want_outputs=True, want_terminal=True, want_reasons=True)
        rb, lb, ob = b.rollout_policy(K, W, first_episode=first, want_outputs=True, want_terminal=True, want_reasons=True)
        assert torch.equal(ra, rb) and torch.equal(la, lb)
        for x, y in zip(oa, ob):
            assert torch.equal(x, y)
        _assert_same_handle(torch, a, b, "free_hip")
    assert a.work_counters()["wave_iterations"] > 0          # the counting step kernel ran: the launch loop
    a.count_work(False)
    a.close(); b.close()


def test_policy_rollout_against_the_oracle(HipSim, torch_mod, oracle):
    """The balancing regime: the tests' posture controller (_pd_policy of test_gpu_parity.py without noise) is affine in the raw
    joint positions and velocities of the no_norm observation; the kernel evaluates it on its own observations for 300 env-steps,
    the oracle is driven by the same policy in numpy on its own.  Trajectories within 1e-4 relative (the closed-loop tolerance)."""
    torch = torch_mod
    n, steps, kp, kd = 64, 300, 8.0, 0.15
    cfg, _, model = make_config("free_hip", "BalancingV1", False, num_envs=n, contact=True, auto_reset=False, dtype=abi.F64,
                                seed=42)
    sim, orc = HipSim(cfg), oracle.OracleSim(cfg, threads=8)
    o_obs = orc.reset()
    sim.reset()
    q0, _ = orc.get_state()
    ih, ik = model["act_dof"]
    D = int(cfg.task.obs_dim)
    kinds, srcs = list(cfg.task.obs_kind)[:D], list(cfg.task.obs_src)[:D]

    def slot(pos, dof):
        ok = (abi.OBS_POS_RAW, abi.OBS_POS_PERIODIC_RAW) if pos else (abi.OBS_VEL_RAW,)
        return next(d for d in range(D) if kinds[d] in ok and srcs[d] == dof)

    W = np.zeros((2, D + 1))
    for j, dof in enumerate((ih, ik)):
        W[j, slot(True, dof)] = -kp / 2.5
        W[j, slot(False, dof)] = -kd / 2.5
        W[j, D] = kp * q0[dof, 0] / 2.5
    assert np.all(q0[ih] == q0[ih, 0]) and np.all(q0[ik] == q0[ik, 0])     # the fixed 'stand' reset: one set for all envs
    o_ret = np.zeros(n)
    for _ in range(steps):
        z = np.repeat(W[:, D][None, :], n, axis=0)
        for d in range(D):
            z = z + W[None, :, d] * o_obs[:, d:d + 1]
        o_obs, o_rew, _, _ = orc.step(np.clip(z, -1.0, 1.0))
        o_ret += o_rew
    ret, length, _ = sim.rollout_policy(steps, torch.as_tensor(W, device=sim.device))
    gq, gqd = (x.cpu().numpy() for x in sim.get_state())
    oq, oqd = orc.get_state()
    err = max(np.max(np.abs(gq - oq) / np.maximum(np.abs(oq), 1.0)), np.max(np.abs(gqd - oqd) / np.maximum(np.abs(oqd), 1.0)))
    assert err < 1e-4, err
    assert bool((length == steps).all())
    assert np.max(np.abs(ret.cpu().numpy() - o_ret)) <= 2.0        # a reward window edge crossed at another step, at most
    # the posture is held: hip and knee stay near the reset pose under the controller
    print(f"[policy vs oracle] rel err {err:.2e}; max |q - q0| hip {np.abs(oq[ih] - q0[ih]).max():.3f} knee "
          f"{np.abs(oq[ik] - q0[ik]).max():.3f}; mean return {o_ret.mean():.1f}")
    sim.close(); orc.close()


def test_ars_example_runs():
    """examples/ars_balancing.py, small: a few hundred environments, two iterations."""
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ars_balancing.py"), "--envs", "256", "--iters", "2",
                        "--horizon", "50"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "iteration 1" in r.stdout, r.stdout
