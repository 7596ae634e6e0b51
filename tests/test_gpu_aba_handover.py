"""The articulated-body passes of `os2r::substep` (csrc/os2r_device.hpp) after round 7: joint rotations built once per
physics iteration and the inward pass's hand-over (U = I^A S, 1/D, u) kept in registers for the compiled-in robots, rebuilt / passed
through the per-lane LDS slots for run-time models.  A wrong joint index or a missed hand-over shows at the base joint, at the last
joint and on a chain of two, so every compiled-in robot (5, 4, 3 and 2 dof) and one run-time-model robot with nq = 5 run here, in
f64 and f32, with and without ground contact where the robot has contact candidates, with and without per-env randomised
parameters, on a full wave beside a one-lane wave (N = 65) and on one lane alone (N = 1).

The oracle is the yardstick, at the tolerances tests/test_gpu_parity.py uses for the same kind of run:
  f64, device-drawn actions from the reset pose -- test_random_action_rollout_short_horizon: 1e-6 relative in q and qd (there after
       150 env-steps; 30 here);
  f32 against the fp64 oracle over a trajectory -- test_trajectory_200_steps_f32_against_f64_oracle: median 2.6e-4, p95 1e-3
       relative over the environments (there after 200 env-steps; 30 here), the oracle running the fp32 handle's sweeps-only
       solver settings as in test_one_step_f32_close_to_oracle.

What the oracle runs reach (measured on the MI355X: f64 max 1e-13 relative, f32 max 1.3e-5): they start at the reset pose, from
which no robot meets the ground within 30 env-steps, and `randomize_params` without a randomised reset leaves the per-env
parameters at their nominal values -- `contact` and `dr` select the kernel (its contact frames and scans, its per-env parameter
slots), the figures with and without them are equal.  Contact impulses go through the same kernels in the permutation test
below (fallen robots) and in tests/test_gpu_finish_dispatch.py, spread parameters in tests/test_gpu_parity.py
(test_substep_sequence_matches_oracle_with_randomised_parameters, the steady-state tests).
"""
import numpy as np
import pytest

from helpers import lying_states, make_config, perturbed_model
from gym_os2r_amd import abi

pytestmark = pytest.mark.gpu
STEPS = 30
F64_TOL = 1e-6
F32_MEDIAN, F32_P95 = 2.6e-4, 1e-3

# (task mode, run-time model?, contact): the four compiled-in robots, contact off and -- where the robot has candidates -- on;
# the 5-dof chain with every constant nudged, which no compiled-in table matches (RtModel kernels)
ROBOTS = [("free_hip", False, True), ("free_hip", False, False), ("fixed_hip", False, True), ("fixed_hip", False, False),
          ("fixed", False, True), ("fixed", False, False), ("simple", False, False),
          ("free_hip", True, True), ("free_hip", True, False)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def HipSim(torch_mod):
    from gym_os2r_amd.sim import HipSim
    return HipSim


def _err(a, b):
    """per environment: the largest relative deviation over the dofs"""
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0), axis=0)


def _configs(mode, runtime, contact, dr, n, dtype):
    """-> (the handle's config, the oracle's config, the model)"""
    reward = "StraightV1" if mode == "simple" else "BalancingV2"
    over = perturbed_model(mode, np.random.default_rng(71)) if runtime else None
    kw = dict(num_envs=n, contact=contact, auto_reset=False, randomize_params=dr, seed=11, model_overrides=over)
    cfg, _, model = make_config(mode, reward, True, dtype=dtype, **kw)
    if dtype == abi.F64:
        return cfg, cfg, model
    # the fp32 handle runs the sweeps-only solver: the oracle is given the same settings, so that what is compared is the arithmetic
    cfg64, _, _ = make_config(mode, reward, True, dtype=abi.F64, pgs_exact=0, pgs_iters=cfg.pgs_iters, pgs_tol=cfg.pgs_tol, **kw)
    assert cfg.pgs_exact == 0
    return cfg, cfg64, model


@pytest.mark.parametrize("n", [65, 1])
@pytest.mark.parametrize("dr", [False, True])
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("mode,runtime,contact", ROBOTS)
def test_thirty_env_steps_match_the_oracle(HipSim, torch_mod, oracle, mode, runtime, contact, dtype, dr, n):
    cfg, cfg_orc, model = _configs(mode, runtime, contact, dr, n, dtype)
    assert model["nq"] == {"free_hip": 5, "fixed_hip": 4, "fixed": 3, "simple": 2}[mode]
    sim, orc = HipSim(cfg), oracle.OracleSim(cfg_orc, threads=4)
    try:
        for _ in range(STEPS):
            sim.step(None); orc.step(None)            # on-device Philox actions against the oracle's Philox
        q, qd = (x.cpu().numpy().astype(np.float64) for x in sim.get_state())
        oq, oqd = orc.get_state()
        a_gpu, a_orc = sim.get_action_history(0).cpu().numpy(), orc.get_action_history(0)
    finally:
        sim.close(); orc.close()
    err = np.maximum(_err(q, oq), _err(qd, oqd))
    print(f"[aba hand-over] {mode}{' (run-time model)' if runtime else ''} contact={contact} dr={dr} n={n} "
          f"{'f64' if dtype == abi.F64 else 'f32'}: rel err median {np.median(err):.2e} p95 {np.quantile(err, 0.95):.2e} max {err.max():.2e}")
    assert np.isfinite(q).all() and np.isfinite(qd).all() and np.isfinite(oq).all() and np.isfinite(oqd).all()
    assert np.abs(oqd).max() > 0                      # the robots moved
    if dtype == abi.F64:
        assert np.array_equal(a_gpu, a_orc)           # identical action streams
        assert err.max() < F64_TOL, err.max()
    else:
        assert np.median(err) < F32_MEDIAN and np.quantile(err, 0.95) < F32_P95, (np.median(err), np.quantile(err, 0.95))


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("mode,runtime", [("free_hip", False), ("fixed", False), ("simple", False), ("free_hip", True)])
def test_permuted_environments_give_permuted_results(HipSim, torch_mod, mode, runtime, dtype):
    """Lanes must not see each other: 128 environments -- fallen robots, per-env parameters -- stepped in a permuted order through
    `copy_envs_from` give the permuted results, bit for bit."""
    n = 128
    cfg, _, model = _configs(mode, runtime, mode != "simple", True, n, dtype)
    rng = np.random.default_rng(72)
    q, qd = lying_states(model, n, rng)
    perm = rng.permutation(n)
    a, b = HipSim(cfg), HipSim(cfg)
    try:
        a.set_state(q, qd)
        for _ in range(2):
            a.step(torch_mod.as_tensor(rng.uniform(-1, 1, (n, 2))))
        idx = torch_mod.as_tensor(perm.astype(np.int32), device=a.device)
        b.copy_envs_from(a, idx, check=True)
        for _ in range(5):
            act = rng.uniform(-1, 1, (n, 2))
            outs_a = a.step(torch_mod.as_tensor(act))
            outs_b = b.step(torch_mod.as_tensor(np.ascontiguousarray(act[perm])))
            for xa, xb in zip(outs_a[:3], outs_b[:3]):            # obs, reward, done
                assert torch_mod.equal(xa[idx.long()], xb)
        for xa, xb in zip(a.get_state(), b.get_state()):
            assert torch_mod.equal(xa[:, idx.long()], xb)
        assert bool((a.get_state()[1] != 0).any())
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_rollout_of_three_equals_three_steps(HipSim, torch_mod, dtype):
    """os2r_rollout with K = 3 (the fused kernel: the step loop around the same `substep`) against three os2r_step calls on the
    monopod, bit for bit: outputs of every step and the state afterwards."""
    n, K = 65, 3
    def make():
        cfg, _, _ = make_config("free_hip", "BalancingV2", True, reset_mode=abi.RESET_RANDOM, randomize_params=True, num_envs=n,
                                contact=True, seed=5, dtype=dtype)
        return HipSim(cfg)
    a, b = make(), make()
    try:
        for _ in range(2):
            per = [a.step(None) for _ in range(K)]
            O, R, Dn, Tm, _ = b.rollout(K, None, want_terminal=True)
            for k in range(K):
                for x, y in zip(per[k], (O[k], R[k], Dn[k], Tm[k])):
                    assert torch_mod.equal(x, y), k
            for x, y in zip(a.get_state() + a.get_solver_state(), b.get_state() + b.get_solver_state()):
                assert torch_mod.equal(x, y)
        assert bool((a.get_state()[1] != 0).any())
    finally:
        a.close(); b.close()
