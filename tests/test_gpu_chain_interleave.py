"""Round 8 (docs/studies/round8_chain_interleave.md): in `os2r::substep` (csrc/os2r_device.hpp) the incremental sin/cos of the joints
advance together, the candidate scan of the compiled-in robots computes the heights of a chunk's four candidates before it sums, and
the row set-up of those robots takes the factor's rows from registers instead of their LDS mirror.  A joint or candidate index that
went wrong in the reordering, or a row of the factor taken from the wrong register, shows at the base joint, at the last joint and
on a chain of two, so the four compiled-in robots (5, 4, 3 and 2 dof) and one run-time-model robot with nq = 5 (whose kernels keep
the parent's scan and mirror) run here, in f64 and f32, with ground contact, with and without per-env parameters (spread, not
nominal), on a full wave beside a one-lane wave (N = 65) and on one lane alone (N = 1).

The start state is one in which the changed code runs: fallen robots (`helpers.lying_states`, the state the permutation check of
tests/test_gpu_aba_handover.py uses; 0 env-steps of falling are needed, the robots lie on the ground at the start), the solver
state cleared on both sides by `set_state`.  Checked on the CPU oracle for the seed used here: 61 / 62 / 60 of the 65 free_hip /
fixed_hip / fixed robots (60 of the run-time model's) have a body inside the contact band at the start and after the first env-step,
58-59 of 65 after the 30 env-steps, in f64 and f32, with and without per-env parameters; the single robot of every N = 1 case has
throughout.  The test itself asserts it: the counting variant of the step kernel (f64, `count_work`) on the same
state must have scanned candidates and set up contact rows (`scanned_bodies > 0`, `row_bodies > 0`), and the oracle's end state
must have a body in the contact band.  Both sin/cos branches run by construction: the first physics iteration of an env-step
evaluates them in full, the other nine turn them.

The oracle is the yardstick, at the tolerances tests/test_gpu_parity.py uses for the same kind of run:
  f64, device-drawn actions, robots flailing on the ground -- test_random_action_rollout_short_horizon: 1e-6 relative in q and qd;
  f32 against the fp64 oracle over a trajectory with contact -- test_trajectory_200_steps_f32_against_f64_oracle: median 2.6e-4,
       p95 1e-3 relative over the environments, the oracle running the fp32 handle's sweeps-only solver settings as in
       test_one_step_f32_close_to_oracle.
"""
import numpy as np
import pytest

from helpers import lying_states, make_config, perturbed_model
from gym_os2r_amd import abi

pytestmark = pytest.mark.gpu
STEPS = 30
F64_TOL = 1e-6
F32_MEDIAN, F32_P95 = 2.6e-4, 1e-3

# (task mode, run-time model?): the four compiled-in robots; the 5-dof chain with every constant nudged (RtModel kernels)
ROBOTS = [("free_hip", False), ("fixed_hip", False), ("fixed", False), ("simple", False), ("free_hip", True)]


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


def configs(mode, runtime, dr, n, dtype):
    """-> (the handle's config, the oracle's config, the f64 config of the counting twin, the model)"""
    reward = "StraightV1" if mode == "simple" else "BalancingV2"
    over = perturbed_model(mode, np.random.default_rng(81)) if runtime else None
    kw = dict(num_envs=n, contact=True, auto_reset=False, randomize_params=dr, seed=13, model_overrides=over)
    cfg, _, model = make_config(mode, reward, True, dtype=dtype, **kw)
    cfg64, _, _ = make_config(mode, reward, True, dtype=abi.F64, **kw)
    if dtype == abi.F64:
        return cfg, cfg, cfg64, model
    # the fp32 handle runs the sweeps-only solver: the oracle is given the same settings, so that what is compared is the arithmetic
    cfg_orc, _, _ = make_config(mode, reward, True, dtype=abi.F64, pgs_exact=0, pgs_iters=cfg.pgs_iters, pgs_tol=cfg.pgs_tol, **kw)
    assert cfg.pgs_exact == 0
    return cfg, cfg_orc, cfg64, model


def start(model, dr, n, dtype):
    """Fallen robots and, with per-env parameters, a spread of them; values an fp32 handle holds exactly. -> (q, qd, params)"""
    rng = np.random.default_rng(82)
    q, qd = lying_states(model, 65, rng)
    q, qd = q[:, :n], qd[:, :n]
    nq = model["nq"]
    params = {}
    if dr:
        params = {abi.PARAM_MASS_SCALE: rng.uniform(0.8, 1.2, (nq, 65)), abi.PARAM_DAMPING: rng.uniform(0.008, 0.012, (nq, 65)),
                  abi.PARAM_FRICTION: rng.uniform(0.01, 0.05, (nq, 65)), abi.PARAM_MU: 0.33 * rng.uniform(0.8, 1.2, (nq, 65))}
        params = {f: v[:, :n] for f, v in params.items()}
    if dtype == abi.F32:
        q, qd = q.astype(np.float32).astype(np.float64), qd.astype(np.float32).astype(np.float64)
        params = {f: v.astype(np.float32).astype(np.float64) for f, v in params.items()}
    return np.ascontiguousarray(q), np.ascontiguousarray(qd), {f: np.ascontiguousarray(v) for f, v in params.items()}


def touching(oracle, cfg, model, oq, oqd):
    """how many environments of the oracle's state have a body inside the contact band"""
    nq = model["nq"]
    count = 0
    for e in range(oq.shape[1]):
        _, _, rw, ow = oracle.dynamics(cfg.model, oq[:, e], oqd[:, e], np.zeros(nq))
        count += bool(oracle.contact_points(cfg.model, rw, ow, cfg.contact_margin)[0].any())
    return count


@pytest.mark.parametrize("n", [65, 1])
@pytest.mark.parametrize("dr", [False, True])
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("mode,runtime", ROBOTS)
def test_thirty_env_steps_on_the_ground_match_the_oracle(HipSim, torch_mod, oracle, mode, runtime, dtype, dr, n):
    cfg, cfg_orc, cfg64, model = configs(mode, runtime, dr, n, dtype)
    assert model["nq"] == {"free_hip": 5, "fixed_hip": 4, "fixed": 3, "simple": 2}[mode]
    can_touch = len(model["cand_body"]) > 0
    counting = can_touch and not runtime                  # the counting variant exists for the compiled-in robots with candidates
    q0, qd0, params = start(model, dr, n, dtype)
    sim, orc = HipSim(cfg), oracle.OracleSim(cfg_orc, threads=4)
    cnt = HipSim(cfg64) if counting else None
    try:
        for h in (sim, orc) + ((cnt,) if counting else ()):
            for f, v in params.items():
                h.set_params(f, v)
            h.set_state(q0, qd0)                          # (clears the solver state)
        if counting:
            cnt.count_work(True)
        for _ in range(STEPS):
            sim.step(None); orc.step(None)                # on-device Philox actions against the oracle's Philox
            if counting:
                cnt.step(None)
        q, qd = (x.cpu().numpy().astype(np.float64) for x in sim.get_state())
        oq, oqd = orc.get_state()
        a_gpu, a_orc = sim.get_action_history(0).cpu().numpy(), orc.get_action_history(0)
        if counting:
            w = cnt.work_counters()
            qc, qdc = (x.cpu().numpy() for x in cnt.get_state())
            cnt.count_work(False)
    finally:
        sim.close(); orc.close()
        if cnt is not None:
            cnt.close()
    err = np.maximum(_err(q, oq), _err(qd, oqd))
    on_ground = touching(oracle, cfg_orc, model, oq, oqd) if can_touch else 0
    print(f"[chain interleave] {mode}{' (run-time model)' if runtime else ''} dr={dr} n={n} {'f64' if dtype == abi.F64 else 'f32'}: "
          f"rel err median {np.median(err):.2e} p95 {np.quantile(err, 0.95):.2e} max {err.max():.2e}; {on_ground} of {n} on the ground"
          + (f"; scanned bodies {w['scanned_bodies']}, bodies with rows {w['row_bodies']} in {w['wave_iterations']} wave-iterations" if counting else ""))
    assert np.isfinite(q).all() and np.isfinite(qd).all() and np.isfinite(oq).all() and np.isfinite(oqd).all()
    assert np.abs(oqd).max() > 0                          # the robots moved
    if can_touch:
        assert on_ground > 0                              # ... on the ground
    if counting:
        assert w["wave_iterations"] == ((n + 63) // 64) * 10 * STEPS
        assert w["scanned_bodies"] > 0 and w["row_bodies"] > 0        # the scan and the row set-up ran in this window
        if dtype == abi.F64:
            assert np.array_equal(q, qc) and np.array_equal(qd, qdc)  # the counting twin computes the same bits
    if dtype == abi.F64:
        assert np.array_equal(a_gpu, a_orc)               # identical action streams
        assert err.max() < F64_TOL, err.max()
    else:
        assert np.median(err) < F32_MEDIAN and np.quantile(err, 0.95) < F32_P95, (np.median(err), np.quantile(err, 0.95))


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_rollout_of_three_equals_three_steps_on_the_ground(HipSim, torch_mod, dtype):
    """os2r_rollout with K = 3 (the fused kernel: the step loop around the same `substep`) against three os2r_step calls on fallen
    monopods with per-env parameters, bit for bit: outputs of every step, the state and the solver state afterwards."""
    n, K = 65, 3
    cfg, _, _, model = configs("free_hip", False, True, n, dtype)
    q0, qd0, params = start(model, True, n, dtype)
    a, b = HipSim(cfg), HipSim(cfg)
    try:
        for h in (a, b):
            for f, v in params.items():
                h.set_params(f, v)
            h.set_state(q0, qd0)
        for _ in range(2):
            per = [a.step(None) for _ in range(K)]
            O, R, Dn, Tm, _ = b.rollout(K, None, want_terminal=True)
            for k in range(K):
                for x, y in zip(per[k], (O[k], R[k], Dn[k], Tm[k])):
                    assert torch_mod.equal(x, y), k
            for x, y in zip(a.get_state() + a.get_solver_state(), b.get_state() + b.get_solver_state()):
                assert torch_mod.equal(x, y)
        assert bool((a.get_state()[1] != 0).any())    # (that these robots are on the ground is asserted by the test above, same start)
    finally:
        a.close(); b.close()
