"""The step kernels off their default settings against the CPU oracle, through the C-ABI (needs an MI355X).

Every other GPU-vs-oracle test with physics on runs substeps = 10, dt = 1e-4, erp = 0.01, max_erv = 1e-3, contact_margin =
1e-3 and per-env parameters from the reference's nominal ranges.  All of these are run-time values of the kernels; here they
take other values:

  1. the five settings of Os2rConfig, one at a time and combined, on the compiled-in free_hip kernels (uniform and per-env
     parameters) and on a run-time chain; in fp32 for the substep count and the time step;
  2. the edges of the five os2r_set_params arrays (zero friction boxes, no gravity, mass scales of 0.1 and 10), one per batch
     and all of them next to each other in every wave;
  3. the non-default solver kernels (sweeps only, exact finish under odd caps, coupled pyramid) on every robot, with uniform
     and per-env parameters, and their independence of a lane's company in the wave;
  4. the fused rollout kernels at substeps != 10;
  5. every refusal of os2r_create's validation.

Common shape of the oracle cases: n = 130 (two waves and a two-lane tail), fallen robots (helpers.lying_states), 4 env-steps,
actions U(-1, 1), auto_reset off, fp64.

Tolerances.  fp64 state: rel(q) < 1e-8, rel(qd) < 1e-6 after the 4 env-steps, test_odd_batch_sizes_and_sweep_counts_match_oracle's
bound for these initial states (1e-6 / 1e-4 on the coupled pyramid, pgs_normal_iters = 0).  It carries over on the oracle's
own evidence: its response to a one-ulp change of (q, qd), worst environment, is 8e-13 / 1.4e-10 at the defaults and at most
3.9e-12 (dt = 1e-3) / 1.9e-9 (mu = 5) over every setting and edge below -- 500 times under the bound.  Observations: rtol =
atol = 1e-8; done: at most 1 of 130 flags may differ (a threshold straddled at the 1e-16 level).  fp32: PHYS_BOUNDS_1 /
PHYS_BOUNDS_3 of test_gpu_fp32.py, scaled by the oracle's own amplification at the setting (_f32_amplification).  Permutation
and fused-rollout checks are bit for bit.
"""
import numpy as np
import pytest

from helpers import lying_states, make_config, perturbed_model
from test_gpu_fp32 import PHYS_BOUNDS_1, PHYS_BOUNDS_3, _f32, _params, _physics_case, _solver_cfg64
from test_gpu_fp32 import _random_states as _random_states_f32

from gym_os2r_amd import abi

pytestmark = pytest.mark.gpu

N, STEPS = 130, 4
# fp64 state bound (module docstring): taken from test_odd_batch_sizes_and_sweep_counts_match_oracle and the oracle's own
# one-ulp response, not from what the kernels give.  Every case prints its measured error (pytest -s).
# Measured on the MI355X, the worst of the 59 cases under this bound: q 7.7e-12, qd 1.0e-8 (both at mu = 5, the case of the
# oracle's own largest one-ulp response); observations 5.2e-10; no done flag apart in any case.
TOL_Q, TOL_QD = 1e-8, 1e-6
# (measured, the worst of the 7 coupled-pyramid cases: q 7.5e-16, qd 2.9e-13)
TOL_Q_PYRAMID, TOL_QD_PYRAMID = 1e-6, 1e-4


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def HipSim(torch_mod):
    from gym_os2r_amd.sim import HipSim
    return HipSim


def _rel(a, b, floor=1.0):
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), floor))


def _rel_per_env(a, b):
    """Worst relative difference of (q, qd) per environment: a, b are (q, qd) pairs of [nq, n] arrays."""
    return np.maximum(*(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1.0), axis=0) for x, y in zip(a, b)))


def _random_states(model, n, rng, vel=8.0):
    """test_gpu_parity.py's random states (for `simple`, which cannot reach the ground)."""
    nq = model["nq"]
    q = rng.uniform(-1.2, 1.2, (nq, n))
    return q, rng.uniform(-vel, vel, (nq, n))


def _inputs(model, n, seed, lying=True, steps=STEPS):
    rng = np.random.default_rng(seed)
    q, qd = lying_states(model, n, rng) if lying else _random_states(model, n, rng)
    return q, qd, [rng.uniform(-1, 1, (n, 2)) for _ in range(steps)]


def _run_oracle(oracle, cfg, q, qd, acts, params=None):
    """-> (q, qd, obs, reward, done) of the oracle after the env-steps, as numpy arrays."""
    orc = oracle.OracleSim(cfg, threads=4)
    for f, v in (params or {}).items():
        orc.set_params(f, v)
    orc.set_state(q, qd)
    for a in acts:
        obs, rew, done, _ = orc.step(a)
    out = tuple(orc.get_state()) + (obs, rew, done)
    orc.close()
    return out


def _run_hip(HipSim, torch, cfg, q, qd, acts, params=None):
    """-> (q, qd, obs, reward, done) of a fresh handle after the env-steps, as device tensors."""
    sim = HipSim(cfg)
    for f, v in (params or {}).items():
        sim.set_params(f, v)
    sim.set_state(q, qd)
    for a in acts:
        obs, rew, done, _ = sim.step(torch.as_tensor(np.ascontiguousarray(a)))
    out = tuple(t.clone() for t in sim.get_state()) + (obs.clone(), rew.clone(), done.clone())
    sim.close()
    return out


def _compare(tag, hip, orc, pyramid=False):
    """State within the fp64 bound, observations within 1e-8, at most one done flag of the batch apart."""
    q2, qd2, obs, rew, done = (t.cpu().numpy() for t in hip)
    oq, oqd, o_obs, o_rew, o_done = orc
    eq, ev = _rel(q2, oq), _rel(qd2, oqd)
    eo = float(np.max(np.abs(obs - o_obs)))
    ndiff = int((done != o_done).sum())
    print(f"[{tag}] rel err q {eq:.2e} qd {ev:.2e}; max obs err {eo:.2e}; done flags apart {ndiff}")
    assert np.isfinite(oq).all() and np.isfinite(oqd).all(), tag
    tq, tv = (TOL_Q_PYRAMID, TOL_QD_PYRAMID) if pyramid else (TOL_Q, TOL_QD)
    assert eq < tq and ev < tv, (tag, eq, ev)
    np.testing.assert_allclose(obs, o_obs, rtol=1e-8, atol=1e-8, err_msg=tag)
    assert ndiff <= 1, (tag, ndiff)
    return eq, ev


def _touching(oracle, cfg, oq, oqd, every=1):
    """The fraction of the sampled environments with an active contact point in the oracle's state."""
    ms, nq = cfg.model, cfg.model.nq
    envs = range(0, oq.shape[1], every)
    hit = 0
    for e in envs:
        _, _, rw, ow = oracle.dynamics(ms, oq[:, e], oqd[:, e], np.zeros(nq))
        hit += int(oracle.contact_points(ms, rw, ow, cfg.contact_margin)[0].any())
    return hit / len(envs)


def _permutation_check(HipSim, torch, cfg, q, qd, acts, params, rng, base=None):
    """The same environments in another order: every result, un-permuted, equals the first run's bit for bit."""
    n = q.shape[1]
    base = base or _run_hip(HipSim, torch, cfg, q, qd, acts, params)
    perm = rng.permutation(n)
    shuf = _run_hip(HipSim, torch, cfg, q[:, perm], qd[:, perm], [a[perm] for a in acts],
                    {f: np.ascontiguousarray(v[:, perm]) for f, v in (params or {}).items()})
    pt = torch.as_tensor(perm, device=base[0].device)
    assert torch.equal(base[0][:, pt], shuf[0]) and torch.equal(base[1][:, pt], shuf[1])          # q, qd
    assert torch.equal(base[2][pt], shuf[2]) and torch.equal(base[3][pt], shuf[3]) and torch.equal(base[4][pt], shuf[4])
    assert int((perm != np.arange(n)).sum()) > n // 2
    return base


# ---------------------------------------------------------------------------------------
# 1. the settings of Os2rConfig
# ---------------------------------------------------------------------------------------
SETTINGS = {
    "substeps=1": dict(substeps=1), "substeps=3": dict(substeps=3), "substeps=25": dict(substeps=25),
    "dt=2.5e-5": dict(dt=2.5e-5), "dt=1e-3": dict(dt=1e-3),
    "margin=0": dict(contact_margin=0.0), "margin=0.01": dict(contact_margin=0.01),
    # at the default max_erv the cap is hit on every penetrating contact and erp alone changes nothing: this pair takes the
    # uncapped branch of the error-reduction velocity
    "erp=0.2,max_erv=10": dict(erp=0.2, max_erv=10.0),
    "max_erv=0": dict(max_erv=0.0),
    "combined": dict(substeps=3, dt=2e-4, erp=0.2, max_erv=10.0, contact_margin=0.005),
}
FORMS = ["static", "static_dr", "runtime"]      # compiled-in free_hip; the same with per-env parameters; a run-time chain


def _form(form, **settings):
    """-> (config, model dict, q, qd, actions, per-env parameters or None): the inputs depend on the form alone."""
    seed = 400 + FORMS.index(form)
    overrides = perturbed_model("free_hip", np.random.default_rng(23)) if form == "runtime" else None
    cfg, _, model = make_config("free_hip", "BalancingV2", True, num_envs=N, contact=True, auto_reset=False, dtype=abi.F64,
                                model_overrides=overrides, **settings)
    q, qd, acts = _inputs(model, N, seed)
    params = _params(np.random.default_rng(seed + 50), model, N) if form == "static_dr" else None
    return cfg, model, q, qd, acts, params


_default_results = {}


def _oracle_at_defaults(oracle, form):
    """The oracle's result on the form's inputs under the default settings: computed once, shared, never modified."""
    if form not in _default_results:
        cfg, _, q, qd, acts, params = _form(form)
        _default_results[form] = _run_oracle(oracle, cfg, q, qd, acts, params)
    return _default_results[form]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_settings_match_oracle(HipSim, torch_mod, oracle, setting, form):
    """One setting away from the defaults (and one case with four of them away): state, observations and done flags against
    the oracle.  The setting must bite: the oracle's own result under it differs from its result under the defaults by more
    than 1e-6 relative in at least a tenth of the environments (on the oracle: 52 % at the least, the contact margin; all of
    them for substeps and dt)."""
    cfg, model, q, qd, acts, params = _form(form, **SETTINGS[setting])
    orc = _run_oracle(oracle, cfg, q, qd, acts, params)
    dflt = _oracle_at_defaults(oracle, form)
    moved = float((_rel_per_env(orc[:2], dflt[:2]) > 1e-6).mean())
    touch = _touching(oracle, cfg, orc[0], orc[1])
    print(f"[{setting} {form}] the setting moves {100 * moved:.0f} % of the environments; {100 * touch:.0f} % touch the ground")
    assert moved >= 0.1, (setting, form, moved)
    assert touch >= 0.5, (setting, form, touch)           # the contact rows are what these settings enter
    hip = _run_hip(HipSim, torch_mod, cfg, q, qd, acts, params)
    _compare(f"{setting} {form}", hip, orc)


def _f32_amplification(oracle, cfg_case, cfg_default, model, n, steps, seed):
    """How much more than at the default settings the oracle itself amplifies one float32 ulp on the inputs of
    _physics_case(n=n, steps=steps, seed=seed): the oracle, on the fp32 solver settings, on the float32-rounded inputs and
    on the states moved by one float32 ulp either way; the p99 of the relative response of q and of qd after the first and
    after the last env-step; the ratio case / default of each quantity on its own, floored at 1.
    -> ((ratio of q, of qd) after 1 step, (ratio of q, of qd) after all, the fraction of the case's environments that touch
    the ground in the oracle's final state)"""
    def response(cfg):
        rng = np.random.default_rng(seed)
        q, qd = _random_states_f32(model, n, rng)
        acts = [_f32(rng.uniform(-1, 1, (n, 2))) for _ in range(steps)]
        prng = np.random.default_rng(seed + 1)

        def one_ulp(x):
            to = np.where(prng.random(x.shape) < 0.5, -np.inf, np.inf).astype(np.float32)
            return np.nextafter(x.astype(np.float32), to).astype(np.float64)
        a, b = oracle.OracleSim(cfg, threads=8), oracle.OracleSim(cfg, threads=8)
        a.set_state(q, qd); b.set_state(one_ulp(q), one_ulp(qd))
        out = []
        for k, act in enumerate(acts):
            a.step(act); b.step(act)
            if k in (0, steps - 1):
                (aq, aqd), (bq, bqd) = a.get_state(), b.get_state()
                out.append((np.quantile(np.abs(bq - aq) / np.maximum(np.abs(aq), 1.0), 0.99),
                            np.quantile(np.abs(bqd - aqd) / np.maximum(np.abs(aqd), 1.0), 0.99)))
        touch = _touching(oracle, cfg, aq, aqd, every=4)
        a.close(); b.close()
        return out, touch
    (case, touch), (dflt, _) = response(cfg_case), response(cfg_default)
    return [(max(1.0, c[0] / d[0]), max(1.0, c[1] / d[1])) for c, d in zip(case, dflt)] + [touch]


@pytest.mark.parametrize("setting", ["substeps=1", "substeps=25", "dt=2.5e-5", "dt=1e-3"])
def test_settings_f32(HipSim, torch_mod, oracle, setting):
    """The substep count and the time step on the compiled-in fp32 free_hip kernels: test_physics_f32_all_modes' case and
    checks (state after 1 and 3 env-steps against the oracle on the fp32 solver settings, the epilogue of every step exactly),
    median and p99 bounded by PHYS_BOUNDS_1 / PHYS_BOUNDS_3, each times the oracle's own amplification of that quantity at the
    setting (q's for the p99 of q, qd's for the median and the p99 of qd).  Those bounds were measured at the default settings;
    what a setting may add is what it adds to the reference's response to the same rounding, one float32 ulp on the inputs.  No
    bound on the maximum: a foot that slips at another instant (1e-3 at dt = 2.5e-5 in the oracle's own one-ulp response).
    Contact is exercised: every joint of that case's states is uniform in +-1.2 rad, which leaves about a fifth of the robots
    on the ground in the oracle's final state (20 - 21 % at the four settings).  The bounded p99 leaves 1 % of the environments
    out; at least 10 % must touch the ground, ten times that share, so that an error in the contact rows cannot stay in the
    part of the batch that the p99 does not see."""
    n, steps, seed = 512, 3, 11
    kw = dict(num_envs=n, contact=True, auto_reset=False)
    cfg32, _, model = make_config("free_hip", "BalancingV2", True, dtype=abi.F32, **kw, **SETTINGS[setting])
    cfg64 = _solver_cfg64("free_hip", cfg32, reward_name="BalancingV2", **kw, **SETTINGS[setting])
    cfg32_d, _, _ = make_config("free_hip", "BalancingV2", True, dtype=abi.F32, **kw)
    cfg64_d = _solver_cfg64("free_hip", cfg32_d, reward_name="BalancingV2", **kw)
    (aq1, av1), (aq3, av3), touch = _f32_amplification(oracle, cfg64, cfg64_d, model, n, steps, seed)
    print(f"[f32 {setting}] amplification of q {aq1:.2f} / {aq3:.2f}, of qd {av1:.2f} / {av3:.2f}; "
          f"{100 * touch:.0f} % touch the ground")
    assert touch >= 0.1, (setting, touch)
    one, three = _physics_case(HipSim, torch_mod, oracle, "free_hip", True, dr=False, n=n, steps=steps, seed=seed,
                               cfg_pair=(cfg32, cfg64, model))
    print(f"[f32 {setting}] 1 step: median qd {one[0]:.2e}, p99 q {one[1]:.2e} qd {one[2]:.2e}; "
          f"3 steps: median qd {three[0]:.2e}, p99 q {three[1]:.2e} qd {three[2]:.2e}")
    assert all(a <= amp * b for a, amp, b in zip(one, (av1, aq1, av1), PHYS_BOUNDS_1)), (one, aq1, av1)
    assert all(a <= amp * b for a, amp, b in zip(three, (av3, aq3, av3), PHYS_BOUNDS_3)), (three, aq3, av3)


# ---------------------------------------------------------------------------------------
# 2. the edges of the per-env parameters
# ---------------------------------------------------------------------------------------
EDGES = [
    ("mu=0", {abi.PARAM_MU: 0.0}), ("mu=5", {abi.PARAM_MU: 5.0}),
    ("friction=0", {abi.PARAM_FRICTION: 0.0}), ("friction=1", {abi.PARAM_FRICTION: 1.0}),
    ("damping=0", {abi.PARAM_DAMPING: 0.0}),
    ("gravity=0", {abi.PARAM_GRAVITY: 0.0}), ("gravity=+9.8", {abi.PARAM_GRAVITY: 9.8}),
    ("mass_scale=0.1", {abi.PARAM_MASS_SCALE: 0.1}), ("mass_scale=10", {abi.PARAM_MASS_SCALE: 10.0}),
    ("mu=friction=damping=0", {abi.PARAM_MU: 0.0, abi.PARAM_FRICTION: 0.0, abi.PARAM_DAMPING: 0.0}),
]


def _edge_case(edge_of_env):
    """free_hip, default solver; environment e carries EDGES[edge_of_env[e]] on all its bodies / joints (len(EDGES): none,
    the nominal draws) on top of nominal draws of the other parameters."""
    cfg, _, model = make_config("free_hip", "BalancingV2", True, num_envs=N, contact=True, auto_reset=False, dtype=abi.F64)
    q, qd, acts = _inputs(model, N, 500)
    params = _params(np.random.default_rng(550), model, N)
    for k, (_, values) in enumerate(EDGES):
        for f, v in values.items():
            params[f][:, edge_of_env == k] = v
    return cfg, q, qd, acts, params


@pytest.mark.parametrize("edge", range(len(EDGES)), ids=[name for name, _ in EDGES])
def test_parameter_edges_match_oracle(HipSim, torch_mod, oracle, edge):
    """One edge value in all 130 environments: the [0, 0] friction boxes of mu = 0 and friction = 0, a stiff box, no damping,
    no gravity and gravity upwards, the row weights under a mass scale of 0.1 and of 10.  The oracle stays finite and in
    contact at every one of them (96 % touch the ground, |qd| below 40)."""
    cfg, q, qd, acts, params = _edge_case(np.full(N, edge))
    orc = _run_oracle(oracle, cfg, q, qd, acts, params)
    touch = _touching(oracle, cfg, orc[0], orc[1])
    print(f"[{EDGES[edge][0]}] {100 * touch:.0f} % touch the ground, max |qd| {np.abs(orc[1]).max():.1f}")
    assert touch >= 0.5, (EDGES[edge][0], touch)
    hip = _run_hip(HipSim, torch_mod, cfg, q, qd, acts, params)
    _compare(EDGES[edge][0], hip, orc)


def test_parameter_edges_mixed_in_every_wave(HipSim, torch_mod, oracle):
    """Lane e carries edge e mod 11 (the eleventh: nominal parameters), so every wave holds every kind of friction box and row
    weight next to every other: against the oracle, and -- the same 130 environments in a permuted order -- bit for bit against
    itself (a lane's result does not depend on its company in the wave)."""
    cfg, q, qd, acts, params = _edge_case(np.arange(N) % (len(EDGES) + 1))
    orc = _run_oracle(oracle, cfg, q, qd, acts, params)
    touch = _touching(oracle, cfg, orc[0], orc[1])
    assert touch >= 0.5, touch
    hip = _run_hip(HipSim, torch_mod, cfg, q, qd, acts, params)
    _compare("edges mixed", hip, orc)
    _permutation_check(HipSim, torch_mod, cfg, q, qd, acts, params, np.random.default_rng(7), base=hip)


# ---------------------------------------------------------------------------------------
# 3. solver settings x robot x parameters
# ---------------------------------------------------------------------------------------
SOLVERS = [(7, 3, 0), (9, 3, 3), (5, 0, 12)]      # sweeps only; exact finish under odd caps; coupled pyramid (sweeps only)
# (robot, run-time chain?, solver): the compiled-in robots on the three settings, free_hip with per-env parameters only (its
# uniform form is test_odd_batch_sizes_and_sweep_counts_match_oracle's), two run-time chains on the sweeps-only fp64 solver
SOLVER_CASES = ([(mode, False, s, dr) for mode in ("fixed_hip", "fixed", "simple") for s in SOLVERS for dr in (False, True)]
                + [("free_hip", False, s, True) for s in SOLVERS]
                + [(mode, True, (20, 2, 0), dr) for mode in ("free_hip", "fixed") for dr in (False, True)])


def _solver_case(mode, runtime, solver, dr, n=N, seed=600):
    reward = "StraightV1" if mode == "simple" else "BalancingV2"
    overrides = perturbed_model(mode, np.random.default_rng(23)) if runtime else None
    kw = {} if solver is None else dict(pgs_iters=solver[0], pgs_normal_iters=solver[1], pgs_exact=solver[2])
    cfg, _, model = make_config(mode, reward, True, num_envs=n, contact=True, auto_reset=False, dtype=abi.F64,
                                model_overrides=overrides, **kw)
    q, qd, acts = _inputs(model, n, seed, lying=mode != "simple")
    params = _params(np.random.default_rng(seed + 50), model, n) if dr else None
    return cfg, q, qd, acts, params


@pytest.mark.parametrize("mode,runtime,solver,dr", SOLVER_CASES,
                         ids=[f"{m}{'-rt' if r else ''}-{s[0]}.{s[1]}.{s[2]}-{'dr' if d else 'uni'}" for m, r, s, d in SOLVER_CASES])
def test_solver_settings_match_oracle(HipSim, torch_mod, oracle, mode, runtime, solver, dr):
    """The kernels for non-default solver settings (kSolverSweeps / kSolverExact with the run-time observation layout) on the
    robots and parameter forms that had never run them, against the oracle on the same settings; the robots that can reach the
    ground do: at least half of them touch it in the oracle's final state (96 - 97 % on the oracle)."""
    cfg, q, qd, acts, params = _solver_case(mode, runtime, solver, dr)
    orc = _run_oracle(oracle, cfg, q, qd, acts, params)
    tag = f"{mode}{' run-time' if runtime else ''} {solver} dr={dr}"
    if mode != "simple":                                  # (`simple` has no contact candidates)
        touch = _touching(oracle, cfg, orc[0], orc[1])
        print(f"[{tag}] {100 * touch:.0f} % touch the ground")
        assert touch >= 0.5, (tag, touch)
    hip = _run_hip(HipSim, torch_mod, cfg, q, qd, acts, params)
    _compare(tag, hip, orc, pyramid=solver[1] == 0)


@pytest.mark.parametrize("runtime,solver,dr", [(False, (9, 3, 3), True), (True, None, False), (True, None, True)],
                         ids=["free_hip-9.3.3-dr", "run-time-default-uni", "run-time-default-dr"])
def test_solver_kernels_do_not_depend_on_company(HipSim, torch_mod, oracle, runtime, solver, dr):
    """The wave-level decisions of the solver (row masks by ballot, rows void for every lane) on the kernels that keep the exact
    finish's multipliers in LDS: 1000 fallen free_hip robots and the same robots in a permuted order give the same results,
    bit for bit -- the compiled-in robot on (9, 3, 3) with per-env parameters, and a run-time chain on its default solver."""
    n = 1000
    cfg, q, qd, acts, params = _solver_case("free_hip", runtime, solver, dr, n=n, seed=700)
    base = _permutation_check(HipSim, torch_mod, cfg, q, qd, acts, params, np.random.default_rng(8))
    oq, oqd = (t.cpu().numpy() for t in base[:2])
    touch = _touching(oracle, cfg, oq, oqd, every=8)
    assert np.isfinite(oq).all() and np.isfinite(oqd).all() and touch >= 0.5, touch


# ---------------------------------------------------------------------------------------
# 4. fused rollouts off the default substep count
# ---------------------------------------------------------------------------------------
def _everything(sim):
    return (sim.get_state() + sim.get_solver_state() + sim.episode_info() + (sim.get_action_history(0), sim.get_action_history(1)))


def _assert_same_handle(torch, a, b, what):
    for x, y in zip(_everything(a), _everything(b)):
        assert torch.equal(x, y), what
    assert a.step_count == b.step_count, what


@pytest.mark.parametrize("mode", ["free_hip", "fixed_hip_simple"])
def test_fused_rollouts_off_the_default_substeps(HipSim, torch_mod, oracle, mode):
    """os2r_rollout and os2r_rollout_policy take their fused kernels whenever the solver counts are the defaults, at any
    substep count: at substeps = 3, dt = 2e-4, K env-steps in one launch are K launches -- per-step outputs, state, solver
    state, episode counters and action history, bit for bit, through randomised resets and TimeLimit truncations.

    An env-step is 0.6 ms here and an episode at most 7 of them: a robot reset to `stand` never falls as far as the ground (on
    the oracle, none of the 200 touches it at any step of the window).  So that the contact rows are part of what is compared,
    both handles get the same fallen robots (helpers.lying_states) as the state each window starts from: at least half of them
    must touch the ground in that state, and they stay there until their episodes are truncated inside the window (on the
    oracle: 96 % touch for the first four env-steps, then all 200 are reset)."""
    torch = torch_mod
    n, K = 200, 12

    def make():
        cfg, _, model = make_config(mode, "BalancingV2", True, reset_mode=abi.RESET_RANDOM, randomize_params=True, num_envs=n,
                                    contact=True, seed=5, max_episode_steps=7, dtype=abi.F64, substeps=3, dt=2e-4)
        sim = HipSim(cfg)
        for _ in range(30):
            sim.step(None)
        return sim, cfg, model

    def lay_down(seed):
        q, qd = lying_states(model, n, np.random.default_rng(seed))
        touch = _touching(oracle, cfg, q, qd)
        print(f"[fused {mode}] {100 * touch:.0f} % of the robots touch the ground at the start of the window")
        assert touch >= 0.5, (mode, touch)
        a.set_state(q, qd); b.set_state(q, qd)
    (a, cfg, model), (b, _, _) = make(), make()
    rng = np.random.default_rng(3)
    lay_down(41)
    actions = torch.as_tensor(rng.uniform(-1, 1, (K, n, 2)), device=a.device).to(a.dtype)
    a.done_reasons(True)
    per = []
    for k in range(K):
        o, r, d, t = a.step(actions[k])
        per.append((o, r, d, t, a.reasons.clone()))
    a.done_reasons(False)
    O, R, Dn, Tm, Wy = b.rollout(K, actions, want_terminal=True, want_reasons=True)
    for k in range(K):
        for x, y in zip(per[k], (O[k], R[k], Dn[k], Tm[k], Wy[k])):
            assert torch.equal(x, y), (mode, "rollout", k)
    assert int((Dn != 0).sum()) > 0                       # episodes ended (and were reset) inside the window
    _assert_same_handle(torch, a, b, (mode, "rollout"))
    # the policy in the loop: the fused kernel on b, the library's launch loop on a (work counters on: no fused variant counts)
    lay_down(42)
    g = torch.Generator().manual_seed(0)
    W = (0.6 * torch.randn((n, 2, a.D + 1), generator=g, dtype=torch.float64)).to(a.device, a.dtype)
    a.count_work(True)
    ra, la, oa = a.rollout_policy(K, W, want_outputs=True, want_terminal=True, want_reasons=True)
    rb, lb, ob = b.rollout_policy(K, W, want_outputs=True, want_terminal=True, want_reasons=True)
    assert torch.equal(ra, rb) and torch.equal(la, lb)
    for x, y in zip(oa, ob):
        assert torch.equal(x, y), (mode, "rollout_policy")
    assert int((ob[2] != 0).sum()) > 0
    _assert_same_handle(torch, a, b, (mode, "rollout_policy"))
    assert a.work_counters()["wave_iterations"] > 0       # the counting step kernel ran: the launch loop
    a.count_work(False)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------
# 5. what os2r_create refuses (no launch)
# ---------------------------------------------------------------------------------------
def _set(path, value):
    def apply(cfg):
        obj, names = cfg, path.split(".")
        for name in names[:-1]:
            obj = getattr(obj, name)
        if "[" in names[-1]:
            name, idx = names[-1][:-1].split("[")
            getattr(obj, name)[int(idx)] = value
        else:
            setattr(obj, names[-1], value)
    return apply


def _both(*fs):
    def apply(cfg):
        for f in fs:
            f(cfg)
    return apply


NQ = 4      # fixed_hip: yaw, pitch, hip, knee
# (what trips exactly one condition of os2r_capi.hip: validate on a valid fixed_hip config, the message it must give);
# abi_version, nq and HoppingV1 are test_capi_rejects_bad_config's
REFUSALS = [
    (_set("dtype", 7), "dtype must be"),
    (_set("num_envs", 0), "num_envs must be positive"),
    (_set("num_envs", -3), "num_envs must be positive"),
    (_set("model.ncand", abi.MAX_CAND + 1), "ncand out of range"),
    (_set("model.ncand", -1), "ncand out of range"),
    (_set("model.cand_body[0]", NQ), "cand_body must be non-decreasing"),
    (_both(_set("model.cand_body[0]", NQ - 1), _set("model.cand_body[1]", 0)), "cand_body must be non-decreasing"),
    (_set("model.axis[1]", 3), "joint axis"),
    (_set("model.axis[0]", -1), "joint axis"),
    (_set("model.mass[2]", 0.0), "mass must be positive"),
    (_set("model.mass[0]", float("nan")), "mass must be positive"),
    (_set("model.act_dof[1]", NQ), "act_dof out of range"),
    (_set("model.act_dof[0]", -1), "act_dof out of range"),
    (_set("task.obs_dim", 0), "obs_dim out of range"),
    (_set("task.obs_dim", abi.MAX_OBS + 1), "obs_dim out of range"),
    (_set("task.obs_kind[3]", abi.OBS_TORQUE_RAW + 1), "unknown obs kind"),
    (_set("task.obs_kind[0]", -1), "unknown obs kind"),
    (_set("task.obs_src[0]", NQ), "obs_src out of range"),
    (_set("task.obs_src[1]", -1), "obs_src out of range"),
    (_set("task.reward_id", abi.REWARD_STRAIGHT_V1 + 1), "unknown reward id"),
    (_set("task.reward_id", -1), "unknown reward id"),
    (_set("task.idx_pitch_pos", -1), "pitch position"),
    (_both(_set("task.reward_id", abi.REWARD_STRAIGHT_V1), _set("task.idx_knee_pos", -1)), "StraightV1 needs"),
    (_both(_set("task.reward_id", abi.REWARD_STRAIGHT_V1), _set("task.idx_hip_pos", -1)), "StraightV1 needs"),
    (_set("task.n_reset_poses", 0), "n_reset_poses out of range"),
    (_set("task.n_reset_poses", abi.MAX_RESET_POSES + 1), "n_reset_poses out of range"),
    (_set("substeps", 0), "substeps out of range"),
    (_set("substeps", 1001), "substeps out of range"),
    (_set("dt", 0.0), "dt must be positive"),
    (_set("dt", -1e-4), "dt must be positive"),
    (_set("dt", float("nan")), "dt must be positive"),
    (_set("pgs_iters", -1), "pgs_iters out of range"),
    (_set("pgs_iters", 10001), "pgs_iters out of range"),
    (_set("contact_margin", -1e-3), "contact_margin must be"),
    (_set("contact_margin", float("nan")), "contact_margin must be"),
    (_set("task.gravity_rollouts", -1), "gravity_rollouts must be"),
    (_set("pgs_normal_iters", -1), "pgs_normal_iters out of range"),
    (_set("pgs_normal_iters", 10001), "pgs_normal_iters out of range"),
    (_set("pgs_tol", -1e-12), "pgs_tol must be"),
    (_set("pgs_tol", float("nan")), "pgs_tol must be"),
    (_set("pgs_exact", -1), "pgs_exact out of range"),
    (_set("pgs_exact", 10001), "pgs_exact out of range"),
    (_both(_set("dtype", abi.F32), _set("pgs_exact", 12)), "needs dtype f64"),
    # a non-finite erp or max_erv would go into every contact row of every environment, silently
    (_set("erp", float("nan")), "erp must be finite"),
    (_set("erp", float("inf")), "erp must be finite"),
    (_set("max_erv", float("nan")), "max_erv must be finite"),
    (_set("max_erv", float("-inf")), "max_erv must be finite"),
    (_set("max_erv", -1e-3), "max_erv must be >= 0"),
]


def _valid_config():
    return make_config("fixed_hip", "BalancingV1", True, num_envs=8, dtype=abi.F64)[0]


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=[f"{k}-{m.split()[0]}" for k, (_, m) in enumerate(REFUSALS)])
def test_create_refuses(HipSim, k):
    """Every condition of the config validation, tripped alone on an otherwise valid config, is refused with its own message
    before anything is allocated or launched."""
    from gym_os2r_amd.sim import Os2rError
    change, message = REFUSALS[k]
    cfg = _valid_config()
    assert cfg.model.nq == NQ and cfg.model.ncand >= 2
    change(cfg)
    with pytest.raises(Os2rError, match=message):
        HipSim(cfg)


def test_create_accepts_zero_erp_and_max_erv(HipSim):
    """erp = 0 and max_erv = 0 (no error reduction) are legal, like every valid config the refusals start from."""
    HipSim(_valid_config()).close()
    cfg = _valid_config()
    cfg.erp = 0.0
    cfg.max_erv = 0.0
    HipSim(cfg).close()
