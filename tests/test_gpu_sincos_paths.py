"""The three-way choice of `substep` step 1 -- series turn, sincos_fast, sincos_lib -- inside the fp64 step kernel (needs an MI355X).

The primitives themselves are held against high-precision references in tests/test_gpu_math_probe.py; here the kernel's choice
between them is: the work counter `full_sincos` counts what it says, far angles (below, at and beyond the guard of sincos_fast)
and fast joints (|dt qd| on both sides of 0.06) match the oracle, and a lane's result does not depend on its wave-mates.

Shape: compiled-in free_hip, contact on, auto_reset off, 128 environments (two waves), one env-step unless stated, fp64.  Bounds:
TOL_Q / TOL_QD of test_gpu_settings.py (the project's, from the oracle's own one-ulp response).  Every input is generated below
from SEED and checked on the oracle alone before anything runs on the device: the oracle's state stays finite, and a speed that
is meant to stay above 0.06 / dt does so in the oracle at substeps = 1.  The speed sits on the knee, the lightest link: 900 rad/s
there stay above 0.067 / dt for the ten iterations in every lane and leave the other joints below 240 rad/s; on the hip such a
speed decays below the limit within the env-step, on the yaw it drives the knee past 1200 rad/s.
"""
import numpy as np
import pytest

from helpers import lying_states, make_config
from test_gpu_settings import TOL_Q, TOL_QD, HipSim, _compare, _permutation_check, _rel, _run_hip, _run_oracle, torch_mod  # noqa: F401

from gym_os2r_amd import abi

pytestmark = pytest.mark.gpu

N, SEED = 128, 20261021
LIMIT = 0.06                                       # substep step 1: the series turn serves |dt * qd| < 0.06
FAR = (1e3, 1e5, 8.19e5, 8.2e5, 1e7)               # below, at and beyond sincos_in_range's 8.2e5
FAST, JUST_BELOW, JUST_ABOVE = 900.0, 599.0, 601.0  # rad/s at dt = 1e-4: 0.09, 0.0599, 0.0601


def _cfg(**kw):
    return make_config("free_hip", "BalancingV2", True, num_envs=N, contact=True, auto_reset=False, dtype=abi.F64, **kw)


def _base(seed):
    """Ordinary states: test_gpu_settings' fallen robots, the boom raised so that the leg swings free at any knee angle."""
    cfg, _, model = _cfg()
    rng = np.random.default_rng(seed)
    q, qd = lying_states(model, N, rng)
    q[model["dof_names"].index("planarizer_pitch_joint")] = 0.3
    return cfg, model, q, qd, rng


def _knee(model):
    return model["dof_names"].index("knee_joint")


def _periodic(model):
    return [model["dof_names"].index(n) for n in ("planarizer_yaw_joint", "knee_joint")]


def _speed_case(fast_lanes):
    """The knee of `fast_lanes` at FAST rad/s, every other speed small -> (cfg, model, q, qd, actions)."""
    cfg, model, q, qd, rng = _base(SEED)
    qd[_knee(model), fast_lanes] = FAST * rng.choice([-1.0, 1.0], len(fast_lanes))
    return cfg, model, q, qd, [np.zeros((N, 2))]


def _far_case(steps):
    """Environment e: yaw and knee at +-FAR[e mod 5] (the sign changes every five environments), the rest ordinary."""
    cfg, model, q, qd, rng = _base(SEED + 1)
    e = np.arange(N)
    far = np.array(FAR)[e % 5] * np.where((e // 5) % 2 == 0, 1.0, -1.0)
    for j in _periodic(model):
        q[j] = far
    assert set(np.abs(q[_periodic(model)]).ravel()) == set(FAR)
    return cfg, model, q, qd, [rng.uniform(-1, 1, (N, 2)) for _ in range(steps)]


def _threshold_case():
    """Item 1's inputs with the knee at JUST_BELOW (even environments) and JUST_ABOVE (odd ones) of 0.06 / dt, either sign."""
    cfg, model, q, qd, rng = _base(SEED)
    e = np.arange(N)
    qd[_knee(model)] = np.where(e % 2 == 0, JUST_BELOW, JUST_ABOVE) * np.where((e // 2) % 2 == 0, 1.0, -1.0)
    assert (np.abs(cfg.dt * qd[_knee(model), 0::2]) < LIMIT).all() and (np.abs(cfg.dt * qd[_knee(model), 1::2]) > LIMIT).all()
    return cfg, model, q, qd, [rng.uniform(-1, 1, (N, 2))]


def _increments(oracle, q, qd, acts):
    """max_joints |dt * qd| per environment at the start of each of the ten physics iterations of one env-step: the oracle at
    substeps = 1, the action held -> [10, N]; its state must stay finite."""
    cfg1 = _cfg(substeps=1)[0]
    orc = oracle.OracleSim(cfg1, threads=4)
    orc.set_state(q, qd)
    out = [np.abs(cfg1.dt * qd).max(axis=0)]
    for _ in range(9):
        orc.step(acts[0])
        oq, oqd = orc.get_state()
        assert np.isfinite(oq).all() and np.isfinite(oqd).all()
        out.append(np.abs(cfg1.dt * oqd).max(axis=0))
    orc.close()
    return np.array(out)


def _step_counted(HipSim, torch, cfg, q, qd, acts):
    """One handle with the counting kernel variant -> ((q, qd, obs, reward, done), counters)."""
    sim = HipSim(cfg)
    sim.count_work(True)
    sim.set_state(q, qd)
    for a in acts:
        obs, rew, done, _ = sim.step(torch.as_tensor(np.ascontiguousarray(a)))
    out = tuple(t.clone() for t in sim.get_state()) + (obs.clone(), rew.clone(), done.clone())
    counters = sim.work_counters()
    sim.count_work(False)
    sim.close()
    return out, counters


# (fast lanes, full evaluations counted: wave 0 + wave 1)
COUNTER_CASES = {"all-slow": ([], 1 + 1), "wave-1-fast": (list(range(64, 128)), 1 + 10), "one-lane-fast": ([64 + 17], 1 + 10)}


@pytest.mark.parametrize("case", list(COUNTER_CASES))
def test_full_sincos_counter(HipSim, torch_mod, oracle, case):
    """`full_sincos` adds one per wave and physics iteration in which some lane evaluated sin / cos in full: the first
    iteration of an env-step for every wave, and every iteration of a wave that holds a lane with |dt qd| >= 0.06 on a joint --
    one lane is enough.  The counting variant's results are the plain kernel's, bit for bit."""
    fast, want = COUNTER_CASES[case]
    cfg, model, q, qd, acts = _speed_case(fast)
    inc = _increments(oracle, q, qd, acts)
    slow = np.setdiff1d(np.arange(N), fast)
    print(f"[{case}] oracle, ten iterations: slow lanes max |dt qd| {inc[:, slow].max():.4f}"
          + (f", fast lanes min {inc[:, fast].min():.4f}" if fast else ""))
    assert (inc[:, slow] < LIMIT).all() and (not fast or (inc[:, fast] > LIMIT).all())
    assert not fast or min(fast) >= 64                      # wave 0 holds slow lanes only
    plain = _run_hip(HipSim, torch_mod, cfg, q, qd, acts)
    counted, counters = _step_counted(HipSim, torch_mod, cfg, q, qd, acts)
    print(f"[{case}] full_sincos {counters['full_sincos']} of {counters['wave_iterations']} wave iterations")
    assert counters["wave_iterations"] == 2 * cfg.substeps == 20
    assert counters["full_sincos"] == want, counters
    for a, b in zip(plain, counted):
        assert torch_mod.equal(a, b), case


@pytest.mark.parametrize("steps", [1, 4])
def test_far_angles_match_oracle(HipSim, torch_mod, oracle, steps):
    """Yaw and knee at 1e3 ... 1e7 rad: sincos_fast below the guard, sincos_lib from it on, the series turn after the first
    iteration everywhere.  The turn advances (sin, cos) by the unrounded increment while the oracle evaluates at the rounded q:
    after m turns the rotations may stand m ulp(q) / 2 apart -- printed per magnitude next to the state's error."""
    cfg, model, q, qd, acts = _far_case(steps)
    orc = _run_oracle(oracle, cfg, q, qd, acts)
    assert np.isfinite(orc[0]).all() and np.isfinite(orc[1]).all() and np.abs(orc[1]).max() < 100.0, np.abs(orc[1]).max()
    hip = _run_hip(HipSim, torch_mod, cfg, q, qd, acts)
    hq, hqd = hip[0].cpu().numpy(), hip[1].cpu().numpy()
    for k, mag in enumerate(FAR):
        sel = np.arange(N) % 5 == k
        print(f"[far {steps}] |q| = {mag:g}: rel err q {_rel(hq[:, sel], orc[0][:, sel]):.2e} qd {_rel(hqd[:, sel], orc[1][:, sel]):.2e}; "
              f"predicted rotation difference up to {(cfg.substeps - 1) * np.spacing(mag) / 2:.1e} (bounds {TOL_Q:g} / {TOL_QD:g})")
    _compare(f"far angles, {steps} env-steps", hip, orc)


def test_fast_joints_match_oracle(HipSim, torch_mod, oracle):
    """The knee just below and just above 0.06 / dt in alternating lanes (every wave takes both sides of the choice), and at
    900 rad/s in a whole wave and in a single lane (the counter cases): one env-step against the oracle."""
    cases = [("threshold",) + _threshold_case()] + [(name,) + _speed_case(COUNTER_CASES[name][0]) for name in ("wave-1-fast", "one-lane-fast")]
    for name, cfg, model, q, qd, acts in cases:
        orc = _run_oracle(oracle, cfg, q, qd, acts)
        print(f"[{name}] oracle: max |qd| after the env-step {np.abs(orc[1]).max():.1f}")
        _compare(f"fast joints, {name}", _run_hip(HipSim, torch_mod, cfg, q, qd, acts), orc)


def test_paths_do_not_depend_on_company(HipSim, torch_mod, oracle):
    """Far lanes (every magnitude) and fast lanes (below, above and well above 0.06) next to each other in every wave: the
    same 128 environments in a permuted order give the same results, bit for bit; and they match the oracle."""
    cfg, model, q, qd, acts = _far_case(1)
    _, _, q3, qd3, _ = _threshold_case()
    e = np.arange(N)
    fast = e % 3 == 1                                           # a third of the lanes: the threshold case's state
    q[:, fast], qd[:, fast] = q3[:, fast], qd3[:, fast]
    well = e % 12 == 1
    qd[_knee(model), well] = FAST
    for w in (slice(0, 64), slice(64, 128)):
        assert fast[w].any() and well[w].any() and all((np.abs(q[0, w]) == m).any() for m in FAR)
    orc = _run_oracle(oracle, cfg, q, qd, acts)
    hip = _run_hip(HipSim, torch_mod, cfg, q, qd, acts)
    _compare("mixed waves", hip, orc)
    _permutation_check(HipSim, torch_mod, cfg, q, qd, acts, None, np.random.default_rng(SEED + 2), base=hip)
