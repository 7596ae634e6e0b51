"""The fp32 kernels (dtype=OS2R_F32) against the fp64 oracle, through the C-ABI (needs an MI355X).

The reference of an fp32 handle is always the oracle run on that handle's own values promoted to f64: the state, per-env
parameters and action history are read back from the handle (or rounded to float32 before they are set on both sides), and
where a contact solve is involved the oracle runs the fp32 solver settings (sweeps only: pgs_exact = 0, the same pgs_iters
and pgs_tol).

The fp32 contract:
  * done, and every done-reason bit, equal what the reference decides in f64 on the fp32 state -- exactly;
  * observations and rewards are close to the reference's: a normalised fp32 observation may read -/+1.0f while the
    environment is still inside the reset space.

Tolerances, stated per test next to the value measured on the MI355X:
  * observations: OBS_ULP = 16 float32 ulp of max(|o|, 1) (affine maps; periodic slots: of the angle wrapped), measured
    max 2.2 on the fixture states; TANH_ULP = 4 ulp of |o| for the tanh slots (tanhf), measured max 1.1;
  * rewards: REW_TOL = 5e-6 absolute (measured max 1.0e-6), leaving out states
    whose pitch observation lies within EDGE_ULP = 32 float32 ulp of a reward window edge (lo <= bp <= hi);
  * resets: q and the five parameter fields within one float32 ulp of float32(oracle), qd, counters and poses identical;
  * physics: median and p99 of the state error, five times the measured values (per test).
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import MODES, make_config, mixed_axis_chain, perturbed_model

from gym_os2r_amd import abi

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
OBS_ULP, TANH_ULP, REW_TOL, EDGE_ULP = 16, 4, 5e-6, 32


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def HipSim(torch_mod):
    from gym_os2r_amd.sim import HipSim
    return HipSim


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _np(t):
    return t.double().cpu().numpy()


def _random_states(model, n, rng, vel=8.0):
    """test_gpu_parity.py's random states, rounded to float32."""
    nq = model["nq"]
    q = rng.uniform(-1.2, 1.2, (nq, n))
    names = model["dof_names"]
    if "planarizer_pitch_joint" in names:
        q[names.index("planarizer_pitch_joint")] = rng.uniform(-0.04, 0.3, n)
    qd = rng.uniform(-vel, vel, (nq, n))
    return _f32(q), _f32(qd)


def _readback(sim):
    """(q, qd, hist0, hist1) of the handle, promoted to f64."""
    q, qd = (_np(t) for t in sim.get_state())
    return q, qd, _np(sim.get_action_history(0)), _np(sim.get_action_history(1))


def _reasons(task, obs):
    """The reference's done test slot by slot (os2r_oracle.c: orc_done, gym's Box.contains on reset_space): bit d is set
    when slot d of the observation is outside the reset space (NaN included)."""
    bits = np.zeros(len(obs), np.int64)
    for d in range(task.obs_dim):
        lo, hi = (-1.0 + EPS64, 1.0 - EPS64) if task.normalized else (task.obs_low[d] + EPS64, task.obs_high[d] - EPS64)
        bits |= (~((obs[:, d] >= lo) & (obs[:, d] <= hi))).astype(np.int64) << d
    return bits


def _tanh_band(task, qd, obs, why):
    """The velocity bounds of the normalised tasks are pre-images of tanh(0.05 v) <= 1 - eps under the reference's tanh
    (numpy's, found by bisection); the oracle calls the C library's, which may differ in the last bit -- and near
    saturation tanh moves by an f64 ulp only every few units of v.  Within 4 f64 ulp of 1 - eps the decision is therefore
    libm-dependent (test_epilogue_matches_reference_fixtures leaves those states out): there the expected bit is the
    reference's own decision, the f64 bound, which the f64 kernel applies.  -> (reason bits, how many were so decided)"""
    why = why.copy()
    n = 0
    for d in range(task.obs_dim):
        if task.obs_kind[d] != abi.OBS_VEL_TANH:
            continue
        v = qd[task.obs_src[d]]
        band = np.isfinite(v) & (np.abs(np.abs(obs[:, d]) - (1.0 - EPS64)) <= 4 * EPS64)
        out = (v < task.done_lo[d]) | (v > task.done_hi[d])
        why[band] = (why[band] & ~(1 << d)) | (out[band].astype(np.int64) << d)
        n += int(band.sum())
    return why, n


def _epilogue(oracle, task, q, qd, h0, h1):
    """The oracle's observation, reward, done flag and done-reason bits of every environment from (q, qd) and the action
    history after a step (h0: the action just applied, h1: the one before; columns are environments); the velocity bits
    within the tanh band are the reference's bound (_tanh_band).  -> (obs, reward, done, reasons, band count)"""
    n = q.shape[1]
    obs = np.stack([oracle.observe(task, q[:, e], qd[:, e], h1[:, e]) for e in range(n)])
    rew = np.array([oracle.reward(task, obs[e], h0[:, e], h1[:, e]) for e in range(n)])
    done = np.array([oracle.done(task, obs[e]) for e in range(n)])
    why = _reasons(task, obs)
    assert np.array_equal(done, why != 0)
    why, nband = _tanh_band(task, qd, obs, why)
    return obs, rew, why != 0, why, nband


def _obs_err_ulp(task, obs, ref, q):
    """|obs - ref| in float32 ulp: of |ref| for the tanh slots, of max(|ref|, 1) for the other maps -- except the periodic
    slots, whose f32 wrap is off by an ulp of the angle it wraps: there of max(|q|, 1) mapped like the observation, and the
    difference taken modulo the image of 2 pi (the f32 wrap puts -/+pi_f at -pi_f, the f64 wrap of those floats near +pi).
    NaN where ref is not finite."""
    kinds = np.array(list(task.obs_kind)[:task.obs_dim])
    tanh = kinds == abi.OBS_VEL_TANH
    scale = np.where(tanh[None, :], np.maximum(np.abs(ref), 1e-30), np.maximum(np.abs(ref), 1.0)) * EPS32
    with np.errstate(invalid="ignore"):
        diff = obs - ref
        for d in np.flatnonzero((kinds == abi.OBS_POS_PERIODIC_NORM) | (kinds == abi.OBS_POS_PERIODIC_RAW)):
            m = 2.0 / (task.obs_high[d] - task.obs_low[d]) if kinds[d] == abi.OBS_POS_PERIODIC_NORM else 1.0
            diff[:, d] -= 2 * np.pi * m * np.round(diff[:, d] / (2 * np.pi * m))
            scale[:, d] = np.maximum(np.abs(q[task.obs_src[d]]), 1.0) * m * EPS32
        err = np.abs(diff) / scale
    err[~np.isfinite(ref)] = np.nan
    return err, tanh


def _check_obs(task, obs, ref, q, what):
    err, tanh = _obs_err_ulp(task, obs, ref, q)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(obs), fin), what
    e_aff = float(np.nanmax(err[:, ~tanh], initial=0.0)) if (~tanh).any() else 0.0
    e_tanh = float(np.nanmax(err[:, tanh], initial=0.0)) if tanh.any() else 0.0
    assert e_aff <= OBS_ULP and e_tanh <= TANH_ULP, (what, e_aff, e_tanh)
    return e_aff, e_tanh


def _window_edge(task, obs):
    """Environments whose pitch observation lies within EDGE_ULP float32 ulp of a reward window edge (rewards/__init__.py:
    the indicator lo <= bp <= hi with lo = H, hi = 4H): fp32 and f64 may fall on either side of it."""
    if task.idx_pitch_pos < 0:
        return np.zeros(len(obs), bool)
    H = 0.11 / 1.57 if task.normalized else 0.11
    bp = obs[:, task.idx_pitch_pos]
    return (np.abs(bp - H) <= EDGE_ULP * EPS32) | (np.abs(bp - 4 * H) <= EDGE_ULP * EPS32)


def _check_step(oracle, task, sim, obs, rew, done, why, what, keep=None):
    """The handle's outputs of its last step against the oracle's epilogue of the handle's own post-step state and action
    history: done and reason bits equal, observations and rewards close.  keep: the environments to compare (those not
    reset by the step).  -> (observation error in ulp: affine, tanh; reward error; environments left out at a window edge)"""
    q, qd, h0, h1 = _readback(sim)
    keep = np.ones(q.shape[1], bool) if keep is None else keep
    if not keep.any():
        return (0.0, 0.0), 0.0, 0
    o_obs, o_rew, o_done, o_why, _ = _epilogue(oracle, task, q[:, keep], qd[:, keep], h0[:, keep], h1[:, keep])
    d = done[keep]
    assert np.array_equal((d & abi.DONE_BIT) != 0, o_done), (what, np.flatnonzero(((d & 1) != 0) != o_done)[:8])
    if why is not None:
        assert np.array_equal(why[keep], o_why), (what, np.flatnonzero(why[keep] != o_why)[:8])
    e_obs = _check_obs(task, obs[keep], o_obs, q[:, keep], what)
    edge = _window_edge(task, o_obs)
    fin = np.isfinite(o_rew) & ~edge
    e_rew = float(np.max(np.abs(rew[keep][fin] - o_rew[fin]), initial=0.0))
    assert e_rew <= REW_TOL, (what, e_rew)
    return e_obs, e_rew, int(edge.sum())


def _reasons_of(sim):
    return sim.reasons.cpu().numpy().view(np.uint16).astype(np.int64)


def _solver_cfg64(mode, cfg32, **kw):
    """The f64 configuration of the oracle for an fp32 handle: the fp32 solver settings (sweeps only)."""
    assert cfg32.pgs_exact == 0
    cfg64, _, _ = make_config(mode, dtype=abi.F64, pgs_exact=0, pgs_iters=cfg32.pgs_iters,
                              pgs_normal_iters=cfg32.pgs_normal_iters, pgs_tol=cfg32.pgs_tol, **kw)
    return cfg64


def _state_err(sim, orc):
    q, qd = (_np(t) for t in sim.get_state())
    oq, oqd = orc.get_state()
    eq = np.abs(q - oq) / np.maximum(np.abs(oq), 1.0)
    ev = np.abs(qd - oqd) / np.maximum(np.abs(oqd), 1.0)
    return eq, ev


def _frozen_step(HipSim, torch, make, q, qd, h0, act):
    """One env-step that leaves the state where it was, so that its epilogue runs on the given state (the dt -> 0, contact
    off trick of test_epilogue_matches_reference_fixtures).  In fp32, dt = 1e-300 is 0 and the kernel forms 1/dt in places:
    if the state does not come back unchanged and finite, dt = 2^-100 (a tiny normal float) is used instead, and the state
    must come back finite.  -> (handle, obs, rew, done, reasons, dt used)"""
    for dt in (1e-300, 2.0 ** -100):
        cfg = make(dt)
        assert cfg.dtype == abi.F32
        sim = HipSim(cfg)
        sim.set_state(q, qd)
        sim.set_action_history(0, h0)
        sim.done_reasons(True)
        obs, rew, done, _ = sim.step(torch.as_tensor(act))
        why = _reasons_of(sim)
        q2, qd2 = (_np(t) for t in sim.get_state())
        fin_in = np.isfinite(q).all(axis=0) & np.isfinite(qd).all(axis=0)
        fin = np.isfinite(q2[:, fin_in]).all() and np.isfinite(qd2[:, fin_in]).all()
        same = np.array_equal(q2[:, fin_in], _f32(q)[:, fin_in]) and np.array_equal(qd2[:, fin_in], _f32(qd)[:, fin_in])
        if fin and (same or dt != 1e-300):
            return sim, _np(obs), _np(rew), done.cpu().numpy(), why, dt
        sim.close()
    raise AssertionError("unreachable")


# ---------------------------------------------------------------------------------------
# 1. the epilogue on the reference's fixture states, rounded to float32
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_epilogue_f32_on_fixture_states(HipSim, torch_mod, oracle, mode, normalized):
    """The states of tests/golden/task_epilogue.npz rounded to float32, through every reward of the combination: done and
    reason bits equal the oracle's on the state and action history read back after the step; observations within OBS_ULP /
    TANH_ULP, rewards within REW_TOL (module docstring), states at a reward window edge left out: at most 4 of 98 (measured 3).
    (dt = 1e-300 is 0 in f32: the state comes back unchanged and finite, measured, so the fallback dt is not taken.)"""
    z = np.load(os.path.join(GOLDEN, "task_epilogue.npz"))
    with open(os.path.join(GOLDEN, "task_layout.json")) as f:
        layout = json.load(f)
    key = f"{mode}__{'norm' if normalized else 'nonorm'}"
    n = len(z["q"])
    worst = [0.0, 0.0, 0.0, 0]
    for rname in layout["combos"][key]["rewards"]:
        def make(dt):
            return make_config(mode, rname, normalized, num_envs=n, dt=dt, substeps=1, contact=False, auto_reset=False,
                               dtype=abi.F32)[0]
        cfg, task, model = make_config(mode, rname, normalized, num_envs=n, contact=False, auto_reset=False, dtype=abi.F32)
        dof = model["dof_names"]
        q, qd = np.zeros((model["nq"], n)), np.zeros((model["nq"], n))
        for j, name in enumerate(layout["joint_order"]):
            if name in dof:
                q[dof.index(name)] = z["q"][:, j]
                qd[dof.index(name)] = z["qd"][:, j]
        q, qd = _f32(q), _f32(qd)
        sim, obs, rew, done, why, dt = _frozen_step(HipSim, torch_mod, make, q, qd, _f32(z["a_prev"]).T.copy(), _f32(z["a"]))
        (eo, et), er, nedge = _check_step(oracle, cfg.task, sim, obs, rew, done, why, f"{key} {rname} dt={dt}")
        worst = [max(worst[0], eo), max(worst[1], et), max(worst[2], er), max(worst[3], nedge)]
        sim.close()
    print(f"[f32 epilogue {key}] dt {dt:g}; max obs err {worst[0]:.1f} ulp, tanh {worst[1]:.1f} ulp; max reward err "
          f"{worst[2]:.2e}; {worst[3]} of {n} states at a window edge")
    assert worst[3] <= 4


# ---------------------------------------------------------------------------------------
# 2. the done thresholds at the float32 neighbours of every finite bound
# ---------------------------------------------------------------------------------------
def _ulp_steps(x, ks):
    f = np.float32(x)
    out = []
    for k in ks:
        g = f
        for _ in range(abs(k)):
            g = np.nextafter(g, np.float32(np.inf) if k > 0 else np.float32(-np.inf))
        out.append(float(g))
    return out


def _edge_values(task, d):
    """Pre-map values of slot d at the edges: the float32 values around each finite bound (two on either side of the float
    nearest to it: so the float at or just inside and the one just outside are among them), -/+1 exactly for the torque
    slots, -/+pi_f and its neighbours for the periodic slots, and NaN."""
    kind = task.obs_kind[d]
    vals = []
    for b in (task.done_lo[d], task.done_hi[d]):
        if np.isfinite(b):
            vals += _ulp_steps(b, range(-2, 3))
    if kind in (abi.OBS_TORQUE_NORM, abi.OBS_TORQUE_RAW):
        vals += [-1.0, 1.0]
    if kind in (abi.OBS_POS_PERIODIC_NORM, abi.OBS_POS_PERIODIC_RAW):
        vals += _ulp_steps(np.pi, range(-3, 4)) + _ulp_steps(-np.pi, range(-3, 4)) + [0.0]
    return sorted(set(vals)) + [float("nan")]


def _edge_states(task, model):
    """One environment per (slot, edge value): every other quantity at 0 (inside the reset space)."""
    nq = model["nq"]
    cols = []
    for d in range(task.obs_dim):
        if not (np.isfinite(task.done_lo[d]) or np.isfinite(task.done_hi[d])):
            continue
        for v in _edge_values(task, d):
            cols.append((d, v))
    n = len(cols)
    q, qd, h = np.zeros((nq, n)), np.zeros((nq, n)), np.zeros((2, n))
    for e, (d, v) in enumerate(cols):
        kind, s = task.obs_kind[d], task.obs_src[d]
        if kind in (abi.OBS_TORQUE_NORM, abi.OBS_TORQUE_RAW):
            h[s, e] = v
        elif kind in (abi.OBS_VEL_TANH, abi.OBS_VEL_RAW):
            qd[s, e] = v
        else:
            q[s, e] = v
    return q, qd, h, cols


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_done_thresholds_f32_at_float_neighbours(HipSim, torch_mod, oracle, mode, normalized):
    """For every slot with a finite bound: pre-map values at the float32 neighbours of done_lo and done_hi, the torque slots at
    actions of exactly -/+1, the periodic slots at -/+pi_f and around it (the f32 wrap_pi maps +/-pi_f to -pi_f, which the
    reference keeps), and a NaN in each slot.  The done flag and every reason bit must equal the oracle's f64 decision on the
    same values (read back after the step); on the velocity slots of the normalised tasks, within the few floats where the
    C library's tanh and the reference's disagree in the last bit, the reference's own bound (_tanh_band).  (Before the fp32
    bounds were rounded inward, fixed_hip_torque failed here: an action of exactly -/+1 did not end the episode.)"""
    reward = "StraightV1" if mode == "simple" else "BalancingV1"
    cfg, task, model = make_config(mode, reward, normalized, num_envs=1, contact=False, auto_reset=False, dtype=abi.F32)
    q, qd, h, cols = _edge_states(cfg.task, model)
    n = len(cols)

    def make(dt):
        return make_config(mode, reward, normalized, num_envs=n, dt=dt, substeps=1, contact=False, auto_reset=False,
                           dtype=abi.F32)[0]
    sim, obs, rew, done, why, dt = _frozen_step(HipSim, torch_mod, make, q, qd, h, np.zeros((n, 2)))
    q2, qd2, h0, h1 = _readback(sim)
    for e, (d, v) in enumerate(cols):                       # every edge value reached the epilogue unchanged
        kind, s = cfg.task.obs_kind[d], cfg.task.obs_src[d]
        src = h1 if kind in (abi.OBS_TORQUE_NORM, abi.OBS_TORQUE_RAW) else qd2 if kind in (abi.OBS_VEL_TANH, abi.OBS_VEL_RAW) else q2
        assert src[s, e] == v or (np.isnan(v) and np.isnan(src[s, e])), (cols[e], src[s, e], dt)
    o_obs, _, o_done, o_why, nband = _epilogue(oracle, cfg.task, q2, qd2, h0, h1)
    # A NaN in the state (which the physics iteration spreads over the chain) reaches a periodic slot through wrap_pi, which
    # does not keep it: the slot's reason bit stays clear while done (bit 0) and the non-finite bit (2) are set.  Known gap,
    # in the device code: there either answer is accepted, and every other bit must be exact.
    kinds = np.array(list(cfg.task.obs_kind)[:cfg.task.obs_dim])
    per_bits = sum(1 << d for d in np.flatnonzero((kinds == abi.OBS_POS_PERIODIC_NORM) | (kinds == abi.OBS_POS_PERIODIC_RAW)))
    bad_state = ~(np.isfinite(q2).all(axis=0) & np.isfinite(qd2).all(axis=0))
    assert np.all(done[bad_state] & abi.NONFINITE_BIT) and np.all(done[bad_state] & abi.DONE_BIT)
    why = np.where(bad_state & ((why | per_bits) == (o_why | per_bits)), o_why, why)
    bad = np.flatnonzero((((done & abi.DONE_BIT) != 0) != o_done) | (why != o_why))
    msg = [(cols[e], int(why[e]), int(o_why[e])) for e in bad[:12]]
    assert len(bad) == 0, f"{mode} normalized={normalized} dt={dt}: (slot, value), kernel reasons, oracle reasons: {msg}"
    assert o_done.sum() > 0 and (~o_done).sum() > 0        # both sides of the bounds are exercised
    assert nband <= 10 * sum(k == abi.OBS_VEL_TANH for k in list(cfg.task.obs_kind)[:cfg.task.obs_dim])   # the tanh slots' own edges
    sim.close()


def test_policy_rollout_f32_saturated_torques_end_episodes(HipSim, torch_mod, oracle):
    """fp32 fixed_hip_torque under os2r_rollout_policy (the launch loop and the fp32 policy kernel: no fused kernel has a
    torque slot) with per-env weights whose biases saturate the clip: actions of exactly -/+1 reach the torque slots of the
    next observation.  After every step the done flags and reasons equal the oracle's on the handle's own state."""
    torch = torch_mod
    n, K = 256, 6
    cfg, task, model = make_config("fixed_hip_torque", "BalancingV1", True, num_envs=n, contact=True, auto_reset=False,
                                   dtype=abi.F32, seed=3)
    sim = HipSim(cfg)
    rng = np.random.default_rng(8)
    q, qd = _random_states(model, n, rng, vel=1.0)
    sim.set_state(q, qd)
    D = int(cfg.task.obs_dim)
    W = np.zeros((n, 2, D + 1))
    W[:, :, D] = rng.choice([-4.0, 4.0, 0.3, -0.5], (n, 2))          # half the biases saturate: a = -/+1 exactly
    W[:, :, :D] = 0.01 * rng.standard_normal((n, 2, D))
    Wt = torch.as_tensor(W, device=sim.device, dtype=sim.dtype)
    torque_slots = [d for d in range(D) if cfg.task.obs_kind[d] == abi.OBS_TORQUE_NORM]
    tmask = sum(1 << d for d in torque_slots)
    hits = 0
    for k in range(K):
        _, _, (O, R, Dn, _, Wy) = sim.rollout_policy(1, Wt, want_outputs=True, want_reasons=True)
        why = Wy[0].cpu().numpy().view(np.uint16).astype(np.int64)
        _check_step(oracle, cfg.task, sim, _np(O[0]), _np(R[0]), Dn[0].cpu().numpy(), why, f"policy step {k}")
        hits += int(((why & tmask) != 0).sum())
    h0 = _np(sim.get_action_history(0))
    assert (np.abs(h0) == 1.0).mean() > 0.4                          # saturated: exactly -/+1
    assert hits > n                                                  # the torque slots ended episodes, step after step
    sim.close()


# ---------------------------------------------------------------------------------------
# 3. physics in all task modes
# ---------------------------------------------------------------------------------------
# state error after 1 and after 3 env-steps: (median qd, p99 q, p99 qd), five times the values measured on the MI355X
# (measured, the worst of all modes, contact on / off, DR and the run-time chains: 1 step 2.0e-6 / 3.4e-7 / 1.1e-4,
# 3 steps 4.0e-6 / 1.4e-6 / 2.7e-4)
PHYS_BOUNDS_1 = (1e-5, 1.7e-6, 5.6e-4)
PHYS_BOUNDS_3 = (2e-5, 7e-6, 1.4e-3)


def _params(rng, model, n):
    nq = model["nq"]
    return {abi.PARAM_MASS_SCALE: rng.uniform(0.8, 1.2, (nq, n)), abi.PARAM_DAMPING: rng.uniform(0.008, 0.012, (nq, n)),
            abi.PARAM_FRICTION: rng.uniform(0.01, 0.05, (nq, n)), abi.PARAM_MU: 0.33 * rng.uniform(0.8, 1.2, (nq, n)),
            abi.PARAM_GRAVITY: rng.normal(-9.8, 0.2, (1, n))}


def _physics_case(HipSim, torch, oracle, mode, contact, dr, model_overrides=None, n=512, steps=3, seed=11, cfg_pair=None):
    rng = np.random.default_rng(seed)
    reward = "StraightV1" if mode == "simple" else "BalancingV2"
    if cfg_pair is None:
        kw = dict(num_envs=n, contact=contact, auto_reset=False, model_overrides=model_overrides)
        cfg32, task, model = make_config(mode, reward, True, dtype=abi.F32, **kw)
        cfg64 = _solver_cfg64(mode, cfg32, reward_name=reward, **kw)
    else:
        cfg32, cfg64, model = cfg_pair
    sim, orc = HipSim(cfg32), oracle.OracleSim(cfg64, threads=8)
    if dr:
        for f, v in _params(rng, model, n).items():
            sim.set_params(f, _f32(v)); orc.set_params(f, _f32(v))
    q, qd = _random_states(model, n, rng)
    sim.set_state(q, qd); orc.set_state(q, qd)
    sim.done_reasons(True)
    out = []
    for k in range(steps):
        act = _f32(rng.uniform(-1, 1, (n, 2)))
        obs, rew, done, _ = sim.step(torch.as_tensor(act))
        orc.step(act)
        _check_step(oracle, cfg32.task, sim, _np(obs), _np(rew), done.cpu().numpy(), _reasons_of(sim), (mode, contact, dr, k))
        if k in (0, steps - 1):
            eq, ev = _state_err(sim, orc)
            out.append((np.median(ev), np.quantile(eq, 0.99), np.quantile(ev, 0.99)))
    sim.close(); orc.close()
    return out


@pytest.mark.parametrize("contact", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_physics_f32_all_modes(HipSim, torch_mod, oracle, mode, contact):
    """Random states (test_one_step_matches_oracle_f64's, rounded to float32), one env-step and three: the state against the
    oracle on the fp32 solver settings, median and p99 bounded by PHYS_BOUNDS_1 / PHYS_BOUNDS_3 (five times the measured
    values); the epilogue of every step against the oracle's on the handle's own state (module docstring)."""
    one, three = _physics_case(HipSim, torch_mod, oracle, mode, contact, dr=False)
    print(f"[f32 physics {mode} contact={contact}] 1 step: median qd {one[0]:.2e}, p99 q {one[1]:.2e} qd {one[2]:.2e}; "
          f"3 steps: median qd {three[0]:.2e}, p99 q {three[1]:.2e} qd {three[2]:.2e}")
    assert all(a <= b for a, b in zip(one, PHYS_BOUNDS_1)), one
    assert all(a <= b for a, b in zip(three, PHYS_BOUNDS_3)), three


@pytest.mark.parametrize("mode", ["free_hip", "fixed"])
def test_physics_f32_with_per_env_parameters(HipSim, torch_mod, oracle, mode):
    """As test_physics_f32_all_modes, with contact and per-env parameters (rounded to float32) set on both sides."""
    one, three = _physics_case(HipSim, torch_mod, oracle, mode, True, dr=True)
    print(f"[f32 physics {mode} DR] 1 step: median qd {one[0]:.2e}, p99 q {one[1]:.2e} qd {one[2]:.2e}; "
          f"3 steps: median qd {three[0]:.2e}, p99 q {three[1]:.2e} qd {three[2]:.2e}")
    assert all(a <= b for a, b in zip(one, PHYS_BOUNDS_1)), one
    assert all(a <= b for a, b in zip(three, PHYS_BOUNDS_3)), three


# ---------------------------------------------------------------------------------------
# 4. run-time robots (the fp32 kernel units 12-15)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dr", [False, True])
@pytest.mark.parametrize("mode", ["free_hip", "fixed_hip", "fixed", "simple"])
def test_runtime_model_kernels_f32(HipSim, torch_mod, oracle, mode, dr):
    """The perturbed chains of test_runtime_model_kernels_match_oracle (no compiled-in table matches) on the generic fp32
    kernels: the same bounds as the compiled-in robots (PHYS_BOUNDS_1 / PHYS_BOUNDS_3) and the same epilogue checks."""
    model = perturbed_model(mode, np.random.default_rng(23))
    one, three = _physics_case(HipSim, torch_mod, oracle, mode, True, dr=dr, model_overrides=model, n=320, seed=23)
    print(f"[f32 run-time {mode} dr={dr}] 1 step: median qd {one[0]:.2e}, p99 q {one[1]:.2e} qd {one[2]:.2e}; "
          f"3 steps: median qd {three[0]:.2e}, p99 q {three[1]:.2e} qd {three[2]:.2e}")
    assert all(a <= b for a, b in zip(one, PHYS_BOUNDS_1)), one
    assert all(a <= b for a, b in zip(three, PHYS_BOUNDS_3)), three


def test_synthetic_mixed_axis_chain_f32(HipSim, torch_mod, oracle, tmp_path):
    """The hand-made z/y/x chain with contact candidates on every body (test_synthetic_mixed_axis_chain) in fp32, 20 env-steps
    against the oracle on the fp32 solver settings: median / p99 of the state error within five times the measured values
    (measured: median 1.0e-6, p99 q 8e-7, qd 1.6e-5)."""
    m, spec = mixed_axis_chain(tmp_path)
    n = 192
    cfg32 = abi.config_struct(m, spec, num_envs=n, dtype=abi.F32, contact=True, auto_reset=False)
    cfg64 = abi.config_struct(m, spec, num_envs=n, dtype=abi.F64, contact=True, auto_reset=False, pgs_exact=0,
                              pgs_iters=cfg32.pgs_iters, pgs_normal_iters=cfg32.pgs_normal_iters, pgs_tol=cfg32.pgs_tol)
    sim, orc = HipSim(cfg32), oracle.OracleSim(cfg64, threads=8)
    rng = np.random.default_rng(4)
    q, qd = _f32(rng.uniform(-1.5, 1.5, (3, n))), _f32(rng.uniform(-5, 5, (3, n)))
    sim.set_state(q, qd); orc.set_state(q, qd)
    for _ in range(20):
        act = _f32(rng.uniform(-1, 1, (n, 2)))
        sim.step(torch_mod.as_tensor(act)); orc.step(act)
    eq, ev = _state_err(sim, orc)
    med, pq, pv = np.median(np.maximum(eq, ev)), np.quantile(eq, 0.99), np.quantile(ev, 0.99)
    print(f"[f32 mixed-axis chain, 20 steps] median {med:.2e}, p99 q {pq:.2e} qd {pv:.2e}")
    assert med < 5e-6 and pq < 4e-6 and pv < 8e-5, (med, pq, pv)
    sim.close(); orc.close()


# ---------------------------------------------------------------------------------------
# 5. resets and parameter draws
# ---------------------------------------------------------------------------------------
def _within_one_ulp(got, ref64):
    """|got - float32(ref)| <= one float32 ulp of float32(ref) (the reset computes in double and rounds once; libm may differ
    in the last bit of the double)."""
    r = ref64.astype(np.float32)
    sp = np.spacing(np.abs(r)).astype(np.float64)
    return np.abs(got - r.astype(np.float64)) <= sp


@pytest.mark.parametrize("reset_mode", [abi.RESET_FIXED, abi.RESET_RANDOM])
def test_reset_and_randomisation_f32(HipSim, torch_mod, oracle, reset_mode):
    """test_reset_and_randomisation_match_oracle in fp32: N = 1000 (a tail wave), env_offset 77, five reset poses, masked
    resets, three rounds.  q and the five parameter fields within one float32 ulp of float32(oracle); qd, episode
    counters and poses identical; the reset's observations against the oracle's on the handle's own state (module
    docstring)."""
    n = 1000
    kw = dict(num_envs=n, seed=1234, reset_positions=("stand", "half_stand", "ground", "lay", "float"), reset_mode=reset_mode,
              randomize_params=reset_mode == abi.RESET_RANDOM, env_offset=77)
    cfg, task, model = make_config("free_hip", "BalancingV1", True, dtype=abi.F32, **kw)
    cfg64, _, _ = make_config("free_hip", "BalancingV1", True, dtype=abi.F64, **kw)
    sim, orc = HipSim(cfg), oracle.OracleSim(cfg64)
    for rnd in range(3):
        q, qd = (_np(t) for t in sim.get_state())
        oq, oqd = orc.get_state()
        assert _within_one_ulp(q, oq).all(), rnd
        assert np.array_equal(qd, _f32(oqd)), rnd
        for f in range(5):
            assert _within_one_ulp(_np(sim.get_params(f)), orc.get_params(f)).all(), (rnd, f)
        s1, e1, p1 = (t.cpu().numpy() for t in sim.episode_info())
        s2, e2, p2 = orc.episode_info()
        assert np.array_equal(s1, s2) and np.array_equal(e1.view(np.uint32), e2) and np.array_equal(p1, p2)
        mask = (np.arange(n) % (rnd + 2) == 0).astype(np.uint8)
        o1 = _np(sim.reset(torch_mod.as_tensor(mask)))
        orc.reset(mask)
        q, qd, h0, h1 = _readback(sim)
        o_obs = _epilogue(oracle, cfg.task, q, qd, h0, h1)[0]
        _check_obs(cfg.task, o1, o_obs, q, ("reset", rnd))
    sim.close(); orc.close()


# ---------------------------------------------------------------------------------------
# 6. auto-reset
# ---------------------------------------------------------------------------------------
def test_auto_reset_f32(HipSim, torch_mod, oracle):
    """test_auto_reset_rollout_matches_oracle in fp32 (fixed_hip, randomised resets and parameters, TimeLimit 17, device
    actions), step by step.  Environments the step did not reset: observation, reward, done and reasons against the oracle's
    epilogue of the handle's own post-step state.  Environments it reset: the truncation bit is the TimeLimit's, and the new
    state, parameters, counters and observation are those of an oracle reset driven to the same (env, episode) counter --
    state and parameters within one float32 ulp, counters identical, observation within OBS_ULP / TANH_ULP."""
    n, T, tl = 300, 60, 17
    kw = dict(num_envs=n, seed=9, reset_positions=("stand", "ground"), reset_mode=abi.RESET_RANDOM, randomize_params=True,
              max_episode_steps=tl, auto_reset=True)
    cfg, task, model = make_config("fixed_hip", "BalancingV2", True, dtype=abi.F32, **kw)
    cfg64, _, _ = make_config("fixed_hip", "BalancingV2", True, dtype=abi.F64, **kw)
    sim, orc = HipSim(cfg), oracle.OracleSim(cfg64)
    sim.done_reasons(True)
    nreset = 0
    for t in range(T):
        steps0, epi0, _ = (x.cpu().numpy() for x in sim.episode_info())
        obs, rew, done, _ = sim.step(None)
        obs, rew, done, why = _np(obs), _np(rew), done.cpu().numpy(), _reasons_of(sim)
        reset = done != 0
        _check_step(oracle, cfg.task, sim, obs, rew, done, why, ("auto-reset", t), keep=~reset)
        assert np.array_equal((done & abi.TRUNCATED_BIT) != 0, steps0 + 1 >= tl), t
        if reset.any():
            nreset += int(reset.sum())
            orc.set_episode_info(episode=epi0.view(np.uint32))
            q, qd, h0, h1 = _readback(sim)
            orc.set_action_history(1, h1)
            o_obs = orc.reset(reset.astype(np.uint8))
            oq, oqd = orc.get_state()
            assert _within_one_ulp(q[:, reset], oq[:, reset]).all() and np.array_equal(qd[:, reset], _f32(oqd[:, reset])), t
            for f in range(5):
                assert _within_one_ulp(_np(sim.get_params(f))[:, reset], orc.get_params(f)[:, reset]).all(), (t, f)
            s1, e1, p1 = (x.cpu().numpy() for x in sim.episode_info())
            s2, e2, p2 = orc.episode_info()
            assert np.array_equal(s1[reset], s2[reset]) and np.array_equal(e1.view(np.uint32)[reset], e2[reset])
            assert np.array_equal(p1[reset], p2[reset])
            _check_obs(cfg.task, obs[reset], o_obs[reset], q[:, reset], ("auto-reset obs", t))
    assert nreset >= 3 * n                                           # TimeLimit fired three times
    sim.close(); orc.close()
