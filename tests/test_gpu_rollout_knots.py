"""os2rr_rollout_policy_recorded (include/os2r_record.h, libos2r_record.so) on the MI355X: a policy rollout that records its knots into another handle in the
same launch.  Every comparison is torch.equal, and every yardstick is a path that existed before the entry point: per env-step
one copy_envs_from(sim, index_k) into a twin knots handle and one rollout_schedule(1, first_slot = k) on a twin of the handle
(`_composed`), and an unsplit unrecorded rollout_schedule(K) on a third twin for the returns and lengths.

N = 130 (two full waves and a tail of two lanes), K = 7, TimeLimit 5 with elapsed steps e mod 5 at the window's start (TimeLimit
auto-resets in every wave inside the window), randomised resets and parameters, robots on the ground after 150 random steps.  The
knots handles have (K + 3) N lanes and record from knot 2 on; they are pre-stepped, so a stray write into a lane that must stay
as it is shows."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from helpers import make_config
from gym_os2r_amd import abi
from test_gpu_policy_rollout import _assert_same_handle, _everything

pytestmark = pytest.mark.gpu

N, K, LIMIT, FIRST = 130, 7, 5, 2
PARAMS = (abi.PARAM_MASS_SCALE, abi.PARAM_DAMPING, abi.PARAM_FRICTION, abi.PARAM_MU, abi.PARAM_GRAVITY)
WANT = dict(want_outputs=True, want_terminal=True, want_reasons=True, want_actions=True)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def HipSim(torch_mod):
    from gym_os2r_amd.sim import HipSim
    return HipSim


def _make(torch, HipSim, mode, dtype, n=N, seed=5, warm=150, **kw):
    """The `_make` of test_gpu_policy_schedule.py with these sizes.  fp32 handles carry the solver's arrays unused: they are given
    values here, so that their copy is a check in fp32 too."""
    kw = {**dict(reset_mode=abi.RESET_RANDOM, randomize_params=True), **kw}
    cfg, _, _ = make_config(mode, "BalancingV2", True, num_envs=n, contact=True, seed=seed, max_episode_steps=LIMIT, dtype=dtype, **kw)
    sim = HipSim(cfg)
    for _ in range(warm):
        sim.step(None)
    sim.set_episode_info(steps=torch.arange(n, dtype=torch.int32, device=sim.device) % LIMIT)
    if dtype == abi.F32:
        g = torch.Generator().manual_seed(seed)
        lam = torch.randn(4 * sim.nq, n, generator=g, dtype=torch.float64).to(sim.device, sim.dtype)
        sim.set_solver_state(lam, (torch.arange(n, device=sim.device) % 7 + 1).to(torch.int32))
    return sim


def _make_knots(torch, HipSim, mode, dtype, **kw):
    """(K + 3) N lanes that hold something of their own: another seed, 20 random env-steps."""
    return _make(torch, HipSim, mode, dtype, n=(K + 3) * N, seed=9, warm=20, **kw)


def _table(torch, sim, T, per_env, seed=0, scale=0.6):
    g = torch.Generator().manual_seed(seed)
    shape = (sim.N, T, 2, sim.D + 1) if per_env else (T, 2, sim.D + 1)
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64)).to(sim.device, sim.dtype)


def _whole(sim):
    """Every array os2r_copy_envs can move, all lanes."""
    return tuple(_everything(sim)) + tuple(sim.get_params(f) for f in PARAMS)


def _same_knots(torch, ka, kb, what):
    for i, (x, y) in enumerate(zip(_whole(ka), _whole(kb))):
        assert torch.equal(x, y), (what, i, int((x != y).sum()))
    assert ka.step_count == kb.step_count, what


def _composed(torch, b, kb, W, first_slot=0, first_knot=FIRST, steps=K, state=True, params=True, **kw):
    """The loop the recorded call replaces, on paths that were there before it.  -> [(the 1-step call's result, the knot's
    observation as copy_envs_from reports it)] per env-step"""
    lanes = torch.arange(kb.N, dtype=torch.int32, device=kb.device)
    out = []
    for k in range(steps):
        lo = (first_knot + k) * b.N
        index = torch.where((lanes >= lo) & (lanes < lo + b.N), lanes - lo, -1).to(torch.int32)
        kobs = kb.copy_envs_from(b, index, state=state, params=params, want_obs=True)[lo:lo + b.N].clone()
        out.append((b.rollout_schedule(1, W, first_slot=first_slot + k, **{**WANT, **kw}), kobs))
    return out


def _assert_steps(torch, got, loop, k0=0, noise=False):
    """The per-step outputs, actions (noise) and knot observations of a recorded call against the loop's env-steps k0 ..."""
    _, _, outs, (act, eps), kobs = got
    for k in range(act.shape[0]):
        (_, _, o1, (a1, e1)), ko = loop[k0 + k]
        for x, y in zip(outs, o1):
            assert torch.equal(x[k], y[0]), k
        assert torch.equal(act[k], a1[0]), k
        if noise:
            assert torch.equal(eps[k], e1[0]), k
        if kobs is not None:
            assert torch.equal(kobs[k], ko), k


def _assert_setting(torch, loop, kb, dtype):
    """On the loop's results: the case tests what it claims."""
    done = torch.stack([r[0][2][2][0] for r in loop])                         # [K, N]
    assert bool((done[:K - 1] != 0).any())
    k, e = (int(v) for v in (done[:K - 1] != 0).nonzero()[0])
    steps, episode, _ = kb.episode_info()
    at = (FIRST + k) * N + e
    # the knot after the reset is the environment as the reset left it: next episode, no elapsed steps
    assert int(steps[at + N]) == 0 and int(episode[at + N]) == int(episode[at]) + 1
    mass = kb.get_params(abi.PARAM_MASS_SCALE)
    first, last = mass[:, FIRST * N:(FIRST + 1) * N], mass[:, (FIRST + K - 1) * N:(FIRST + K) * N]
    assert bool((first != last).any())                                         # a parameter row re-drawn inside the window
    flags = kb.get_solver_state()[1][FIRST * N:(FIRST + K) * N]
    assert bool((flags != 0).any())


class Yardstick:
    """The composed path of one configuration, computed once and kept: the twin's and the twin knots handle's arrays afterwards,
    the per-step results, and returns, lengths and outputs of an unsplit unrecorded call on a third twin."""

    def __init__(self, torch, HipSim, mode, dtype, per_env):
        b, kb, c = _make(torch, HipSim, mode, dtype), _make_knots(torch, HipSim, mode, dtype), _make(torch, HipSim, mode, dtype)
        self.W = _table(torch, b, 5, per_env)
        self.loop = _composed(torch, b, kb, self.W)
        _assert_setting(torch, self.loop, kb, dtype)
        self.unsplit = c.rollout_schedule(K, self.W, **WANT)
        _assert_same_handle(torch, b, c, "the loop of one-step calls is the unsplit call")
        self.sim, self.knots, self.count, self.knots_count = _whole(b), _whole(kb), b.step_count, kb.step_count
        self.kb = kb                                                            # kept for the consumer test (only read there)
        b.close(); c.close()

    def check(self, torch, a, ka, got, what):
        for i, (x, y) in enumerate(zip(_whole(a), self.sim)):
            assert torch.equal(x, y), (what, "sim", i)
        for i, (x, y) in enumerate(zip(_whole(ka), self.knots)):
            assert torch.equal(x, y), (what, "knots", i, int((x != y).sum()))
        assert a.step_count == self.count and ka.step_count == self.knots_count, what


@pytest.fixture(scope="module")
def yardsticks(torch_mod, HipSim):
    made = {}

    def get(mode, dtype, per_env):
        key = (mode, dtype, per_env)
        if key not in made:
            made[key] = Yardstick(torch_mod, HipSim, mode, dtype, per_env)
        return made[key]
    yield get
    for y in made.values():
        y.kb.close()


# ---------------------------------------------------------------------------------------
# 1. the fused kernel against the composed path
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_env", [False, True], ids=["shared", "per-env"])
@pytest.mark.parametrize("mode,dtype", [("free_hip", abi.F64), ("free_hip", abi.F32), ("fixed_hip_simple", abi.F64)],
                         ids=["free_hip-f64", "free_hip-f32", "fixed_hip_simple-f64"])
def test_recorded_rollout_equals_the_composed_path(HipSim, torch_mod, yardsticks, mode, dtype, per_env):
    torch = torch_mod
    y = yardsticks(mode, dtype, per_env)
    a, ka = _make(torch, HipSim, mode, dtype), _make_knots(torch, HipSim, mode, dtype)
    c0 = a.step_count
    got = a.rollout_schedule(K, y.W, knots=ka, first_knot=FIRST, want_knot_obs=True, **WANT)
    torch.cuda.synchronize()
    assert int(a.violation_mirror()[1]) == c0                  # one launch: the last one that started is the window's first
    y.check(torch, a, ka, got, (mode, dtype, per_env))
    _assert_steps(torch, got, y.loop)
    ret, length, outs, (act, _) = y.unsplit
    assert torch.equal(got[0], ret) and torch.equal(got[1], length) and torch.equal(got[3][0], act)
    for x, z in zip(got[2], outs):
        assert torch.equal(x, z)
    a.close(); ka.close()


# ---------------------------------------------------------------------------------------
# 2. what is selected moves, what is not stays
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("state,params", [(True, False), (False, True)], ids=["state-only", "params-only"])
def test_only_the_selected_arrays_are_recorded(HipSim, torch_mod, yardsticks, state, params):
    torch = torch_mod
    mode, dtype = "free_hip", abi.F64
    y = yardsticks(mode, dtype, False)
    a, ka = _make(torch, HipSim, mode, dtype), _make_knots(torch, HipSim, mode, dtype)
    b, kb = _make(torch, HipSim, mode, dtype), _make_knots(torch, HipSim, mode, dtype)
    before = _whole(ka)
    got = a.rollout_schedule(K, y.W, knots=ka, first_knot=FIRST, knot_state=state, knot_params=params, **WANT)
    assert len(got) == 5 and got[4] is None
    _composed(torch, b, kb, y.W, state=state, params=params)
    _same_knots(torch, ka, kb, (state, params))
    after, n_state = _whole(ka), len(before) - len(PARAMS)
    kept = range(n_state, len(before)) if state else range(n_state)
    moved = range(n_state) if state else range(n_state, len(before))
    for i in kept:
        assert torch.equal(after[i], before[i]), i
    assert any(not torch.equal(after[i], before[i]) for i in moved)
    for i, (x, z) in enumerate(zip(_whole(a), y.sim)):        # the handle that rolls out does what it always did
        assert torch.equal(x, z), i
    for s in (a, ka, b, kb):
        s.close()


# ---------------------------------------------------------------------------------------
# 3. a split window
# ---------------------------------------------------------------------------------------
def test_a_split_window_equals_the_whole(HipSim, torch_mod, yardsticks):
    torch = torch_mod
    mode, dtype = "free_hip", abi.F64
    y = yardsticks(mode, dtype, True)
    a, ka = _make(torch, HipSim, mode, dtype), _make_knots(torch, HipSim, mode, dtype)
    g1 = a.rollout_schedule(3, y.W, knots=ka, first_knot=FIRST, want_knot_obs=True, **WANT)
    g2 = a.rollout_schedule(4, y.W, first_slot=3, knots=ka, first_knot=FIRST + 3, want_knot_obs=True, **WANT)
    y.check(torch, a, ka, None, "3 + 4")
    _assert_steps(torch, g1, y.loop)
    _assert_steps(torch, g2, y.loop, k0=3)
    a.close(); ka.close()


# ---------------------------------------------------------------------------------------
# 4. exploration noise: recording draws nothing
# ---------------------------------------------------------------------------------------
def test_recording_with_noise(HipSim, torch_mod):
    torch = torch_mod
    mode, dtype = "free_hip", abi.F64
    a, ka, b, kb, c = (_make(torch, HipSim, mode, dtype), _make_knots(torch, HipSim, mode, dtype), _make(torch, HipSim, mode, dtype),
                       _make_knots(torch, HipSim, mode, dtype), _make(torch, HipSim, mode, dtype))
    W = _table(torch, a, 5, True, seed=3)
    noise = dict(sigma=0.3, salt=7, want_noise=True)
    got = a.rollout_schedule(K, W, knots=ka, first_knot=FIRST, want_knot_obs=True, **WANT, **noise)
    loop = _composed(torch, b, kb, W, **noise)
    ret, length, outs, (act, eps) = c.rollout_schedule(K, W, **WANT, **noise)      # the unrecorded noisy call
    assert float(eps.abs().max()) > 1.0
    assert torch.equal(got[3][0], act) and torch.equal(got[3][1], eps) and torch.equal(got[0], ret) and torch.equal(got[1], length)
    for x, z in zip(got[2], outs):
        assert torch.equal(x, z)
    _assert_steps(torch, got, loop, noise=True)
    _same_knots(torch, ka, kb, "noisy")
    _assert_same_handle(torch, a, b, "noisy")
    _assert_same_handle(torch, a, c, "noisy, unrecorded")
    for s in (a, ka, b, kb, c):
        s.close()


# ---------------------------------------------------------------------------------------
# 5. the launch loop
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["pgs_iters", "count_work"])
def test_the_launch_loop_records_the_same(HipSim, torch_mod, how):
    torch = torch_mod
    mode, dtype = "free_hip", abi.F64
    kw = dict(pgs_iters=abi.DEFAULT_PGS_ITERS + 3) if how == "pgs_iters" else {}
    a, b = _make(torch, HipSim, mode, dtype, **kw), _make(torch, HipSim, mode, dtype, **kw)
    ka, kb = _make_knots(torch, HipSim, mode, dtype), _make_knots(torch, HipSim, mode, dtype)
    if how == "count_work":
        a.count_work(True); b.count_work(True)
    W = _table(torch, a, 5, True, seed=4)
    c0 = a.step_count
    got = a.rollout_schedule(K, W, knots=ka, first_knot=FIRST, want_knot_obs=True, **WANT)
    torch.cuda.synchronize()
    assert int(a.violation_mirror()[1]) == c0 + K - 1          # a step launch per env-step
    loop = _composed(torch, b, kb, W)
    _assert_setting(torch, loop, kb, dtype)
    _assert_steps(torch, got, loop)
    _same_knots(torch, ka, kb, how)
    _assert_same_handle(torch, a, b, how)
    for i, (x, z) in enumerate(zip(_whole(a), _whole(b))):
        assert torch.equal(x, z), i
    if how == "count_work":
        assert a.work_counters()["wave_iterations"] > 0
        a.count_work(False); b.count_work(False)
    for s in (a, ka, b, kb):
        s.close()


# ---------------------------------------------------------------------------------------
# 6. a consumer: the recorded handle linearizes and steps like the composed one
# ---------------------------------------------------------------------------------------
def test_the_recorded_handle_linearizes_and_steps_per_lane(HipSim, torch_mod):
    """The knots handles are created with fixed resets and nominal parameters: their kernels read the parameter arrays per lane
    only after the parameter copy (os2r_copy_envs' rule); a recorded handle that kept the nominal ones would step differently."""
    torch = torch_mod
    mode, dtype = "free_hip", abi.F64
    nominal = dict(reset_mode=abi.RESET_FIXED, randomize_params=False)
    a, b = _make(torch, HipSim, mode, dtype), _make(torch, HipSim, mode, dtype)
    ka, kb = _make_knots(torch, HipSim, mode, dtype, **nominal), _make_knots(torch, HipSim, mode, dtype, **nominal)
    W = _table(torch, a, 5, False, seed=5)
    got = a.rollout_schedule(K, W, knots=ka, first_knot=FIRST, want_knot_obs=True, **WANT)
    loop = _composed(torch, b, kb, W)
    _assert_steps(torch, got, loop)
    _same_knots(torch, ka, kb, "nominal knots")
    scale = ka.get_params(abi.PARAM_MASS_SCALE)[:, FIRST * N:(FIRST + K) * N]
    assert bool((scale != 1.0).any())                           # per-environment parameters arrived
    actions = torch.zeros(ka.N, 2, dtype=ka.dtype, device=ka.device)
    actions[FIRST * N:(FIRST + K) * N] = got[3][0].view(K * N, 2)
    for x, z in zip(ka.linearize(actions), kb.linearize(actions)):
        assert torch.equal(x, z)
    for x, z in zip(ka.step(actions), kb.step(actions)):
        assert torch.equal(x, z)
    _same_knots(torch, ka, kb, "after a step")
    for s in (a, ka, b, kb):
        s.close()


# ---------------------------------------------------------------------------------------
# the refusals behind valid handles: each has its own text, nothing is written
# ---------------------------------------------------------------------------------------
def test_refusals_behind_valid_handles(HipSim, torch_mod):
    torch = torch_mod
    from gym_os2r_amd.sim import _ptr
    a = _make(torch, HipSim, "free_hip", abi.F64, warm=3)
    ka = _make(torch, HipSim, "free_hip", abi.F64, n=3 * N, seed=9, warm=3)
    k32 = _make(torch, HipSim, "free_hip", abi.F32, n=3 * N, warm=3)
    other = _make(torch, HipSim, "fixed_hip_simple", abi.F64, n=3 * N, warm=3)
    from gym_os2r_amd import _lib
    lib, rec, st = a._lib, _lib.load_record(), a._stream()
    W = _table(torch, a, 5, False)
    buf = torch.full((3, N, a.D), 7.0, dtype=a.dtype, device=a.device)
    eps = torch.zeros(3, N, 2, dtype=a.dtype, device=a.device)
    both = abi.COPY_STATE | abi.COPY_PARAMS
    before, before_k, count = _whole(a), _whole(ka), a.step_count

    def call(knots=ka, first_knot=0, what=both, kobs=buf, nsteps=3, w=W, period=5, first=0, flags=0, salt=0, noise=None):
        return rec.os2rr_rollout_policy_recorded(a._h, None if knots is None else knots._h, first_knot, what, _ptr(kobs), nsteps, _ptr(w),
                                                period, first, flags, None, salt, None, None, None, None, None, None, None, None,
                                                _ptr(noise), st)
    cases = [(dict(nsteps=0), "nsteps must be >= 1"), (dict(period=0), "period must be >= 1"), (dict(first=-1), "first_slot must be >= 0"),
             (dict(w=None), "null weights"), (dict(flags=64), "unknown flag bits"), (dict(noise=eps), "noise_dev needs sigma_dev"),
             (dict(salt=9), "a non-zero salt needs sigma_dev"),
             (dict(knots=None, kobs=None), "knots and knot_obs_dev are both null"), (dict(knots=a), "another handle"),
             (dict(knots=k32), "differ in dtype"), (dict(knots=other), "different robot models"),
             (dict(what=0), "nothing selected (what == 0)"), (dict(what=4), "unknown bits in what"), (dict(what=both | 8), "unknown bits in what"),
             (dict(first_knot=-1), "first_knot must be >= 0"),
             (dict(first_knot=1), f"knots has {3 * N} environments, (first_knot + nsteps) * num_envs = {4 * N} are needed"),
             (dict(first_knot=2 ** 31 - 1), f"(first_knot + nsteps) * num_envs = {(2 ** 31 + 2) * N} are needed")]
    texts = set()
    for kw, text in cases:
        assert call(**kw) == abi.ERR_INVALID, kw
        msg = lib.os2r_last_error(a._h).decode()
        assert msg.startswith("os2rr_rollout_policy_recorded: ") and text in msg, (kw, msg)
        texts.add(msg)
    assert len(texts) == len(cases) - 1                         # every cause its own text (the unknown bit twice)
    torch.cuda.synchronize()
    for x, z in zip(before + before_k, _whole(a) + _whole(ka)):
        assert torch.equal(x, z)
    assert a.step_count == count and bool((buf == 7.0).all())
    # what and first_knot are not looked at without a knots handle; either sink alone is enough
    assert call(knots=None, what=0, first_knot=-5) == abi.OK and call(kobs=None) == abi.OK
    torch.cuda.synchronize()
    assert a.step_count == count + 6 and not bool((buf == 7.0).any())
    for s in (a, ka, k32, other):
        s.close()


# ---------------------------------------------------------------------------------------
# 7. a custom robot's own code objects
# ---------------------------------------------------------------------------------------
JIT_K, JIT_N = 6, 200


def _jit_run(torch, HipSim, recorded, path=None):
    """The robot, configuration and start of tests/test_gpu_jit_fused.py (lying states, per-env parameters, three warm-up steps),
    then the window: recorded, or composed.  -> every result as a flat list of tensors (saved to `path` for a child process)"""
    import numpy as np
    from helpers import lying_states
    from test_jit_fused_host import config, robot

    def make(n, seed):
        sim = HipSim(config(abi.F64, n, auto_reset=True, max_episode_steps=5, seed=seed))
        assert sim.specialised
        return sim
    sim, knots = make(JIT_N, 5), make((JIT_K + 1) * JIT_N, 9)
    rng = np.random.default_rng(11)
    q, qd = lying_states(robot(), JIT_N, rng)
    nq = sim.nq
    for f, v in ((abi.PARAM_MASS_SCALE, rng.uniform(0.8, 1.2, (nq, JIT_N))), (abi.PARAM_DAMPING, rng.uniform(0.008, 0.012, (nq, JIT_N))),
                 (abi.PARAM_FRICTION, rng.uniform(0.01, 0.05, (nq, JIT_N))), (abi.PARAM_MU, 0.33 * rng.uniform(0.8, 1.2, (nq, JIT_N)))):
        sim.set_params(f, v)
    sim.set_state(q, qd)
    for _ in range(3):
        sim.step(torch.as_tensor(rng.uniform(-1, 1, (JIT_N, 2))))
        knots.step(None)
    assert int((sim.get_solver_state()[1] != 0).sum()) * 2 >= JIT_N           # contact rows at the window's start
    W = _table(torch, sim, 4, True, seed=6)
    c0 = sim.step_count
    if recorded:
        ret, length, outs, (act, _), kobs = sim.rollout_schedule(JIT_K, W, knots=knots, first_knot=1, want_knot_obs=True, **WANT)
        torch.cuda.synchronize()
        launches = int(sim.violation_mirror()[1]) - c0 + 1
    else:
        loop = _composed(torch, sim, knots, W, first_knot=1, steps=JIT_K)
        outs = tuple(torch.cat([r[0][2][i] for r in loop]) for i in range(5))
        act, kobs = torch.cat([r[0][3][0] for r in loop]), torch.stack([r[1] for r in loop])
        launches = 0
    assert bool((outs[2] != 0).any())                                          # TimeLimit 5: auto-resets inside the window
    flat = [t.cpu() for t in outs + (act, kobs) + _whole(sim) + _whole(knots)]
    sim.close(); knots.close()
    if path:
        torch.save((launches, flat), path)
    return launches, flat


def test_jit_objects_record_fused_and_in_the_launch_loop(HipSim, torch_mod, tmp_path, monkeypatch):
    torch = torch_mod
    from conftest import KERNEL_CACHE
    from gym_os2r_amd import jit
    if jit.hipcc_path() is None:
        pytest.skip("no hipcc on this machine")
    monkeypatch.setenv("OS2R_JIT", "1")
    monkeypatch.setenv("OS2R_KERNEL_CACHE", KERNEL_CACHE)
    monkeypatch.delenv("OS2R_JIT_FUSED", raising=False)
    want = _jit_run(torch, HipSim, recorded=False)[1]
    launches, got = _jit_run(torch, HipSim, recorded=True)
    assert launches == 1                                       # the policy object announces the sink: one launch
    assert len(got) == len(want)
    for i, (x, z) in enumerate(zip(got, want)):
        assert torch.equal(x, z), i
    # a fresh process without the fused objects: the launch loop records the same
    path = str(tmp_path / "loop.pt")
    env = dict(os.environ, OS2R_JIT="1", OS2R_JIT_FUSED="0", OS2R_KERNEL_CACHE=KERNEL_CACHE,
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    code = ("import torch; from gym_os2r_amd.sim import HipSim; import test_gpu_rollout_knots as t; "
            f"t._jit_run(torch, HipSim, True, {path!r})")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    launches, child = torch.load(path)
    assert launches == JIT_K                                   # a step launch per env-step
    for i, (x, z) in enumerate(zip(child, want)):
        assert torch.equal(x, z), i


# ---------------------------------------------------------------------------------------
# 8. the example: both ways of getting the knots print the same costs
# ---------------------------------------------------------------------------------------
def test_ilqr_example_prints_the_same_costs_either_way():
    import re
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    costs = {}
    for how in ("recorded", "loop"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ilqr_balancing.py"), "--envs", "8", "--steps", "20", "--iters", "3",
                            "--knots", how], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        costs[how] = re.findall(r"^iter +\d+ cost (\S+)", r.stdout, re.M)
        assert len(costs[how]) == 4, r.stdout
    assert costs["recorded"] == costs["loop"], costs
