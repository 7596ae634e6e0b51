"""A custom robot's own code objects behind rollout(), rollout_policy(), rollout_schedule() and linearize() on the MI355X
(gym_os2r_amd/jit.py, csrc/os2r_jit_fused_unit.hip).  Every comparison is torch.equal.  The yardstick of a fused call is the
launch loop on the same arithmetic: handles created under OS2R_JIT_FUSED=0 before any fused object of the robot is registered
(a handle keeps what was registered when it was created).  The yardstick of linearize is the fork / perturb / step path.

Robot, task and schedule: tests/test_jit_fused_host.py (N = 200), helpers.lying_states (seed 11), three warm-up env-steps with
random actions, then a window of K = 6; auto-reset, TimeLimit 5.  Two conditions every test checks on its own data: at least
half of the environments carry contact rows at the window's start, and a done flag is raised inside the window."""
import ctypes as C

import numpy as np
import pytest

from conftest import KERNEL_CACHE
from helpers import lying_states, make_config
from test_gpu_linearize import _actions, _assert_equal, _composed, _default_eps, _violations
from test_jit_fused_host import config, robot
from gym_os2r_amd import _lib, abi, jit

pytestmark = pytest.mark.gpu
K, N = 6, 200
CASES = [(abi.F64, False), (abi.F64, True), (abi.F32, False)]        # (dtype, per-env parameters)
IDS = ["f64", "f64-dr", "f32"]


def _probe(torch, sim):
    """Which path rollout(3) takes: the step counter the last STARTED launch stored in the mirror, minus the window's first
    (0: one launch, 2: a launch per env-step)."""
    c = sim.step_count
    sim.rollout(3)
    torch.cuda.synchronize()
    assert sim.step_count == c + 3
    return int(sim.violation_mirror()[1]) - (c & 0xFFFFFFFF)


def _flat(ck):
    out = {k: v for k, v in ck.items() if k != "params"}
    out.update({f"param{f}": v for f, v in ck["params"].items()})
    return out


def _same(torch, a, b, what):
    """torch.equal over two nested results (tuples, None, tensors, checkpoints)."""
    if isinstance(a, dict):
        a, b = _flat(a), _flat(b)
        assert a.keys() == b.keys(), what
        for k in a:
            _same(torch, a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(torch, x, y, f"{what}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (what, int((a != b).sum()))
    else:
        assert a == b, (what, a, b)


class World:
    """The handles of the module.  loop[case]: launch loop; start[case]: holds the window's start and is never advanced."""

    def __init__(self, torch, HipSim):
        self.torch, self.HipSim = torch, HipSim
        self.model = robot()
        self.loop, self.start, self.fused = {}, {}, {}

    def make(self, dtype, n=N, **kw):
        kw = {**dict(auto_reset=True, max_episode_steps=5, seed=5), **kw}
        sim = self.HipSim(config(dtype, n, **kw))
        assert sim.specialised
        return sim

    def prepare_start(self, case):
        """lying states, per-env parameters where the case has them, three warm-up env-steps."""
        torch = self.torch
        dtype, dr = case
        sim = self.make(dtype)
        rng = np.random.default_rng(11)
        q, qd = lying_states(self.model, N, rng)
        if dr:
            nq = sim.nq
            for f, v in ((abi.PARAM_MASS_SCALE, rng.uniform(0.8, 1.2, (nq, N))), (abi.PARAM_DAMPING, rng.uniform(0.008, 0.012, (nq, N))),
                         (abi.PARAM_FRICTION, rng.uniform(0.01, 0.05, (nq, N))), (abi.PARAM_MU, 0.33 * rng.uniform(0.8, 1.2, (nq, N)))):
                sim.set_params(f, v)
        sim.set_state(q, qd)
        for _ in range(3):
            sim.step(torch.as_tensor(rng.uniform(-1, 1, (N, 2))))
        torch.cuda.synchronize()
        # contact rows at the window's start.  (The fp32 kernels carry no solver state -- their solver_flags stay 0 by design --
        # so the fp32 case is vouched for by its fp64 twin: same states, same warm-up actions, prepared before it.)
        witness = sim if dtype == abi.F64 else self.start[abi.F64, dr]
        touching = witness.get_solver_state()[1] != 0
        assert int(touching.sum()) * 2 >= N, int(touching.sum())
        assert sim.step_count == 3
        return sim

    def load(self, sim, case):
        """sim becomes the window's start of `case` (state, solver state, histories, episode clocks, parameters, counter)."""
        src = self.start[case]
        sim.copy_envs_from(src)
        sim.step_count = src.step_count
        return sim

    def fused_handle(self, case, which=0):
        """Handles created after the fused objects were registered, two per case (the second replays)."""
        if (case, which) not in self.fused:
            self.fused[case, which] = self.make(case[0])
        return self.load(self.fused[case, which], case)

    def close(self):
        for group in (self.loop, self.start, self.fused):
            for sim in group.values():
                sim.close()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def world(torch_mod):
    from gym_os2r_amd.sim import HipSim
    if jit.hipcc_path() is None:
        pytest.skip("no hipcc on this machine")
    torch = torch_mod
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OS2R_JIT", "1")
        mp.setenv("OS2R_KERNEL_CACHE", KERNEL_CACHE)
        mp.delenv("OS2R_JIT_FUSED", raising=False)
        # into the cache first, all kinds side by side (a cache that arrives empty costs one build of each dtype here, not one
        # per handle below); nothing is registered yet
        for dtype in (abi.F64, abi.F32):
            cfg = config(dtype)
            assert tuple(jit.build_all(cfg.model, dtype, True, jit.task_layout(cfg.task))) == jit.KINDS
        mp.setenv("OS2R_JIT_FUSED", "0")
        w = World(torch, HipSim)
        for case in CASES:                                   # all loop handles first: only the step objects are registered yet
            w.loop[case] = w.make(case[0])
            w.start[case] = w.prepare_start(case)
            assert _probe(torch, w.loop[case]) == 2, case
        mp.delenv("OS2R_JIT_FUSED")
        for case in CASES:
            assert _probe(torch, w.fused_handle(case)) == 0, case
            assert _probe(torch, w.loop[case]) == 2, case    # a later registration does not change an existing handle
        yield w
        w.close()


def _weights(torch, sim, *lead, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*lead, 2, sim.D + 1, generator=g, dtype=torch.float64) * 0.6).to(sim.dtype).to(sim.device)


# ---------------------------------------------------------------------------------------
# 4. which path a call takes
# ---------------------------------------------------------------------------------------
def test_fused_objects_put_the_three_rollouts_on_one_launch(world, torch_mod):
    torch = torch_mod
    case = CASES[0]
    calls = (lambda s: s.rollout(3), lambda s: s.rollout_policy(3, _weights(torch, s)),
             lambda s: s.rollout_schedule(3, _weights(torch, s, 4)))
    for sim, last in ((world.fused_handle(case), 0), (world.load(world.loop[case], case), 2)):
        for call in calls:
            c = sim.step_count
            call(sim)
            torch.cuda.synchronize()
            assert sim.step_count == c + 3
            assert int(sim.violation_mirror()[1]) == c + last, (last, c)
    # the default solver only: sweep counts off the default keep the launch loop
    other = world.make(case[0], pgs_iters=abi.DEFAULT_PGS_ITERS + 3)
    assert _probe(torch, other) == 2
    c = other.step_count
    other.rollout_policy(3, _weights(torch, other))
    torch.cuda.synchronize()
    assert int(other.violation_mirror()[1]) == c + 2
    other.close()
    # and a code object has no counting variant, fused or not
    from gym_os2r_amd.sim import Os2rError
    sim = world.fused_handle(case)
    sim.count_work(True)
    for call in calls:
        with pytest.raises(Os2rError, match="no counting variant"):
            call(sim)
    sim.count_work(False)
    assert _probe(torch, sim) == 0


# ---------------------------------------------------------------------------------------
# 5. rollout(K) = K x step()
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("drawn", [False, True], ids=["actions", "drawn"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_rollout_equals_k_steps(world, torch_mod, case, drawn):
    torch = torch_mod
    a, b = world.fused_handle(case), world.fused_handle(case, 1)
    g = torch.Generator().manual_seed(2)
    actions = None if drawn else (torch.rand(K, N, 2, generator=g, dtype=torch.float64) * 2 - 1).to(a.dtype).to(a.device)
    obs, rew, done, term, why = a.rollout(K, actions, want_terminal=True, want_reasons=True)
    torch.cuda.synchronize()
    assert int(a.violation_mirror()[1]) == 3                 # one launch
    b.done_reasons(True)
    for k in range(K):
        o, r, d, t = b.step(None if drawn else actions[k])
        _same(torch, (obs[k], rew[k], done[k], why[k]), (o, r, d, b.reasons), f"step {k}")
        # (the terminal observation is defined where the episode ended)
        ended = d != 0
        assert torch.equal(term[k][ended], t[ended]), f"terminal obs, step {k}"
    b.done_reasons(False)
    assert bool((done != 0).any())                           # TimeLimit 5: an auto-reset inside the window
    _same(torch, a.checkpoint(), b.checkpoint(), "checkpoint")


# ---------------------------------------------------------------------------------------
# 6. policy rollouts: fused = launch loop, and rollout(K, actions) replays the window
# ---------------------------------------------------------------------------------------
def _policy_calls(torch):
    out = (lambda s: s.rollout_policy(K, _weights(torch, s), want_outputs=True, want_terminal=True, want_reasons=True),
           lambda s: s.rollout_policy(K, _weights(torch, s, s.N), tanh=True, first_episode=True, want_outputs=True),
           lambda s: s.rollout_policy(K, _weights(torch, s), sigma=0.3, salt=7, want_outputs=True, want_actions=True, want_noise=True),
           lambda s: s.rollout_schedule(K, _weights(torch, s, 4), want_outputs=True, want_actions=True),
           lambda s: s.rollout_schedule(K, _weights(torch, s, 4), clock="episode", wrap=True, first_slot=2, first_episode=True,
                                        sigma=torch.tensor([0.2, 0.4], dtype=s.dtype, device=s.device), salt=3, want_outputs=True,
                                        want_reasons=True, want_actions=True, want_noise=True),
           lambda s: s.rollout_schedule(K, _weights(torch, s, s.N, 4), wrap=True, tanh=True, want_outputs=True, want_terminal=True,
                                        want_actions=True))
    return dict(zip(POLICY_CALLS, out))


POLICY_CALLS = ("shared-clip", "per-env-tanh-first", "noisy", "schedule-hold", "schedule-episode-wrap-noisy", "schedule-per-env-wrap")


@pytest.mark.parametrize("case,call", [(c, p) for c in CASES[:2] for p in POLICY_CALLS] + [(CASES[2], "noisy")],
                         ids=[f"{i}-{p}" for i in IDS[:2] for p in POLICY_CALLS] + ["f32-noisy"])
def test_fused_policy_rollouts_equal_the_launch_loop(world, torch_mod, case, call):
    torch = torch_mod
    run = _policy_calls(torch)[call]
    fused, loop = world.fused_handle(case), world.load(world.loop[case], case)
    got, want = run(fused), run(loop)
    torch.cuda.synchronize()
    assert int(fused.violation_mirror()[1]) == 3 and int(loop.violation_mirror()[1]) == 3 + K - 1
    _same(torch, got, want, call)
    _same(torch, fused.checkpoint(), loop.checkpoint(), "checkpoint")
    ret, length, outs = got[:3]
    assert bool((outs[2] != 0).any())                        # a done flag inside the window
    assert 1 <= int(length.min()) and int(length.max()) <= K and bool(torch.isfinite(ret).all())
    if len(got) == 4 and got[3][0] is not None:
        # the reported actions replay the window on the open-loop rollout, bit for bit
        replay = world.fused_handle(case, 1)
        o, r, d, t, why = replay.rollout(K, got[3][0], want_terminal=outs[3] is not None, want_reasons=outs[4] is not None)
        _same(torch, (o, r, d), outs[:3], "replay")
        if outs[4] is not None:
            _same(torch, why, outs[4], "replay reasons")
        if outs[3] is not None:
            ended = d != 0
            assert torch.equal(t[ended], outs[3][ended])
        _same(torch, replay.checkpoint(), fused.checkpoint(), "replay checkpoint")


# ---------------------------------------------------------------------------------------
# 7. linearize on the robot's own arithmetic
# ---------------------------------------------------------------------------------------
def _check_linearize(torch, world, sim, make):
    eps = (_default_eps(torch, sim.dtype),) * 3
    actions = _actions(torch, sim, eps[2])
    torch.cuda.synchronize()
    before, count, mirror = sim.checkpoint(), sim.step_count, list(sim.violation_mirror())
    next_q, next_qd, A, B = sim.linearize(actions, eps)
    torch.cuda.synchronize()
    _same(torch, sim.checkpoint(), before, "the handle is only read")
    assert sim.step_count == count and list(sim.violation_mirror()) == mirror and _violations(torch, sim) == 0
    want_next, want_A, want_B = _composed(torch, make, sim, actions, eps)
    _assert_equal(torch, torch.cat([next_q, next_qd]), want_next, "next")
    _assert_equal(torch, A, want_A, "A")
    _assert_equal(torch, B, want_B, "B")
    assert bool((A != 0).any()) and bool((B != 0).any())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_linearize_equals_the_fork_and_step_path_on_the_code_object(world, torch_mod, case):
    sim = world.fused_handle(case)
    witness = sim if case[0] == abi.F64 else world.start[abi.F64, case[1]]      # (fp32 carries no solver state: prepare_start)
    assert int((witness.get_solver_state()[1] != 0).sum()) * 2 >= N
    _check_linearize(torch_mod, world, sim, lambda n: world.make(case[0], n, auto_reset=False))


def test_linearize_off_the_default_solver_and_without_contact(world, torch_mod):
    torch = torch_mod
    case = CASES[1]                                          # per-env parameters
    solver = dict(pgs_exact=0, pgs_iters=20)                 # run-time sweep counts: the plain step kernel's instantiation
    sim = world.load(world.make(abi.F64, **solver), case)
    assert int((sim.get_solver_state()[1] != 0).sum()) * 2 >= N
    _check_linearize(torch, world, sim, lambda n: world.make(abi.F64, n, auto_reset=False, **solver))
    sim.close()
    off = world.make(abi.F64, contact=False)
    off.copy_envs_from(world.start[CASES[0]])
    _check_linearize(torch, world, off, lambda n: world.make(abi.F64, n, auto_reset=False, contact=False))
    off.close()


# ---------------------------------------------------------------------------------------
# 8. what must stay as it was
# ---------------------------------------------------------------------------------------
def _short_equalities(torch, make, fused_rollout):
    """rollout = steps, rollout_policy's actions replay, linearize = fork and step: one short run of each on `make`'s handles."""
    a, b = make(N), make(N)
    rng = np.random.default_rng(11)
    q, qd = lying_states(robot(), N, rng)
    for s in (a, b):
        s.set_state(q, qd)
    assert _probe(torch, a) == (0 if fused_rollout else 2)
    for _ in range(3):
        b.step(None)
    _same(torch, a.checkpoint(), b.checkpoint(), "rollout(3) = 3 steps")
    ret, length, outs, (act, _) = a.rollout_policy(3, _weights(torch, a), sigma=0.0, want_outputs=True, want_actions=True)
    torch.cuda.synchronize()
    assert int(a.violation_mirror()[1]) == (3 if fused_rollout else 5)
    o, r, d, _, _ = b.rollout(3, act)
    _same(torch, (o, r, d), outs[:3], "policy replay")
    _same(torch, a.checkpoint(), b.checkpoint(), "policy replay checkpoint")
    eps = (_default_eps(torch, a.dtype),) * 3
    actions = _actions(torch, a, eps[2])
    next_q, next_qd, A, B = a.linearize(actions, eps)
    want_next, want_A, want_B = _composed(torch, make, a, actions, eps)
    _assert_equal(torch, torch.cat([next_q, next_qd]), want_next, "next")
    _assert_equal(torch, A, want_A, "A")
    _assert_equal(torch, B, want_B, "B")
    a.close(); b.close()


def test_generic_and_compiled_in_handles_keep_their_paths(world, torch_mod, monkeypatch):
    torch = torch_mod
    from gym_os2r_amd.sim import HipSim
    monkeypatch.setenv("OS2R_JIT", "0")
    # a robot one bit away from the registered one (os2r_create looks registrations up whatever the package's switch says)
    model = robot()
    model["mass"] = list(model["mass"]); model["mass"][0] = np.nextafter(model["mass"][0], 1.0)

    def generic(n):
        sim = HipSim(make_config("free_hip", "BalancingV1", True, num_envs=n, contact=True, auto_reset=False, seed=5, model_overrides=model)[0])
        assert not sim.specialised
        return sim
    _short_equalities(torch, generic, fused_rollout=False)

    def compiled_in(n):
        sim = HipSim(make_config("free_hip", "BalancingV1", True, num_envs=n, contact=True, auto_reset=False, seed=5)[0])
        assert not sim.specialised
        return sim
    _short_equalities(torch, compiled_in, fused_rollout=True)


def test_registration_by_hand(world, monkeypatch):
    """An object that exports only the linearize kernels is accepted; one that exports nothing known is refused with a message."""
    monkeypatch.setenv("OS2R_KERNEL_CACHE", KERNEL_CACHE)
    lib = _lib.load()
    cfg = config()
    lin = jit.build(cfg.model, abi.F64, True, kind="linearize")       # (the registration takes the caller's word for the robot)
    cfg.model.mass[0] = np.nextafter(cfg.model.mass[0], 0.0)          # a robot no handle of the suite has
    assert lib.os2r_register_model_kernels(C.byref(cfg.model), abi.F64, 0, lin.encode()) == abi.OK
    empty = jit.build(cfg.model, abi.F64, False, kind="policy")       # fused kernels exist with ground contact only: no kernel
    rc = lib.os2r_register_model_kernels(C.byref(cfg.model), abi.F64, 0, empty.encode())
    msg = lib.os2r_last_error(None).decode()
    assert rc == abi.ERR_INVALID and empty in msg and "exports no os2r_jit_" in msg, (rc, msg)
