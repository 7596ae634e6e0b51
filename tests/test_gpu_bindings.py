"""The two bindings are one library: the same script through HipSim(binding="ctypes") and HipSim(binding="pybind11") returns the
same tensors and numbers, bit for bit.  Nothing is asserted about the values themselves (the oracle tests do that): what is
tested is that every entry point receives the same arguments through the ctypes table and through the adapter made from it."""
import pytest

from gym_os2r_amd import abi

pytestmark = pytest.mark.gpu
N = 65        # one full wave and a tail wave of one lane


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _maker(mode, dtype, contact):
    from helpers import make_config
    from gym_os2r_amd.sim import HipSim

    def make(binding):
        cfg, _, _ = make_config(mode, "StraightV1" if mode == "simple" else "BalancingV2", True, num_envs=N, seed=11, dtype=dtype,
                                contact=contact, reset_mode=abi.RESET_RANDOM, randomize_params=True, max_episode_steps=3)
        sim = HipSim(cfg, binding=binding)
        assert sim.binding == binding and type(sim._lib).__name__ == ("_PybindLib" if binding == "pybind11" else "CDLL")
        return sim
    return make


def _script(torch, s, fresh):
    """Every HipSim call once, on inputs drawn from a fixed seed; -> everything the calls returned.  `fresh` makes a handle of
    the other binding."""
    D, nq = s.D, s.nq
    gen = torch.Generator().manual_seed(5)

    def rnd(*shape):
        return (torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1).to(s.dtype).to(s.device)

    out = []
    mask = (torch.arange(N) % 3 == 0).to(torch.uint8).to(s.device)
    out.append(s.reset(mask))
    out.append(s.step(rnd(N, 2), want_mask=True))
    reasons = s.done_reasons(True)
    out.append(s.step(2 * rnd(N, 2)))                       # (some of these actions are clamped: violations to count)
    out.append(reasons.clone())
    assert s.done_reasons(False) is None
    out.append(s.rollout(2, want_terminal=True, want_reasons=True))
    for w in (0.1 * rnd(2, D + 1), 0.1 * rnd(N, 2, D + 1)):
        out.append(s.rollout_policy(2, w, want_outputs=True))
    out.append(s.rollout_policy(2, 0.1 * rnd(2, D + 1), sigma=0.1, want_actions=True, want_noise=True))
    out.append(s.rollout_schedule(2, 0.1 * rnd(2, 2, D + 1), sigma=0.1, salt=3, want_outputs=True, want_actions=True, want_noise=True))
    q, qd = s.get_state()
    lam, flags = s.get_solver_state()
    s.set_state(q, 0.5 * qd)
    s.set_solver_state(lam, flags)
    out += [q, qd, lam, flags, s.get_state(), s.get_solver_state()]
    hist = s.get_action_history(0)
    s.set_action_history(1, hist)
    out += [hist, s.get_action_history(1)]
    damping = s.get_params(abi.PARAM_DAMPING)
    s.set_params(abi.PARAM_DAMPING, 1.5 * damping)
    out += [damping, s.get_params(abi.PARAM_DAMPING)]
    steps, episode, pose = s.episode_info()
    s.set_episode_info(steps + 1, episode, pose)
    out += [steps, episode, pose, s.episode_info()]
    count = s.step_count
    s.step_count = count + 2 ** 33
    out += [count, s.step_count]
    other = fresh()
    other.restore(s.checkpoint())
    a = rnd(N, 2)
    out += [other.step(a), s.step(a), other.step_count]
    index = torch.arange(N - 1, -1, -1, dtype=torch.int32, device=s.device)
    out.append(s.copy_envs_from(other, index, want_obs=True))
    lin = s.linearize(a)
    out.append(lin)
    eye = torch.eye(2 * nq, dtype=torch.float64)
    out.append(s.lqr_gains(lin[2], lin[3], eye, 0.1 * torch.eye(2, dtype=torch.float64), knots=1, sweeps=2))
    seen = torch.zeros(1, dtype=torch.int32, device=s.device)
    s.action_violations_into(seen)
    torch.cuda.synchronize()
    out += [seen, torch.from_numpy(s.violation_mirror().astype("int64"))]
    assert s.bench_steps(2) > 0.0                           # (a time: the one number that is not compared)
    s.bench_enqueue(2)
    type(s).bench_enqueue_shards([s], [torch.cuda.current_stream(s.device)], 2)
    torch.cuda.synchronize()
    out += [s.step_count, s.get_state(), torch.from_numpy(s.violation_mirror().astype("int64"))]
    other.close()
    s.close()
    return out


def _same(torch, a, b, where="out"):
    if isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(torch, x, y, f"{where}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b), where
    else:
        assert type(a) is type(b) and a == b, (where, a, b)


@pytest.mark.parametrize("mode,dtype,contact", [("free_hip", abi.F64, True), ("free_hip", abi.F32, True)])
def test_the_two_bindings_are_one_library(torch_mod, mode, dtype, contact):
    make = _maker(mode, dtype, contact)
    a = _script(torch_mod, make("ctypes"), lambda: make("pybind11"))
    b = _script(torch_mod, make("pybind11"), lambda: make("ctypes"))
    _same(torch_mod, a, b)


@pytest.mark.parametrize("mode,contact", [("free_hip", True), ("simple", False)])
def test_work_counters_through_both_bindings(torch_mod, mode, contact):
    """count_work(True), a step, work_counters().  The two-dof robot without ground contact has no counting variant: the
    launcher's other branch, whose refusal must read the same through both bindings; with contact the counters come back."""
    from gym_os2r_amd.sim import Os2rError
    make = _maker(mode, abi.F64, contact)
    seen = []
    for binding in ("ctypes", "pybind11"):
        s = make(binding)
        s.count_work(True)
        if contact:
            s.step(None)
            seen.append(s.work_counters())
            assert set(seen[-1]) == set(s.WORK_COUNTERS) and seen[-1]["wave_iterations"] > 0
        else:
            with pytest.raises(Os2rError, match="no counting variant") as refusal:
                s.step(None)
            seen.append(str(refusal.value))
        s.count_work(False)
        seen.append(s.step(None))
        s.close()
    _same(torch_mod, seen[:2], seen[2:])


def test_policy_entry_points_refuse_in_their_order_with_their_texts(torch_mod):
    """The three os2r_rollout_policy* entry points share one check (csrc/os2r_capi.hip: check_policy_call): which cause is
    named when several apply, and the text of each, through both bindings.  Nothing is launched: every call is refused."""
    make = _maker("free_hip", abi.F64, True)
    for binding in ("ctypes", "pybind11"):
        s = make(binding)
        lib, h = s._lib, s._h
        w = torch_mod.zeros(2, 2, s.D + 1, dtype=s.dtype, device=s.device)
        p, no = w.data_ptr(), None
        bad, sg_bit = 64, abi.POLICY_SIGMA_PER_ENV
        out = (no,) * 7                                    # return, length, obs, reward, done, term_obs, reason
        cases = [
            ("os2r_rollout_policy", (0, no, bad), "nsteps must be >= 1"),
            ("os2r_rollout_policy", (1, no, bad), "null weights"),
            ("os2r_rollout_policy", (1, p, sg_bit), "unknown flag bits"),
            ("os2r_rollout_policy_noisy", (0, no, bad, no, 0), "nsteps must be >= 1"),
            ("os2r_rollout_policy_noisy", (1, no, bad, no, 0), "null weights"),
            ("os2r_rollout_policy_noisy", (1, p, bad, no, 0), "null sigma"),
            ("os2r_rollout_policy_noisy", (1, p, abi.POLICY_CLOCK_EPISODE, p, 0), "unknown flag bits"),
            ("os2r_rollout_policy_scheduled", (0, no, 0, -1, bad, no, 1), "nsteps must be >= 1"),
            ("os2r_rollout_policy_scheduled", (1, no, 0, -1, bad, no, 1), "period must be >= 1"),
            ("os2r_rollout_policy_scheduled", (1, no, 1, -1, bad, no, 1), "first_slot must be >= 0"),
            ("os2r_rollout_policy_scheduled", (1, no, 1, 0, bad, no, 1), "null weights"),
            ("os2r_rollout_policy_scheduled", (1, p, 1, 0, bad, no, 1), "unknown flag bits"),
            ("os2r_rollout_policy_scheduled", (1, p, 1, 0, 0, no, 1), "noise_dev needs sigma_dev"),
            ("os2r_rollout_policy_scheduled", (1, p, 1, 0, 0, no, 1, False), "a non-zero salt needs sigma_dev"),
        ]
        for name, head, why in cases:
            noise = no if head[-1] is False else p
            head = tuple(x for x in head if x is not False)
            tail = out + (() if name == "os2r_rollout_policy" else (no, noise)) + (no,)      # ..., action, noise, stream
            assert getattr(lib, name)(h, *head, *tail) == abi.ERR_INVALID, (name, head)
            assert lib.os2r_last_error(h) == f"{name}: {why}".encode(), (name, head)
        count = s.step_count
        s.close()
        assert count == 0
