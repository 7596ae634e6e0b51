"""os2rg_policy_gradient on the device (libos2r_pg.so, include/os2r_pg.h): every output bit for bit against the numpy restatement
of tests/test_pg_host.py on crafted inputs -- both weightings, three discounts, the baseline, obs0 given and null, shared and
per-lane sigma, tanh --, the outputs that were left out untouched, and the call against its real consumers: a noisy
rollout_policy on a real handle, the same window recorded into a knots handle, one policy per environment feeding the next
rollout, and policy_gradient_into on the caller's tensors."""
import ctypes

import numpy as np
import pytest

from gym_os2r_amd import abi
from helpers import make_config
from test_pg_host import MARGIN, MEASURED, SHAPES, at_most_a_quarter_invalid, crafted_pg, restate_pg

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
FLOATS = ("grad", "lane_grad", "lsig_grad", "lane_lsig", "rtg")
OUTPUTS = ("grad", "lane_grad", "lsig_grad", "lane_lsig", "steps", "clipped", "valid", "rtg", "lane_count")      # the header's order
# weight, gamma, baseline, obs0, per-lane sigma, tanh, outputs left out
CONFIGS = [("adv", 1.0, False, True, False, False, ("rtg",)),
           ("adv", 1.0, False, False, True, True, ("rtg", "lsig_grad", "lane_lsig", "steps", "clipped", "valid")),
           ("adv", 1.0, False, True, True, False, ("rtg", "clipped")),
           ("rtg", 1.0, False, True, False, False, ()),
           ("rtg", 0.0, True, False, True, False, ("rtg", "steps")),
           ("rtg", 0.97, True, True, True, True, ("valid",)),
           ("rtg", 0.97, False, False, False, True, ("lsig_grad", "lane_lsig")),
           ("rtg", 1.0, True, True, False, False, ("rtg", "lsig_grad", "lane_lsig", "steps", "clipped", "valid"))]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _np(dtype):
    return np.float64 if dtype == abi.F64 else np.float32


@pytest.fixture(scope="module")
def crafted():
    """The crafted inputs of every shape and dtype, made once and left unchanged."""
    return {(shape, dtype): crafted_pg(*shape, _np(dtype)) for shape in SHAPES for dtype in (abi.F64, abi.F32)}


class Call:
    """One os2rg_policy_gradient call through ctypes: the inputs of `crafted_pg` on the device, every output between guard bands of
    PAD sentinel elements.  The constructor uploads, run() launches and synchronises."""

    def __init__(self, torch, c, shape, dtype):
        from gym_os2r_amd import pg
        self.torch, self.lib, self.dtype, self.shape, self.c = torch, pg.load(), dtype, shape, c
        K, P, S, D = shape
        N = S * P
        self.dev = torch.device("cuda:0")
        self.t = {k: torch.as_tensor(v).to(self.dev) for k, v in c.items()}
        real = self.t["obs"].dtype
        self.shapes = dict(grad=(2, D + 1, P), lane_grad=(2, D + 1, N), lsig_grad=(2, P), lane_lsig=(2, N), steps=(P,), clipped=(2, P),
                           valid=(P,), rtg=(K, N), lane_count=(4, N))
        self.sizes = {k: int(np.prod(v)) for k, v in self.shapes.items()}
        self.bufs = {name: torch.full((PAD + size + PAD,), MARK if name in FLOATS else IMARK, dtype=real if name in FLOATS else torch.int32,
                                      device=self.dev) for name, size in self.sizes.items()}

    def run(self, weight, gamma, baseline, obs0, per_lane, tanh, leave_out=(), device=0):
        from gym_os2r_amd import control, pg
        K, P, S, D = self.shape
        lay = control.layout(self.dtype, 3, device, [-1] * D)
        t = self.t
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        rew = weight == "rtg"
        if not rew:
            leave_out = tuple(leave_out) + (("rtg",) if "rtg" not in leave_out else ())
        outs = [None if name in leave_out else p(self.bufs[name][PAD:]) for name in OUTPUTS]
        self.rc = self.lib.os2rg_policy_gradient(
            ctypes.byref(lay), K, P, S, (pg.TANH if tanh else 0) | (pg.SIGMA_PER_LANE if per_lane else 0), p(t["obs"]),
            p(t["obs0"]) if obs0 else None, p(t["noise"]), None if tanh else p(t["action"]), p(t["lane_sigma"] if per_lane else t["sigma"]),
            p(t["length"]), None if rew else p(t["adv"]), p(t["reward"]) if rew else None, p(t["done"]) if rew else None, gamma,
            p(t["baseline"]) if rew and baseline else None, *outs, None)
        self.error = self.lib.os2rg_last_error()
        self.torch.cuda.synchronize()
        self.left_out = tuple(leave_out)
        c = self.c
        self.want = dict(P=P, dtype=_np(self.dtype), obs0=c["obs0"] if obs0 else None, action=None if tanh else c["action"], tanh=tanh,
                         length=c["length"], adv=None if rew else c["adv"], reward=c["reward"] if rew else None, done=c["done"] if rew else None,
                         gamma=gamma, baseline=c["baseline"] if rew and baseline else None)
        self.sigma = c["lane_sigma"] if per_lane else c["sigma"]
        return self

    def out(self, name):
        """-> the array the call wrote, after a look at its guard bands (and, if it was left out, at all of it)"""
        host = self.bufs[name].cpu().numpy()
        mark = MARK if name in FLOATS else IMARK
        assert (host[:PAD] == mark).all() and (host[PAD + self.sizes[name]:] == mark).all(), f"{name}: written outside"
        inner = host[PAD:PAD + self.sizes[name]]
        if name in self.left_out:
            assert (inner == mark).all(), f"{name}: written although left out"
            return None
        return inner.reshape(self.shapes[name])

    def check(self, what, crafted_lanes=True):
        """Every output against the restatement, bit for bit (the sign of a zero and the payload of a NaN are not part of the contract).
        `crafted_lanes`: the inputs are crafted_pg's as they are, with their invalid lanes."""
        assert self.rc == abi.OK, (what, self.rc, self.error)
        want = restate_pg(self.c["obs"], self.c["noise"], self.sigma, **self.want)
        if crafted_lanes:                                                              # (on the CPU, before the outputs are read)
            assert at_most_a_quarter_invalid(want, self.shape[1], self.shape[2])
        for name in OUTPUTS:
            got = self.out(name)
            if got is not None:
                assert got.dtype == want[name].dtype and np.array_equal(got, want[name], equal_nan=True), \
                    (what, name, np.argwhere(~((got == want[name]) | (np.isnan(got) & np.isnan(want[name]))))[:4])
        return want


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_bit_for_bit(torch_mod, crafted, shape, dtype):
    """grad, lane_grad, lsig_grad, lane_lsig, steps, clipped, valid, rtg and lane_count equal the restatement in every
    configuration; an output that was left out still holds the sentinel."""
    K, P, S, D = shape
    c = crafted[(shape, dtype)]
    seen = set()
    for config in CONFIGS:
        want = Call(torch_mod, c, shape, dtype).run(*config).check(f"{shape} {dtype} {config}")
        seen.add(want["grad"].tobytes())
        if P > 2:
            assert want["valid"][2] == 0 and (want["grad"][:, :, 2] == 0).all()
        assert np.isfinite(want["grad"]).all() and (S < 6 or not np.isfinite(want["lane_grad"]).all())
    assert len(seen) == len(CONFIGS) or K * S * P == 1                          # the configurations differ in what they compute


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_a_shared_sigma_of_zero_and_nan_leaves_zeros(torch_mod, crafted, dtype):
    shape = SHAPES[1]
    c = dict(crafted[(shape, dtype)])
    c["sigma"] = np.array([0.0, np.nan], _np(dtype))
    want = Call(torch_mod, c, shape, dtype).run("adv", 1.0, False, True, False, False).check("sigma 0 and NaN", crafted_lanes=False)   # (no component opens: no lane is invalid)
    assert (want["grad"] == 0).all() and (want["lane_grad"] == 0).all() and want["valid"].tolist() == [shape[2]] * shape[1]
    assert (want["clipped"] > 0).all()


def test_refusals_on_the_device(torch_mod, crafted):
    shape = SHAPES[1]
    c = crafted[(shape, abi.F64)]
    call = Call(torch_mod, c, shape, abi.F64).run("adv", 1.0, False, True, False, False, device=1000)
    assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(b"os2rg_policy_gradient: "), (call.rc, call.error)
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)                        # a refused call wrote nothing
    call = Call(torch_mod, c, shape, abi.F64).run("rtg", float("nan"), False, True, False, False)
    assert call.rc == abi.ERR_INVALID and call.error == b"os2rg_policy_gradient: gamma must be finite"
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)


# ---------------------------------------------------------------------------------------
# the real consumers
# ---------------------------------------------------------------------------------------
N_REAL, K_REAL = 128, 8


def _handle(num, seed=5):
    from gym_os2r_amd.sim import HipSim
    return HipSim(make_config("free_hip", "BalancingV2", False, num_envs=num, contact=True, seed=seed, auto_reset=True, dtype=abi.F64)[0])


def _cpu(t):
    return t.detach().cpu().numpy().copy()


@pytest.fixture(scope="module")
def window(torch_mod):
    """One noisy window of K_REAL steps on a real handle of N_REAL environments from reset(), and the same window recorded into a
    knots handle by a twin handle: made once, shared, left unchanged."""
    torch = torch_mod
    sim, twin, knots = _handle(N_REAL), _handle(N_REAL), _handle(K_REAL * N_REAL)
    D, dev = sim.D, sim.device
    rng = np.random.default_rng(11)
    theta = torch.as_tensor(rng.normal(0, 0.3, (2, D + 1))).to(dev)
    sigma = torch.as_tensor(np.array([0.3, 0.5])).to(dev)
    kw = dict(sigma=sigma, salt=3, first_episode=True, want_outputs=True, want_actions=True, want_noise=True)
    obs0 = sim.reset()
    ret, length, (O, R, Dn, _, _), (A, E) = sim.rollout_policy(K_REAL, theta, **kw)
    obs0_twin = twin.reset()
    recorded = twin.rollout_policy(K_REAL, theta, knots=knots, want_knot_obs=True, **kw)
    torch.cuda.synchronize()
    out = dict(sim=sim, theta=theta, sigma=sigma, obs0=obs0, ret=ret, length=length, O=O, R=R, Dn=Dn, A=A, E=E, obs0_twin=obs0_twin,
               recorded=recorded, adv=(ret - ret.mean()) / ret.std().clamp_min(1e-8))
    yield out
    for h in (sim, twin, knots):
        h.close()


def test_real_consumer_the_gradient_of_a_noisy_rollout(torch_mod, window):
    """policy_gradient on what rollout_policy returned equals the restatement bit for bit, and the torch statement of
    examples/reinforce_balancing.py within the margin of tests/test_pg_host.py."""
    torch, w = torch_mod, window
    sim, sigma, O, A, E, Dn, length, adv, obs0 = (w[k] for k in ("sim", "sigma", "O", "A", "E", "Dn", "length", "adv", "obs0"))
    grad, steps, clipped, valid, lsig, lane, rtg = sim.policy_gradient(O, E, sigma, obs0=obs0, actions=A, length=length, adv=adv,
                                                                     want_log_sigma=True, want_lane=True)
    torch.cuda.synchronize()
    assert tuple(grad.shape) == (1, 2, sim.D + 1) and tuple(lane.shape) == (N_REAL, 2, sim.D + 1) and rtg is None
    assert tuple(clipped.shape) == (1, 2) and tuple(lsig.shape) == (1, 2) and grad.permute(1, 2, 0).is_contiguous()
    want = restate_pg(_cpu(O), _cpu(E), _cpu(sigma), P=1, dtype=np.float64, obs0=_cpu(obs0), action=_cpu(A), length=_cpu(length), adv=_cpu(adv))
    for name, got in (("grad", grad.permute(1, 2, 0)), ("steps", steps), ("clipped", clipped.t()), ("valid", valid), ("lsig_grad", lsig.t()),
                      ("lane_grad", lane.permute(1, 2, 0))):
        assert np.array_equal(_cpu(got), want[name]), name
    assert int(valid) == N_REAL and int(steps) == int(length.sum()) and (want["grad"] != 0).all()
    # the five statements of the example
    dt = sim.dtype
    prev = torch.cat([obs0.unsqueeze(0), O[:-1]])
    ended = (Dn != 0).to(torch.int32)
    alive = ((torch.cumsum(ended, 0) - ended) == 0).to(dt)
    coef = (A.abs() < 1.0).to(dt) * E / sigma * (alive * adv.unsqueeze(0)).unsqueeze(-1)
    torch_grad = torch.cat([torch.einsum("knj,knd->jd", coef, prev), coef.sum((0, 1)).unsqueeze(1)], 1)
    far = float((grad[0] - torch_grad).abs().max() / torch_grad.abs().max())
    print(f"policy_gradient against the torch statement: {far:.3e}")
    assert far <= MARGIN * MEASURED[np.float64]["grad"]
    assert int(clipped.sum()) == int(((A.abs() >= 1.0) & (alive != 0).unsqueeze(-1)).sum())
    # the reward-to-go on the same window, against the restatement
    base = torch.as_tensor(np.linspace(0.0, 1.0, K_REAL)).to(sim.device).reshape(K_REAL, 1)
    out = sim.policy_gradient(O, E, sigma, obs0=obs0, actions=A, length=length, rewards=w["R"], done=Dn, gamma=0.97, baseline=base, want_rtg=True)
    torch.cuda.synchronize()
    want = restate_pg(_cpu(O), _cpu(E), _cpu(sigma), P=1, dtype=np.float64, obs0=_cpu(obs0), action=_cpu(A), length=_cpu(length),
                      reward=_cpu(w["R"]), done=_cpu(Dn), gamma=0.97, baseline=_cpu(base))
    assert np.array_equal(_cpu(out[0].permute(1, 2, 0)), want["grad"]) and np.array_equal(_cpu(out[6]), want["rtg"]) and out[4] is None


def test_recorded_consumer_the_knot_observations_are_what_the_policy_saw(torch_mod, window):
    """The same window recorded into a knots handle of K x N lanes with want_knot_obs: obs0=None with obs=knot_obs gives the bits
    of obs0=the reset's observation with obs=the rollout's."""
    torch, w = torch_mod, window
    sim = w["sim"]
    ret, length, (O, _, _, _, _), (A, E), knot_obs = w["recorded"]
    assert torch.equal(O, w["O"]) and torch.equal(E, w["E"]) and torch.equal(A, w["A"]) and torch.equal(w["obs0_twin"], w["obs0"])
    assert torch.equal(knot_obs[0], w["obs0"]) and torch.equal(knot_obs[1:], O[:-1])
    kw = dict(actions=A, length=length, adv=w["adv"], want_log_sigma=True, want_lane=True)
    first = sim.policy_gradient(w["O"], E, w["sigma"], obs0=w["obs0"], **kw)
    second = sim.policy_gradient(knot_obs, E, w["sigma"], obs0=None, **kw)
    torch.cuda.synchronize()
    for a, b in zip(first[:6], second[:6]):
        assert np.array_equal(_cpu(a).view(np.uint8), _cpu(b).view(np.uint8))
    assert (_cpu(first[0]) != 0).all()


def test_per_environment_consumer_the_gradient_is_the_weight_layout(torch_mod):
    """P = N: weights_per_env + step * grad is what the next rollout_policy takes as it stands, with no permute and no copy."""
    torch = torch_mod
    sim = _handle(N_REAL, seed=7)
    D, dev = sim.D, sim.device
    rng = np.random.default_rng(2)
    weights = torch.as_tensor(rng.normal(0, 0.3, (2, D + 1, N_REAL))).to(dev).permute(2, 0, 1)        # [N, 2, D+1] over the kernel's layout
    sigma = torch.as_tensor(rng.uniform(0.2, 0.5, (N_REAL, 2))).to(dev)
    obs0 = sim.reset()
    ret, length, (O, R, Dn, _, _), (A, E) = sim.rollout_policy(K_REAL, weights, sigma=sigma, first_episode=True, want_outputs=True,
                                                               want_actions=True, want_noise=True)
    grad, steps, clipped, valid, _, lane, _ = sim.policy_gradient(O, E, sigma, policies=N_REAL, obs0=obs0, actions=A, length=length,
                                                                  rewards=R, done=Dn, gamma=0.97, want_lane=True)
    torch.cuda.synchronize()
    want = restate_pg(_cpu(O), _cpu(E), _cpu(sigma).T, P=N_REAL, dtype=np.float64, obs0=_cpu(obs0), action=_cpu(A), length=_cpu(length),
                      reward=_cpu(R), done=_cpu(Dn), gamma=0.97)
    assert np.array_equal(_cpu(grad.permute(1, 2, 0)), want["grad"]) and np.array_equal(_cpu(steps), _cpu(length))
    assert np.array_equal(_cpu(grad), _cpu(lane)) and (_cpu(valid) == 1).all()                         # one sample: the lane's sums
    new = weights + 0.01 * grad
    assert tuple(new.shape) == (N_REAL, 2, D + 1)
    taken, per_env, _ = sim._policy_weights("rollout_policy", new, table=False)
    assert taken.data_ptr() == new.data_ptr() and per_env == abi.POLICY_PER_ENV                       # no copy on the way into the rollout
    sim.reset()
    ret2, _, _ = sim.rollout_policy(K_REAL, new, first_episode=True)
    torch.cuda.synchronize()
    assert np.isfinite(_cpu(ret2)).all()
    sim.close()


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_policy_gradient_into_gives_the_bits_of_the_allocating_call(torch_mod, crafted, dtype):
    """On the crafted inputs of (7, 3, 65, 10), through a handle of the same observation width: the caller's tensors hold what the
    allocating call returned."""
    torch = torch_mod
    from gym_os2r_amd.sim import HipSim
    shape = K, P, S, D = SHAPES[1]
    N = S * P
    sim = HipSim(make_config("free_hip", "BalancingV2", False, num_envs=4, contact=True, seed=1, dtype=dtype)[0])
    assert sim.D == D
    c = {k: torch.as_tensor(v).to(sim.device) for k, v in crafted[(shape, dtype)].items()}
    kw = dict(policies=P, obs0=c["obs0"], actions=c["action"], length=c["length"], rewards=c["reward"], done=c["done"], gamma=0.97,
              baseline=c["baseline"])
    whole = sim.policy_gradient(c["obs"], c["noise"], c["lane_sigma"].t(), want_log_sigma=True, want_lane=True, want_rtg=True, **kw)
    i32 = torch.int32
    z = lambda *s, dtype=sim.dtype: torch.full(s, -3, dtype=dtype, device=sim.device)
    grad, lane, count, lsig, lane_lsig = z(2, D + 1, P), z(2, D + 1, N), z(4, N, dtype=i32), z(2, P), z(2, N)
    steps, clipped, valid, rtg = z(P, dtype=i32), z(2, P, dtype=i32), z(P, dtype=i32), z(K, N)
    sim.policy_gradient_into(c["obs"], c["noise"], c["lane_sigma"], grad, lane, count, lsig_grad=lsig, lane_lsig=lane_lsig, steps=steps,
                             clipped=clipped, valid=valid, rtg=rtg, **kw)
    torch.cuda.synchronize()
    for got, ret in ((grad.permute(2, 0, 1), whole[0]), (steps, whole[1]), (clipped.t(), whole[2]), (valid, whole[3]), (lsig.t(), whole[4]),
                     (lane.permute(2, 0, 1), whole[5]), (rtg, whole[6])):
        assert got.shape == ret.shape and np.array_equal(_cpu(got).view(np.uint8), _cpu(ret).view(np.uint8))
    want = restate_pg(_cpu(c["obs"]), _cpu(c["noise"]), _cpu(c["lane_sigma"]), P=P, dtype=_np(dtype), obs0=_cpu(c["obs0"]), action=_cpu(c["action"]),
                      length=_cpu(c["length"]), reward=_cpu(c["reward"]), done=_cpu(c["done"]), gamma=0.97, baseline=_cpu(c["baseline"]))
    assert np.array_equal(_cpu(grad), want["grad"]) and np.array_equal(_cpu(count), want["lane_count"]) and (_cpu(valid) < S).all()
    sim.close()
