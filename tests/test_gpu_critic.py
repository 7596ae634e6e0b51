"""os2rv_gae and os2rv_value_fit on the device (libos2r_critic.so, include/os2r_critic.h): every output of both calls bit for bit
against the numpy restatements of tests/test_critic_host.py on crafted inputs -- every optional array present and absent, both
ridges, a rank-deficient batch --, the outputs that were left out untouched, and the calls against their real consumers: a noisy
rollout_policy with auto-reset and a short TimeLimit on a real handle, the policy gradient weighted by the advantages, a
non-default stream, and the *_into forms on the caller's tensors between sentinels."""
import ctypes

import numpy as np
import pytest

from gym_os2r_amd import abi
from helpers import make_config
from test_critic_host import NONE_VALID, SHAPES, broken_lanes, crafted_critic, restate_fit, restate_gae
from test_pg_host import restate_pg

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
GAE_OUTPUTS = ("adv", "ret", "value")                                            # the header's order
FIT_OUTPUTS = ("w", "lane_mom", "mom", "lane_count", "failed", "steps", "valid")
FIT_INTS = ("lane_count", "failed", "steps", "valid")
# term_obs, length, gamma, lambda, outputs left out
GAE_CONFIGS = [(True, True, 0.97, 0.9, ()), (False, True, 0.97, 0.9, ("ret",)), (True, False, 1.0, 1.0, ()), (True, True, 0.0, 0.5, ("ret",)),
               (False, False, 0.99, 0.0, ())]
# prev, length, ridge, the column that is 0, outputs left out
FIT_CONFIGS = [(True, True, 0.0, None, ()), (False, True, 1e-3, None, ("failed", "steps", "valid")), (True, False, 1e-3, None, ("steps",)),
               (True, True, 0.0, 0, ("valid",)), (False, True, 0.0, -1, ())]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _np(dtype):
    return np.float64 if dtype == abi.F64 else np.float32


def _cpu(t):
    return t.detach().cpu().numpy().copy()


@pytest.fixture(scope="module")
def crafted():
    """The crafted inputs of every shape and dtype, and those with an observation column of zeros, made once and left unchanged."""
    out = {}
    for shape in SHAPES:
        for dtype in (abi.F64, abi.F32):
            out[(shape, dtype, None)] = crafted_critic(*shape, _np(dtype))
            for col in (0, -1):
                out[(shape, dtype, col)] = crafted_critic(*shape, _np(dtype), zero_col=col % shape[3])
    return out


class Call:
    """One call of libos2r_critic.so through ctypes: the inputs of `crafted_critic` on the device, every output between guard bands
    of PAD sentinel elements.  The constructor uploads, gae() and fit() launch and synchronise."""

    def __init__(self, torch, c, shape, dtype):
        from gym_os2r_amd import critic
        self.torch, self.lib, self.dtype, self.shape, self.c = torch, critic.load(), dtype, shape, c
        K, P, S, D = shape
        N, E = S * P, critic.moments(D)
        self.dev = torch.device("cuda:0")
        self.t = {k: torch.as_tensor(v).to(self.dev) for k, v in c.items()}
        real = self.t["obs"].dtype
        self.shapes = dict(adv=(K, N), ret=(K, N), value=(K, N), w=(D + 1, P), lane_mom=(E, N), mom=(E, P), lane_count=(2, N), failed=(P,),
                           steps=(P,), valid=(P,))
        self.sizes = {k: int(np.prod(v)) for k, v in self.shapes.items()}
        self.bufs = {name: torch.full((PAD + size + PAD,), IMARK if name in FIT_INTS else MARK, dtype=torch.int32 if name in FIT_INTS else real,
                                      device=self.dev) for name, size in self.sizes.items()}

    def _lay(self, device):
        from gym_os2r_amd import control
        return control.layout(self.dtype, 3, device, [-1] * self.shape[3])

    def _ptrs(self, names, leave_out):
        return [None if name in leave_out else ctypes.c_void_p(self.bufs[name][PAD:].data_ptr()) for name in names]

    def gae(self, term, length, gamma, lam, leave_out=(), device=0, stream=None):
        K, P, S, D = self.shape
        t = self.t
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        self.rc = self.lib.os2rv_gae(ctypes.byref(self._lay(device)), K, P, S, p(t["obs"]), p(t["obs0"]), p(t["term_obs"]) if term else None,
                                     p(t["reward"]), p(t["done"]), p(t["length"]) if length else None, p(t["value_w"]), gamma, lam,
                                     *self._ptrs(GAE_OUTPUTS, leave_out), stream)
        self.error = self.lib.os2rv_last_error()
        self.torch.cuda.synchronize()
        self.left_out, self.outputs, c = tuple(leave_out), GAE_OUTPUTS, self.c
        self.want = lambda: restate_gae(c["obs"], c["obs0"], c["reward"], c["done"], c["value_w"], P=P, dtype=_np(self.dtype),
                                        term_obs=c["term_obs"] if term else None, length=c["length"] if length else None, gamma=gamma, lam=lam)
        return self

    def fit(self, prev, length, ridge, leave_out=(), device=0, stream=None):
        K, P, S, D = self.shape
        t = self.t
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        self.rc = self.lib.os2rv_value_fit(ctypes.byref(self._lay(device)), K, P, S, p(t["obs"]), p(t["obs0"]), p(t["target"]),
                                           p(t["length"]) if length else None, p(t["prev"]) if prev else None, ridge,
                                           *self._ptrs(FIT_OUTPUTS, leave_out), stream)
        self.error = self.lib.os2rv_last_error()
        self.torch.cuda.synchronize()
        self.left_out, self.outputs, c = tuple(leave_out), FIT_OUTPUTS, self.c
        self.want = lambda: restate_fit(c["obs"], c["obs0"], c["target"], P=P, dtype=_np(self.dtype), length=c["length"] if length else None,
                                        prev=c["prev"] if prev else None, ridge=ridge)
        return self

    def out(self, name):
        """-> the array the call wrote, after a look at its guard bands (and, if it was left out, at all of it)"""
        host = self.bufs[name].cpu().numpy()
        mark = IMARK if name in FIT_INTS else MARK
        assert (host[:PAD] == mark).all() and (host[PAD + self.sizes[name]:] == mark).all(), f"{name}: written outside"
        inner = host[PAD:PAD + self.sizes[name]]
        if name in self.left_out:
            assert (inner == mark).all(), f"{name}: written although left out"
            return None
        return inner.reshape(self.shapes[name])

    def check(self, what):
        """Every output against the restatement, bit for bit (the sign of a zero and the payload of a NaN are not part of the
        contract); the outputs of the other call still hold the sentinel."""
        assert self.rc == abi.OK, (what, self.rc, self.error)
        want = self.want()
        for name in self.outputs:
            got = self.out(name)
            if got is not None:
                assert got.dtype == want[name].dtype and np.array_equal(got, want[name], equal_nan=True), \
                    (what, name, np.argwhere(~((got == want[name]) | (np.isnan(got) & np.isnan(want[name]))))[:4])
        return want


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_of_gae_bit_for_bit(torch_mod, crafted, shape, dtype):
    """adv, ret and value equal the restatement in every configuration; an output that was left out still holds the sentinel."""
    K, P, S, D = shape
    c = crafted[(shape, dtype, None)]
    broken = broken_lanes(P, S)
    seen = set()
    for config in GAE_CONFIGS:
        want = Call(torch_mod, c, shape, dtype).gae(*config).check(f"{shape} {dtype} {config}")
        seen.add(want["adv"].tobytes())
        assert np.isfinite(want["adv"][:, ~broken]).all() or not config[1]          # (without the lengths, NaNs beyond them count)
        assert not broken.any() or np.isnan(want["adv"][0, broken]).all()
    assert len(seen) == len(GAE_CONFIGS) or K * S * P == 1                          # the configurations differ in what they compute


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_of_value_fit_bit_for_bit(torch_mod, crafted, shape, dtype):
    """w, lane_mom, mom, lane_count, failed, steps and valid equal the restatement in every configuration: with and without prev,
    both ridges, a policy without a valid lane, a batch whose first or last observation column is 0."""
    K, P, S, D = shape
    failed = set()
    for prev, length, ridge, col, leave_out in FIT_CONFIGS:
        c = crafted[(shape, dtype, col)]
        want = Call(torch_mod, c, shape, dtype).fit(prev, length, ridge, leave_out).check(f"{shape} {dtype} {(prev, length, ridge, col)}")
        failed |= set(want["failed"].tolist())
        if length:
            assert np.array_equal(want["lane_count"][1].astype(bool), ~broken_lanes(P, S))
        if P > 2 and length:
            assert want["valid"][NONE_VALID] == 0 and want["failed"][NONE_VALID] == (0 if ridge > 0 else 1)
        if ridge > 0:
            assert (want["failed"] == 0).all()
    assert {0, 1} <= failed and (D in failed or K * S < D + 1)                      # no failure, at the first and at the last column


def test_refusals_on_the_device(torch_mod, crafted):
    shape = SHAPES[3]
    c = crafted[(shape, abi.F64, None)]
    for run, prefix, names in ((lambda call, **kw: call.gae(True, True, kw.pop("x", 0.97), 0.9, **kw), b"os2rv_gae: ", GAE_OUTPUTS),
                               (lambda call, **kw: call.fit(True, True, kw.pop("x", 0.0), **kw), b"os2rv_value_fit: ", FIT_OUTPUTS)):
        call = run(Call(torch_mod, c, shape, abi.F64), device=1000)
        assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(prefix), (call.rc, call.error)
        call.left_out = GAE_OUTPUTS + FIT_OUTPUTS
        assert all(call.out(name) is None for name in names)                      # a refused call wrote nothing
        call = run(Call(torch_mod, c, shape, abi.F64), x=float("nan"))
        assert call.rc == abi.ERR_INVALID and call.error in (b"os2rv_gae: gamma must be finite", b"os2rv_value_fit: ridge must be finite")
        call.left_out = GAE_OUTPUTS + FIT_OUTPUTS
        assert all(call.out(name) is None for name in names)


def test_a_call_on_another_stream(torch_mod, crafted):
    torch = torch_mod
    shape = SHAPES[3]
    c = crafted[(shape, abi.F32, None)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    handle = ctypes.c_void_p(side.cuda_stream)
    assert side.cuda_stream != 0
    Call(torch, c, shape, abi.F32).gae(True, True, 0.97, 0.9, stream=handle).check("gae on a side stream")
    Call(torch, c, shape, abi.F32).fit(True, True, 1e-3, stream=handle).check("value_fit on a side stream")


# ---------------------------------------------------------------------------------------
# through HipSim
# ---------------------------------------------------------------------------------------
def _guarded(torch, sim, shape, dtype=None, mark=MARK):
    """A tensor of `shape` on the handle's device between guard bands of PAD sentinels -> (the flat buffer, the tensor)."""
    size = int(np.prod(shape))
    flat = torch.full((PAD + size + PAD,), mark, dtype=dtype or sim.dtype, device=sim.device)
    return flat, flat[PAD:PAD + size].view(*shape)


def _bands_hold(flat, size, mark):
    host = _cpu(flat)
    return (host[:PAD] == mark).all() and (host[PAD + size:] == mark).all()


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_the_into_forms_write_their_outputs_and_nothing_else(torch_mod, crafted, dtype):
    """On the crafted inputs of (9, 3, 65, 10), through a handle of the same observation width: the caller's tensors, between
    sentinels, hold the restatement's bits and what the allocating calls return; the sentinels stand."""
    torch = torch_mod
    from gym_os2r_amd import critic
    from gym_os2r_amd.sim import HipSim
    shape = K, P, S, D = SHAPES[3]
    N, E, i32 = S * P, critic.moments(D), torch.int32
    sim = HipSim(make_config("free_hip", "BalancingV2", False, num_envs=4, contact=True, seed=1, dtype=dtype)[0])
    assert sim.D == D
    raw = crafted[(shape, dtype, None)]
    c = {k: torch.as_tensor(v).to(sim.device) for k, v in raw.items()}
    kw = dict(obs0=c["obs0"], policies=P, length=c["length"])
    bufs = {name: _guarded(torch, sim, s) for name, s in (("adv", (K, N)), ("ret", (K, N)), ("values", (K, N)), ("w", (D + 1, P)),
                                                          ("lane_mom", (E, N)), ("mom", (E, P)))}
    ints = {name: _guarded(torch, sim, s, i32, IMARK) for name, s in (("lane_count", (2, N)), ("failed", (P,)), ("steps", (P,)), ("valid", (P,)))}
    sim.gae_into(c["obs"], c["reward"], c["done"], c["value_w"], bufs["adv"][1], bufs["values"][1], term_obs=c["term_obs"], gamma=0.97, lam=0.9,
                 ret=bufs["ret"][1], **kw)
    sim.value_fit_into(c["obs"], c["target"], bufs["w"][1], bufs["lane_mom"][1], bufs["mom"][1], ints["lane_count"][1], prev=c["prev"],
                       ridge=1e-3, failed=ints["failed"][1], steps=ints["steps"][1], valid=ints["valid"][1], **kw)
    adv, ret, values = sim.gae(c["obs"], c["reward"], c["done"], c["value_w"].t(), term_obs=c["term_obs"], gamma=0.97, lam=0.9, want_values=True, **kw)
    w, failed, steps, valid = sim.value_fit(c["obs"], c["target"], prev=c["prev"].t(), ridge=1e-3, **kw)
    only_adv = sim.gae(c["obs"], c["reward"], c["done"], c["value_w"].t(), term_obs=c["term_obs"], gamma=0.97, lam=0.9, want_returns=False, **kw)
    torch.cuda.synchronize()
    assert only_adv[1] is None and only_adv[2] is None and torch.equal(only_adv[0].view(torch.uint8), adv.view(torch.uint8))
    assert tuple(w.shape) == (P, D + 1) and w.t().is_contiguous()
    want = restate_gae(raw["obs"], raw["obs0"], raw["reward"], raw["done"], raw["value_w"], P=P, dtype=_np(dtype), term_obs=raw["term_obs"],
                       length=raw["length"], gamma=0.97, lam=0.9)
    want.update(restate_fit(raw["obs"], raw["obs0"], raw["target"], P=P, dtype=_np(dtype), length=raw["length"], prev=raw["prev"], ridge=1e-3))
    want["values"] = want["value"]
    for name, (flat, t) in list(bufs.items()) + list(ints.items()):
        assert _bands_hold(flat, t.numel(), IMARK if name in ints else MARK), name
        assert np.array_equal(_cpu(t), want[name], equal_nan=True), name
    for got, name in ((adv, "adv"), (ret, "ret"), (values, "value"), (w.t(), "w"), (failed, "failed"), (steps, "steps"), (valid, "valid")):
        assert np.array_equal(_cpu(got), want[name], equal_nan=True), name
    sim.close()


N_REAL, K_REAL, P_REAL = 96, 12, 3


@pytest.fixture(scope="module")
def window(torch_mod):
    """One noisy window of K_REAL steps with auto-reset and a TimeLimit of 5 steps on a real handle of N_REAL environments from
    reset(): made once, shared, left unchanged."""
    torch = torch_mod
    from gym_os2r_amd.sim import HipSim
    sim = HipSim(make_config("free_hip", "BalancingV2", False, num_envs=N_REAL, contact=True, seed=5, auto_reset=True, dtype=abi.F64,
                             max_episode_steps=5)[0])
    D, dev = sim.D, sim.device
    rng = np.random.default_rng(11)
    theta = torch.as_tensor(rng.normal(0, 0.3, (2, D + 1))).to(dev)
    sigma = torch.as_tensor(np.array([0.3, 0.5])).to(dev)
    obs0 = sim.reset().clone()
    ret, length, (O, R, Dn, T, _), (A, E) = sim.rollout_policy(K_REAL, theta, sigma=sigma, salt=3, want_outputs=True, want_terminal=True,
                                                               want_actions=True, want_noise=True)
    torch.cuda.synchronize()
    value_w = torch.as_tensor(rng.normal(0, 0.5, (P_REAL, D + 1))).to(dev)
    yield dict(sim=sim, sigma=sigma, obs0=obs0, O=O, R=R, Dn=Dn, T=T, A=A, E=E, value_w=value_w)
    sim.close()


def test_real_consumer_the_advantages_of_a_noisy_rollout(torch_mod, window):
    """gae() of what rollout_policy returned -- truncations, terminal observations and post-reset observations from the simulator
    -- equals the restatement bit for bit, with and without term_obs; value_fit() on its returns likewise."""
    torch, w = torch_mod, window
    sim, O, R, Dn, T, obs0, vw = (w[k] for k in ("sim", "O", "R", "Dn", "T", "obs0", "value_w"))
    flags = _cpu(Dn)
    assert ((flags & 2) != 0).sum() >= N_REAL and (flags == 2).any()               # every lane ran into the TimeLimit, twice
    kw = dict(obs0=obs0, policies=P_REAL, gamma=0.97, lam=0.9)
    adv, ret, values = sim.gae(O, R, Dn, vw, term_obs=T, want_values=True, **kw)
    bare = sim.gae(O, R, Dn, vw, **kw)
    fit = sim.value_fit(O, ret, obs0=obs0, policies=P_REAL, prev=vw, ridge=1e-3)
    torch.cuda.synchronize()
    host = dict(P=P_REAL, dtype=np.float64, gamma=0.97, lam=0.9)
    want = restate_gae(_cpu(O), _cpu(obs0), _cpu(R), flags, _cpu(vw).T, term_obs=_cpu(T), **host)
    want_bare = restate_gae(_cpu(O), _cpu(obs0), _cpu(R), flags, _cpu(vw).T, **host)
    for got, exp in ((adv, want["adv"]), (ret, want["ret"]), (values, want["value"]), (bare[0], want_bare["adv"]), (bare[1], want_bare["ret"])):
        assert np.array_equal(_cpu(got), exp)
    assert bare[2] is None and not np.array_equal(want["adv"], want_bare["adv"]) and np.isfinite(want["adv"]).all()
    want_fit = restate_fit(_cpu(O), _cpu(obs0), want["ret"], P=P_REAL, dtype=np.float64, prev=_cpu(vw).T, ridge=1e-3)
    for got, name in zip(fit, ("w", "failed", "steps", "valid")):
        assert np.array_equal(_cpu(got.t() if name == "w" else got), want_fit[name]), name
    assert want_fit["failed"].tolist() == [0] * P_REAL and want_fit["valid"].tolist() == [N_REAL // P_REAL] * P_REAL


def test_the_policy_gradient_takes_the_advantages_as_they_are(torch_mod, window):
    """policy_gradient(rewards=adv, done=done, gamma=0.0) weights step k of lane l with adv[k][l]: its lane sums equal a numpy
    statement of the per-step-weighted sums bit for bit -- the composition examples/actor_critic_balancing.py relies on."""
    torch, w = torch_mod, window
    sim, O, R, Dn, T, A, E, obs0, sigma = (w[k] for k in ("sim", "O", "R", "Dn", "T", "A", "E", "obs0", "sigma"))
    adv, _, _ = sim.gae(O, R, Dn, w["value_w"], term_obs=T, obs0=obs0, policies=P_REAL, gamma=0.97, lam=0.9)
    grad, steps, clipped, valid, _, lane, rtg = sim.policy_gradient(O, E, sigma, policies=P_REAL, obs0=obs0, actions=A, rewards=adv, done=Dn,
                                                                   gamma=0.0, want_lane=True, want_rtg=True)
    torch.cuda.synchronize()
    assert torch.equal(rtg, adv)                                                    # psi = adv[k][l], whatever done holds
    a, x, eps, act, sg = _cpu(adv), np.concatenate([_cpu(obs0)[None], _cpu(O)[:-1]]), _cpu(E), _cpu(A), _cpu(sigma)
    D = sim.D
    L = np.zeros((2, D + 1, N_REAL))
    for k in range(K_REAL - 1, -1, -1):
        for j in range(2):
            opened = np.abs(act[k, :, j]) < 1
            c = a[k] * (eps[k, :, j] / sg[j])
            for d in range(D):
                L[j, d] = np.where(opened, L[j, d] + c * x[k, :, d], L[j, d])
            L[j, D] = np.where(opened, L[j, D] + c, L[j, D])
    assert np.array_equal(_cpu(lane.permute(1, 2, 0)), L) and (L != 0).any()
    want = restate_pg(_cpu(O), eps, sg, P=P_REAL, dtype=np.float64, obs0=_cpu(obs0), action=act, reward=a, done=_cpu(Dn), gamma=0.0)
    assert np.array_equal(_cpu(grad.permute(1, 2, 0)), want["grad"]) and int(valid.sum()) == N_REAL
