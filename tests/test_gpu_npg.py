"""os2rn_natural_step on the device (libos2r_npg.so, include/os2r_npg.h): every output bit for bit against the numpy
restatement of tests/test_npg_host.py on crafted inputs -- obs0 given and null, shared and per-lane sigma, tanh, with and without
the gradient of the widths, outputs left out (the solve then adds the integer totals up itself), damping and kl of 0 --, 300
policies of two samples (the few-samples sum and ten workgroups of the solve), refusals that write nothing, and the call
against its real consumer: a noisy rollout_policy on a real handle, gae, policy_gradient, natural_step, theta += step and the
next rollout."""
import ctypes

import numpy as np
import pytest

from gym_os2r_amd import abi
from helpers import make_config
from test_npg_host import CLIPPED, DAMPING, KL, SHAPES, crafted_npg, restate_npg

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
FLOATS = ("step", "dir", "lsig_step", "beta", "quad", "lane_mom", "mom")
OUTPUTS = ("step", "dir", "lsig_step", "beta", "quad", "failed", "steps", "open", "valid", "lane_mom", "mom", "lane_count")   # the header's order
OPTIONAL = ("dir", "beta", "quad", "failed", "steps", "open", "valid")
# obs0, per-lane sigma, tanh, the gradient of the widths, outputs left out, damping, kl
CONFIGS = [(True, False, False, True, (), DAMPING, KL),
           (False, True, False, True, ("steps",), DAMPING, KL),
           (True, True, True, False, ("open", "dir"), DAMPING, 0.5),
           (False, False, True, True, ("valid", "failed"), 0.25, KL),
           (True, False, False, False, OPTIONAL, DAMPING, KL),                       # only step and the scratch arrays
           (True, False, False, True, ("beta", "quad"), 0.0, 0.0)]


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
    return {(shape, dtype): crafted_npg(*shape, _np(dtype)) for shape in SHAPES + [FEW] for dtype in (abi.F64, abi.F32)}


FEW = (3, 300, 2, 10)                   # K, P, S, D: the few-samples sum over two workgroups of policies, ten of the solve


class Call:
    """One os2rn_natural_step call through ctypes: the inputs of `crafted_npg` on the device, every output between guard bands of
    PAD sentinel elements.  The constructor uploads, run() launches and synchronises."""

    def __init__(self, torch, c, shape, dtype):
        from gym_os2r_amd import npg
        self.torch, self.lib, self.dtype, self.shape, self.c = torch, npg.load(), dtype, shape, c
        K, P, S, D = shape
        N, E = S * P, npg.moments(D)
        self.dev = torch.device("cuda:0")
        self.t = {k: torch.as_tensor(v).to(self.dev) for k, v in c.items() if k != "broken"}
        real = self.t["obs"].dtype
        self.shapes = dict(step=(2, D + 1, P), dir=(2, D + 1, P), lsig_step=(2, P), beta=(P,), quad=(P,), failed=(3, P), steps=(P,), open=(2, P),
                           valid=(P,), lane_mom=(E, N), mom=(E, P), lane_count=(4, N))
        self.sizes = {k: int(np.prod(v)) for k, v in self.shapes.items()}
        self.bufs = {name: torch.full((PAD + size + PAD,), MARK if name in FLOATS else IMARK, dtype=real if name in FLOATS else torch.int32,
                                      device=self.dev) for name, size in self.sizes.items()}

    def run(self, obs0, per_lane, tanh, lsig, leave_out=(), damping=DAMPING, kl=KL, device=0):
        from gym_os2r_amd import control, npg
        K, P, S, D = self.shape
        lay = control.layout(self.dtype, 3, device, [-1] * D)
        t = self.t
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        leave_out = tuple(leave_out) + (() if lsig else ("lsig_step",))
        outs = [None if name in leave_out else p(self.bufs[name][PAD:]) for name in OUTPUTS]
        self.rc = self.lib.os2rn_natural_step(
            ctypes.byref(lay), K, P, S, (npg.TANH if tanh else 0) | (npg.SIGMA_PER_LANE if per_lane else 0), p(t["obs"]),
            p(t["obs0"]) if obs0 else None, None if tanh else p(t["action"]), p(t["lane_sigma"] if per_lane else t["sigma"]), p(t["length"]),
            p(t["grad"]), p(t["lsig_grad"]) if lsig else None, damping, kl, *outs, None)
        self.error = self.lib.os2rn_last_error()
        self.torch.cuda.synchronize()
        self.left_out = leave_out
        c = self.c
        self.args = (c["obs"], c["lane_sigma"] if per_lane else c["sigma"], c["grad"])
        self.want = dict(P=P, dtype=_np(self.dtype), obs0=c["obs0"] if obs0 else None, action=None if tanh else c["action"], tanh=tanh,
                         length=c["length"], lsig_grad=c["lsig_grad"] if lsig else None, damping=damping, kl=kl)
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

    def check(self, what):
        """Every output against the restatement, bit for bit (the sign of a zero and the payload of a NaN are not part of the
        contract)."""
        assert self.rc == abi.OK, (what, self.rc, self.error)
        want = restate_npg(*self.args, **self.want)
        for name in OUTPUTS:
            got = self.out(name)
            if got is not None:
                assert got.dtype == want[name].dtype and np.array_equal(got, want[name], equal_nan=True), \
                    (what, name, np.argwhere(~((got == want[name]) | (np.isnan(got) & np.isnan(want[name]))))[:4])
        return want


def _every_configuration(torch, c, shape, dtype):
    K, P, S, D = shape
    seen = set()
    for config in CONFIGS:
        what = f"{shape} {_np(dtype).__name__} {config}"
        want = Call(torch, c, shape, dtype).run(*config).check(what)
        seen.add(want["step"].tobytes())
        assert np.isfinite(want["step"]).all() and np.isfinite(want["mom"]).all()
        assert np.array_equal(want["lane_count"][3] == 0, c["broken"])                 # a NaN observation: invalid, left out
        if P > 2:
            assert want["valid"][2] == 0 and (want["step"][:, :, 2] == 0).all() and want["failed"][:, 2].tolist() == [1, 1, 1]
        if P > 1 and not config[2] and want["steps"][CLIPPED] > 0:                    # the component clipped on every step
            assert want["open"][1, CLIPPED] == 0 and want["failed"][1, CLIPPED] == (1 if config[5] == 0.0 else 0)
        if config[6] == 0.0:
            assert set(want["beta"].tolist()) <= {0.0, 1.0} and np.array_equal(want["step"], want["dir"])
    assert len(seen) == len(CONFIGS)                                                  # the configurations differ in what they compute


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_against_the_restatement(torch_mod, crafted, shape, dtype):
    """step, dir, lsig_step, beta, quad, failed, steps, open, valid, lane_mom, mom and lane_count equal the restatement in every
    configuration; an output that was left out still holds the sentinel, and the outputs beside it are unchanged by its absence."""
    _every_configuration(torch_mod, crafted[(shape, dtype)], shape, dtype)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_three_hundred_policies_of_two_samples(torch_mod, crafted, dtype):
    """P = 300 at S = 2: the few-samples sum kernel over two workgroups of policies, ten workgroups of the solve, the last one
    partly filled."""
    want = Call(torch_mod, crafted[(FEW, dtype)], FEW, dtype).run(*CONFIGS[0]).check(f"{FEW} {_np(dtype).__name__}")
    assert (want["failed"][:, 0] == 0).all() and want["failed"][:, 2].tolist() == [1, 1, 1] and (want["beta"] > 0).sum() == FEW[1] - 1
    bare = Call(torch_mod, crafted[(FEW, dtype)], FEW, dtype).run(*CONFIGS[4]).check(f"{FEW} {_np(dtype).__name__}, step alone")
    assert np.array_equal(bare["dir"], want["dir"]) and not np.array_equal(bare["step"], want["step"])   # (q without the widths' share)


def test_refusals_on_the_device(torch_mod, crafted):
    shape = SHAPES[1]
    c = crafted[(shape, abi.F64)]
    call = Call(torch_mod, c, shape, abi.F64).run(True, False, False, True, device=1000)
    assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(b"os2rn_natural_step: "), (call.rc, call.error)
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)                        # a refused call wrote nothing
    call = Call(torch_mod, c, shape, abi.F64).run(True, False, False, True, kl=float("nan"))
    assert call.rc == abi.ERR_INVALID and call.error == b"os2rn_natural_step: kl must be finite"
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)
    call = Call(torch_mod, c, shape, abi.F64).run(True, False, False, True, damping=-1.0)
    assert call.rc == abi.ERR_INVALID and call.error == b"os2rn_natural_step: damping must be >= 0"
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)


# ---------------------------------------------------------------------------------------
# the real consumer
# ---------------------------------------------------------------------------------------
P_REAL, S_REAL, K_REAL = 8, 32, 20


def _cpu(t):
    return t.detach().cpu().numpy().copy()


def test_real_consumer_a_natural_step_on_a_noisy_rollout(torch_mod):
    """A handle of 8 policies x 32 samples = 256 environments, 20 steps: noisy rollout_policy -> gae -> policy_gradient ->
    natural_step.  step, lsig_step, beta, quad, failed and the counts equal the restatement on the rollout's own arrays bit for
    bit; beta is finite and positive for every policy with failed == 0; theta + step goes into the next rollout of the same
    seeds and widths as it is; natural_step_into on the caller's tensors gives the bits of the allocating call."""
    torch = torch_mod
    from gym_os2r_amd import npg
    from gym_os2r_amd.sim import HipSim
    N = P_REAL * S_REAL
    sim = HipSim(make_config("free_hip", "BalancingV2", False, num_envs=N, contact=True, seed=5, auto_reset=True, dtype=abi.F64)[0])
    D, dev = sim.D, sim.device
    rng = np.random.default_rng(23)
    theta = torch.as_tensor(rng.normal(0, 0.3, (2, D + 1, P_REAL))).to(dev).permute(2, 0, 1)       # [P, 2, D+1] over the kernel's layout
    sigma = torch.as_tensor(np.array([0.3, 0.4])).to(dev)
    value_w = torch.as_tensor(rng.normal(0, 0.1, (P_REAL, D + 1))).to(dev)
    lanes = torch.arange(N, device=dev) % P_REAL                                                    # lane s P + p runs policy p
    obs0 = sim.reset()
    roll = dict(sigma=sigma, salt=3, first_episode=False, want_outputs=True, want_actions=True, want_noise=True)
    ret, length, (O, R, Dn, _, _), (A, E) = sim.rollout_policy(K_REAL, theta[lanes], **roll)
    adv, _, _ = sim.gae(O, R, Dn, value_w, obs0=obs0, policies=P_REAL, gamma=0.97, lam=0.9)
    common = dict(policies=P_REAL, obs0=obs0, actions=A)
    grad, _, clipped, _, lsig, _, _ = sim.policy_gradient(O, E, sigma, rewards=adv, done=Dn, gamma=0.0, want_log_sigma=True, **common)
    got = sim.natural_step(O, sigma, grad, lsig_grad=lsig, damping=DAMPING, kl=KL, want_dir=True, **common)
    torch.cuda.synchronize()
    step, lsig_step, beta, quad, failed, steps, opened, valid, direction = got
    assert tuple(step.shape) == (P_REAL, 2, D + 1) == tuple(direction.shape) and step.permute(1, 2, 0).is_contiguous()
    assert tuple(lsig_step.shape) == (P_REAL, 2) == tuple(opened.shape) and tuple(failed.shape) == (P_REAL, 3)
    to_kernel = lambda w: _cpu(w.permute(1, 2, 0))
    want = restate_npg(_cpu(O), _cpu(sigma), to_kernel(grad), P=P_REAL, dtype=np.float64, obs0=_cpu(obs0), action=_cpu(A), lsig_grad=_cpu(lsig.t()),
                       damping=DAMPING, kl=KL)
    for name, have in (("step", step.permute(1, 2, 0)), ("dir", direction.permute(1, 2, 0)), ("lsig_step", lsig_step.t()), ("beta", beta),
                       ("quad", quad), ("failed", failed.t()), ("steps", steps), ("open", opened.t()), ("valid", valid)):
        assert np.array_equal(_cpu(have), want[name]), name
    b, f = _cpu(beta), _cpu(failed)
    assert (f == 0).all() and np.isfinite(b).all() and (b > 0).all() and (_cpu(valid) == S_REAL).all() and (_cpu(steps) == S_REAL * K_REAL).all()
    assert np.array_equal(_cpu(opened), S_REAL * K_REAL - _cpu(clipped))                           # open is what the clip left
    # the step goes into the next rollout as it is: the same seeds (reset and salt), the widths unchanged
    new = theta + step
    sim.reset()
    ret2, _, (O2, _, _, _, _), (A2, E2) = sim.rollout_policy(K_REAL, new[lanes], **roll)
    torch.cuda.synchronize()
    assert np.isfinite(_cpu(ret2)).all() and np.isfinite(_cpu(O2)).all() and not np.array_equal(_cpu(A2), _cpu(A))
    # the divergence of the step on the batch it was formed on, from the observations: q = d' (F + damping I) d >= d' F d, so the
    # divergence is kl at the most, and less by what the damping took
    prev = np.concatenate([_cpu(obs0)[None], _cpu(O)[:-1]])
    phi = np.concatenate([prev, np.ones((K_REAL, N, 1))], 2).reshape(K_REAL, S_REAL, P_REAL, D + 1)
    inside = (np.abs(_cpu(A)) < 1).reshape(K_REAL, S_REAL, P_REAL, 2)
    shift = np.einsum("kspa,jap->kspj", phi, want["step"])
    mean = (0.5 * inside * shift * shift / _cpu(sigma) ** 2).sum((0, 1, 3)) / (S_REAL * K_REAL)
    widths = (want["lsig_step"] ** 2 * want["open"] / want["steps"][None]).sum(0)                   # 1/2 (2 n_j / c) dls^2
    print("natural_step on the rollout: the divergence of the mean step", mean, "of the widths", widths, "kl", KL)
    assert (mean + widths <= KL * (1 + 1e-9)).all() and (mean > 0).all()
    # natural_step_into on the caller's tensors
    i32, E_ = torch.int32, npg.moments(D)
    z = lambda *s, dtype=sim.dtype: torch.full(s, -3, dtype=dtype, device=dev)
    st, lm, mm, cnt = z(2, D + 1, P_REAL), z(E_, N), z(E_, P_REAL), z(4, N, dtype=i32)
    dr, ls, bt, qd, fl = z(2, D + 1, P_REAL), z(2, P_REAL), z(P_REAL), z(P_REAL), z(3, P_REAL, dtype=i32)
    sim.natural_step_into(O, sigma, grad.permute(1, 2, 0), st, lm, mm, cnt, lsig_grad=lsig.t(), damping=DAMPING, kl=KL, dir=dr, lsig_step=ls,
                          beta=bt, quad=qd, failed=fl, **common)                                    # (the counts left out: the solve adds them up)
    torch.cuda.synchronize()
    for have, ret in ((st.permute(2, 0, 1), step), (dr.permute(2, 0, 1), direction), (ls.t(), lsig_step), (bt, beta), (qd, quad), (fl.t(), failed)):
        assert have.shape == ret.shape and np.array_equal(_cpu(have).view(np.uint8), _cpu(ret).view(np.uint8))
    assert np.array_equal(_cpu(cnt), want["lane_count"]) and np.array_equal(_cpu(mm), want["mom"]) and np.array_equal(_cpu(lm), want["lane_mom"])
    sim.close()
