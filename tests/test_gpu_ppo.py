"""os2ro_ppo_gradient on the device (libos2r_ppo.so, include/os2r_ppo.h): rho within 8 ulp of numpy's exp of the bit-exact
argument, every other output bit for bit against the numpy restatement of tests/test_ppo_host.py fed with the device's rho, on
crafted inputs -- obs0 given and null, shared and per-lane sigma, a new width given and null, tanh, outputs left out --, the
first-epoch identity against os2rg_policy_gradient on the same device arrays, and the call against its real consumer: a noisy
rollout_policy on a real handle, gae, two epochs of ppo_gradient, and ppo_gradient_into on the caller's tensors."""
import ctypes

import numpy as np
import pytest

from gym_os2r_amd import abi
from helpers import make_config
from test_gpu_mppi import ULPS
from test_pg_host import SHAPES
from test_ppo_host import CLIP, MARGIN, SAME, at_most_a_quarter_invalid, crafted_ppo, restate_ppo

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
FLOATS = ("grad", "lane_grad", "lsig_grad", "lane_lsig", "stat", "lane_stat", "ratio")
OUTPUTS = ("grad", "lane_grad", "lsig_grad", "lane_lsig", "stat", "lane_stat", "steps", "clipped", "gated", "valid", "ratio",
           "lane_count")                                                             # the header's order
OPTIONAL = ("lsig_grad", "lane_lsig", "stat", "steps", "clipped", "gated", "valid", "ratio")
# obs0, per-lane sigma, a new width, tanh, outputs left out
CONFIGS = [(True, False, False, False, ()),
           (False, True, False, False, ("clipped",)),
           (True, True, True, False, ("steps", "stat")),
           (False, False, True, True, ("lsig_grad", "lane_lsig", "gated")),
           (True, True, False, True, ("valid",)),
           (True, False, True, False, OPTIONAL)]
# The largest distance of the device's rho from the float64 textbook ratio formed from the rollout's own actions, relative to
# the textbook ratio, over the counted steps on which no clip bound, measured on the MI355X this test was written on
# (test_real_consumer_two_epochs_on_a_noisy_rollout prints it), per squash
MEASURED_RATIO = {False: 3.553e-15, True: 6.128e-14}


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
    return {(shape, dtype): crafted_ppo(*shape, _np(dtype)) for shape in SHAPES for dtype in (abi.F64, abi.F32)}


class Call:
    """One os2ro_ppo_gradient call through ctypes: the inputs of `crafted_ppo` on the device, every output between guard bands of
    PAD sentinel elements.  The constructor uploads, run() launches and synchronises."""

    def __init__(self, torch, c, shape, dtype):
        from gym_os2r_amd import ppo
        self.torch, self.lib, self.dtype, self.shape, self.c = torch, ppo.load(), dtype, shape, c
        K, P, S, D = shape
        N = S * P
        self.dev = torch.device("cuda:0")
        self.t = {k: torch.as_tensor(v).to(self.dev) for k, v in c.items()}
        real = self.t["obs"].dtype
        self.shapes = dict(grad=(2, D + 1, P), lane_grad=(2, D + 1, N), lsig_grad=(2, P), lane_lsig=(2, N), stat=(3, P), lane_stat=(3, N),
                           steps=(P,), clipped=(2, P), gated=(P,), valid=(P,), ratio=(K, N), lane_count=(5, N))
        self.sizes = {k: int(np.prod(v)) for k, v in self.shapes.items()}
        self.bufs = {name: torch.full((PAD + size + PAD,), MARK if name in FLOATS else IMARK, dtype=real if name in FLOATS else torch.int32,
                                      device=self.dev) for name, size in self.sizes.items()}

    def run(self, obs0, per_lane, new_width, tanh, leave_out=(), device=0, clip=CLIP, same_weights=False):
        from gym_os2r_amd import control, ppo
        K, P, S, D = self.shape
        lay = control.layout(self.dtype, 3, device, [-1] * D)
        t = self.t
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        outs = [None if name in leave_out else p(self.bufs[name][PAD:]) for name in OUTPUTS]
        self.rc = self.lib.os2ro_ppo_gradient(
            ctypes.byref(lay), K, P, S, (ppo.TANH if tanh else 0) | (ppo.SIGMA_PER_LANE if per_lane else 0), p(t["obs"]),
            p(t["obs0"]) if obs0 else None, p(t["noise"]), None if tanh else p(t["action"]), p(t["lane_sigma"] if per_lane else t["sigma"]),
            p(t["sigma_new"]) if new_width else None, p(t["weight_old"] if same_weights else t["weight"]), p(t["weight_old"]), p(t["length"]),
            p(t["adv"]), clip, *outs, None)
        self.error = self.lib.os2ro_last_error()
        self.torch.cuda.synchronize()
        self.left_out = tuple(leave_out)
        c = self.c
        self.args = (c["obs"], c["noise"], c["lane_sigma"] if per_lane else c["sigma"], c["weight_old"] if same_weights else c["weight"],
                     c["weight_old"], c["adv"])
        self.want = dict(P=P, dtype=_np(self.dtype), clip=clip, obs0=c["obs0"] if obs0 else None, action=None if tanh else c["action"], tanh=tanh,
                         length=c["length"], sigma_new=c["sigma_new"] if new_width else None)
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

    def check(self, what, ratio=None):
        """rho against numpy's exp of the bit-exact h times r' (within ULPS, exactly 1 where h = 0 and r' = 1, exactly 0 behind len,
        not finite where numpy's is not), then every other output against the restatement fed with the device's rho, bit for bit
        (the sign of a zero and the payload of a NaN are not part of the contract).  `ratio`: the device's rho of another run of the
        same configuration, where this one left it out."""
        assert self.rc == abi.OK, (what, self.rc, self.error)
        dt = self.want["dtype"]
        got_ratio = self.out("ratio")
        if got_ratio is not None:
            plain = restate_ppo(*self.args, **self.want)                               # (rho formed with np.exp)
            assert at_most_a_quarter_invalid(plain, self.shape[1], self.shape[2])     # (on the CPU, before the outputs are compared)
            K = self.shape[0]
            counted = np.arange(K)[:, None] < plain["lane_count"][0][None]
            h, rprod = plain["h"].astype(np.float64), plain["rprod"].astype(np.float64)
            with np.errstate(all="ignore"):
                ref = np.exp(h) * rprod                                                # numpy's exp, in double for both dtypes
                known = counted & np.isfinite(ref) & (ref <= np.finfo(dt).max)
                ulp = np.spacing(np.maximum(np.abs(ref), np.finfo(dt).tiny).astype(dt)).astype(np.float64)
                err = np.where(known, np.abs(got_ratio.astype(np.float64) - ref) / ulp, 0)
            print(f"ppo ratio {what}: worst {err.max():.3f} ulp over {int(known.sum())} steps")
            assert err.max() <= ULPS, (what, err.max())
            assert (got_ratio[~counted] == 0).all() and (got_ratio[counted & (plain["h"] == 0) & (plain["rprod"] == 1)] == 1).all()
            assert not np.isfinite(got_ratio[counted & ~known]).any()
            ratio = got_ratio
        assert ratio is not None
        want = restate_ppo(*self.args, ratio=ratio, **self.want)
        for name in OUTPUTS:
            got = self.out(name)
            if got is not None:
                assert got.dtype == want[name].dtype and np.array_equal(got, want[name], equal_nan=True), \
                    (what, name, np.argwhere(~((got == want[name]) | (np.isnan(got) & np.isnan(want[name]))))[:4])
        return want


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_against_the_restatement(torch_mod, crafted, shape, dtype):
    """rho within 8 ulp; grad, lane_grad, lsig_grad, lane_lsig, stat, lane_stat, steps, clipped, gated, valid and lane_count equal
    the restatement fed with the device's rho in every configuration; an output that was left out still holds the sentinel, and
    with ratio left out the other outputs are those of the run that had it."""
    K, P, S, D = shape
    c = crafted[(shape, dtype)]
    seen = set()
    for config in CONFIGS:
        what = f"{shape} {_np(dtype).__name__} {config[:4]}"
        ratio = None
        if "ratio" in config[4]:
            full = Call(torch_mod, c, shape, dtype).run(*config[:4])
            full.check(what + " (all outputs)")
            ratio = full.out("ratio")
        want = Call(torch_mod, c, shape, dtype).run(*config).check(what, ratio)
        if "ratio" in config[4]:
            for name in ("grad", "lane_grad", "lane_stat", "lane_count"):
                assert np.array_equal(full.out(name), want[name], equal_nan=True), name
        seen.add(want["grad"].tobytes())
        if P > 2:
            assert want["valid"][2] == 0 and (want["grad"][:, :, 2] == 0).all()
        assert np.isfinite(want["grad"]).all() and np.isfinite(want["stat"]).all()
        if S >= 6 and not config[2]:
            assert not np.isfinite(want["lane_stat"]).all()                            # (an overflowing rho, or the infinite adv)
    assert len(seen) == len(CONFIGS) or K * S * P == 1                              # the configurations differ in what they compute
    if P > 1 and S >= 5:
        new = Call(torch_mod, c, shape, dtype).run(True, True, True, False)
        new.check("rho at the bounds")
        dt = _np(dtype)
        rho = new.out("ratio")
        assert (rho[:, 3 * P + SAME] == dt(1 + CLIP)).all() and (rho[:, 4 * P + SAME] == dt(1 - CLIP)).all()
        assert new.out("lane_count")[3][[3 * P + SAME, 4 * P + SAME]].tolist() == [0, 0]


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_first_epoch_is_the_score_function_gradient_on_the_device(torch_mod, crafted, shape, dtype):
    """os2ro_ppo_gradient with weight == weight_old (one array for both, and two equal arrays) against
    os2rg_policy_gradient(reward = adv, done all ones, gamma = 0) on the same device arrays: grad, lane_grad, lsig_grad,
    lane_lsig, steps, clipped and valid are equal bit for bit; every rho is 1 and nothing is gated."""
    torch = torch_mod
    from gym_os2r_amd import control, pg
    K, P, S, D = shape
    N = S * P
    c = crafted[(shape, dtype)]
    for per_lane, tanh in ((False, False), (True, True)):
        ours = Call(torch, c, shape, dtype).run(True, per_lane, False, tanh, same_weights=True)
        assert ours.rc == abi.OK, ours.error
        t = ours.t
        real = t["obs"].dtype
        z = lambda *s, dtype=real: torch.full(s, -3, dtype=dtype, device=ours.dev)
        i32 = torch.int32
        theirs = dict(grad=z(2, D + 1, P), lane_grad=z(2, D + 1, N), lsig_grad=z(2, P), lane_lsig=z(2, N), steps=z(P, dtype=i32),
                      clipped=z(2, P, dtype=i32), valid=z(P, dtype=i32))
        count = z(4, N, dtype=i32)
        done = torch.ones(K, N, dtype=torch.uint8, device=ours.dev)
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        lay = control.layout(dtype, 3, 0, [-1] * D)
        lib = pg.load()
        rc = lib.os2rg_policy_gradient(ctypes.byref(lay), K, P, S, (pg.TANH if tanh else 0) | (pg.SIGMA_PER_LANE if per_lane else 0), p(t["obs"]),
                                       p(t["obs0"]), p(t["noise"]), None if tanh else p(t["action"]), p(t["lane_sigma"] if per_lane else t["sigma"]),
                                       p(t["length"]), None, p(t["adv"]), p(done), 0.0, None, p(theirs["grad"]), p(theirs["lane_grad"]),
                                       p(theirs["lsig_grad"]), p(theirs["lane_lsig"]), p(theirs["steps"]), p(theirs["clipped"]), p(theirs["valid"]),
                                       None, p(count), None)
        torch.cuda.synchronize()
        assert rc == abi.OK, lib.os2rg_last_error()
        for name, want in theirs.items():
            got, want = ours.out(name), want.cpu().numpy()
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), (shape, dtype, per_lane, tanh, name)
        lane_count, rho = ours.out("lane_count"), ours.out("ratio")
        assert np.array_equal(lane_count[[0, 1, 2, 4]], count.cpu().numpy()) and (lane_count[3] == 0).all() and (ours.out("gated") == 0).all()
        assert (rho[np.arange(K)[:, None] < lane_count[0][None]] == 1).all() and (ours.out("lane_stat")[1:] == 0).all()
        # two arrays that hold the same weights give the same bits
        twin = Call(torch, dict(c, weight=c["weight_old"].copy()), shape, dtype).run(True, per_lane, False, tanh)
        for name in OUTPUTS:
            assert np.array_equal(twin.out(name), ours.out(name), equal_nan=True), name


def test_refusals_on_the_device(torch_mod, crafted):
    shape = SHAPES[1]
    c = crafted[(shape, abi.F64)]
    call = Call(torch_mod, c, shape, abi.F64).run(True, False, False, False, device=1000)
    assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(b"os2ro_ppo_gradient: "), (call.rc, call.error)
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)                        # a refused call wrote nothing
    call = Call(torch_mod, c, shape, abi.F64).run(True, False, False, False, clip=float("nan"))
    assert call.rc == abi.ERR_INVALID and call.error == b"os2ro_ppo_gradient: clip must be finite"
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)


# ---------------------------------------------------------------------------------------
# the real consumer
# ---------------------------------------------------------------------------------------
P_REAL, S_REAL, K_REAL = 4, 8, 12


def _cpu(t):
    return t.detach().cpu().numpy().copy()


@pytest.mark.parametrize("tanh", [False, True])
def test_real_consumer_two_epochs_on_a_noisy_rollout(torch_mod, tanh):
    """A handle of 4 policies x 8 samples, 12 steps: noisy rollout_policy -> gae -> ppo_gradient.  Epoch 1 (weights == weights_old)
    equals policy_gradient(rewards=adv, gamma=0.0) bit for bit; after theta += step grad, epoch 2 equals the restatement fed
    with the device's rho, and on the steps where no clip bound rho is the float64 textbook ratio of the rollout's own actions
    (the pre-squash sample recovered from them) within MARGIN x the distance measured on the GPU: 3.6e-15 over the 39 such steps of the clipped window, 6.1e-14 over the
    146 of the tanh window.
    ppo_gradient_into on the caller's tensors gives the bits of the allocating call."""
    torch = torch_mod
    from gym_os2r_amd.sim import HipSim
    N = P_REAL * S_REAL
    sim = HipSim(make_config("free_hip", "BalancingV2", False, num_envs=N, contact=True, seed=5, auto_reset=True, dtype=abi.F64)[0])
    D, dev = sim.D, sim.device
    rng = np.random.default_rng(17)
    theta = torch.as_tensor(rng.normal(0, 0.3, (2, D + 1, P_REAL))).to(dev).permute(2, 0, 1)       # [P, 2, D+1] over the kernel's layout
    sigma = torch.as_tensor(np.array([0.3, 0.4])).to(dev)
    value_w = torch.as_tensor(rng.normal(0, 0.1, (P_REAL, D + 1))).to(dev)
    per_env = theta[torch.arange(N, device=dev) % P_REAL]                                           # lane s P + p runs policy p
    obs0 = sim.reset()
    ret, length, (O, R, Dn, _, _), (A, E) = sim.rollout_policy(K_REAL, per_env, sigma=sigma, tanh=tanh, salt=3,
                                                                  first_episode=False, want_outputs=True, want_actions=True, want_noise=True)
    adv, _, _ = sim.gae(O, R, Dn, value_w, obs0=obs0, policies=P_REAL, gamma=0.97, lam=0.9)
    common = dict(policies=P_REAL, obs0=obs0, actions=A, tanh=tanh)
    first = sim.ppo_gradient(O, E, sigma, theta, theta, adv, clip=CLIP, want_log_sigma=True, want_lane=True, want_ratio=True, **common)
    score = sim.policy_gradient(O, E, sigma, rewards=adv, done=Dn, gamma=0.0, want_log_sigma=True, want_lane=True, **common)
    torch.cuda.synchronize()
    grad, stats, steps, clipped, gated, valid, lsig, lane, ratio = first
    assert tuple(grad.shape) == (P_REAL, 2, D + 1) and tuple(stats.shape) == (P_REAL, 3) and tuple(ratio.shape) == (K_REAL, N)
    assert grad.permute(1, 2, 0).is_contiguous() and tuple(lane.shape) == (N, 2, D + 1)
    for got, want in ((grad, score[0]), (steps, score[1]), (clipped, score[2]), (valid, score[3]), (lsig, score[4]), (lane, score[5])):
        assert got.shape == want.shape and np.array_equal(_cpu(got).view(np.uint8), _cpu(want).view(np.uint8))
    assert (_cpu(ratio) == 1).all() and (_cpu(gated) == 0).all() and (_cpu(stats)[:, 1:] == 0).all() and (_cpu(valid) == S_REAL).all()
    assert (_cpu(steps) == S_REAL * K_REAL).all() and (_cpu(grad) != 0).all()
    # epoch 2: a step along the gradient
    new = theta + (0.05 / grad.abs().max()) * grad                                                  # the largest weight moves by 0.05
    second = sim.ppo_gradient(O, E, sigma, new, theta, adv, clip=CLIP, want_log_sigma=True, want_lane=True, want_ratio=True, **common)
    torch.cuda.synchronize()
    rho = _cpu(second[8])
    to_kernel = lambda w: _cpu(w.permute(1, 2, 0))
    want = restate_ppo(_cpu(O), _cpu(E), _cpu(sigma), to_kernel(new), to_kernel(theta), _cpu(adv), P=P_REAL, dtype=np.float64, clip=CLIP,
                       obs0=_cpu(obs0), action=None if tanh else _cpu(A), tanh=tanh, ratio=rho)
    for name, got in (("grad", second[0].permute(1, 2, 0)), ("stat", second[1].t()), ("steps", second[2]), ("clipped", second[3].t()),
                      ("gated", second[4]), ("valid", second[5]), ("lsig_grad", second[6].t()), ("lane_grad", second[7].permute(1, 2, 0))):
        assert np.array_equal(_cpu(got), want[name]), name
    assert (rho != 1).any() and (want["valid"] == S_REAL).all() and 0 < want["gated"].sum() < want["steps"].sum()
    # the textbook ratio in float64, from the actions the rollout applied: u = atanh(a), or a itself where the clip did not bind
    a, eps, sg = _cpu(A), _cpu(E), _cpu(sigma)
    prev = np.concatenate([_cpu(obs0)[None], _cpu(O)[:-1]])
    X = np.concatenate([prev, np.ones((K_REAL, N, 1))], 2)
    pol = np.arange(N) % P_REAL
    mu_old = np.einsum("knd,jdn->knj", X, to_kernel(theta)[:, :, pol])
    mu_new = np.einsum("knd,jdn->knj", X, to_kernel(new)[:, :, pol])
    inside = np.abs(a) < 1
    with np.errstate(all="ignore"):
        u = np.arctanh(a) if tanh else a
    free = inside.all(2) & (np.abs(a) < 0.999).all(2)                                              # (atanh loses digits at the ends)
    with np.errstate(all="ignore"):                                                                # (the steps that are not free)
        textbook = np.exp((((u - mu_old) ** 2 - (u - mu_new) ** 2) / (2 * sg ** 2)).sum(2))
    far = float(np.abs(rho[free] / textbook[free] - 1).max())
    # ... and with the pre-squash sample the noise says, the two agree to rounding
    u_eps = mu_old + sg * eps
    assert np.abs(u[free] - u_eps[free]).max() < 1e-9
    print(f"ppo ratio against the textbook ratio of the rollout's actions, tanh={tanh}: {far:.3e} over {int(free.sum())} steps")
    assert free.sum() > 0 and far <= MARGIN * MEASURED_RATIO[tanh]
    # ppo_gradient_into on the caller's tensors
    i32 = torch.int32
    z = lambda *s, dtype=sim.dtype: torch.full(s, -3, dtype=dtype, device=dev)
    g, lg, ls, cnt, st = z(2, D + 1, P_REAL), z(2, D + 1, N), z(3, N), z(5, N, dtype=i32), z(3, P_REAL)
    lsg, lls, stp, clp, gtd, vld, rat = z(2, P_REAL), z(2, N), z(P_REAL, dtype=i32), z(2, P_REAL, dtype=i32), z(P_REAL, dtype=i32), z(P_REAL, dtype=i32), z(K_REAL, N)
    sim.ppo_gradient_into(O, E, sigma, new.permute(1, 2, 0), theta.permute(1, 2, 0), adv, g, lg, ls, cnt, clip=CLIP, lsig_grad=lsg, lane_lsig=lls,
                          stat=st, steps=stp, clipped=clp, gated=gtd, valid=vld, ratio=rat, **common)
    torch.cuda.synchronize()
    for got, ret in ((g.permute(2, 0, 1), second[0]), (st.t(), second[1]), (stp, second[2]), (clp.t(), second[3]), (gtd, second[4]), (vld, second[5]),
                     (lsg.t(), second[6]), (lg.permute(2, 0, 1), second[7]), (rat, second[8])):
        assert got.shape == ret.shape and np.array_equal(_cpu(got).view(np.uint8), _cpu(ret).view(np.uint8))
    assert np.array_equal(_cpu(cnt), want["lane_count"]) and np.array_equal(_cpu(ls), want["lane_stat"])
    sim.close()
