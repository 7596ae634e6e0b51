"""os2rp_pf_update on the device (libos2r_pf.so, include/os2r_pf.h): the weights against numpy's exp of the bit-exact argument,
everything else -- the index and the -inf bit patterns of logw_out included -- bit for bit against the numpy restatement of
tests/test_pf_host.py fed with the device's own weights, the calls with null inputs and without the optional outputs, a refused
call, the index against its real consumer -- copy_envs_from on real handles --, and the example."""
import ctypes

import numpy as np
import pytest

from gym_os2r_amd import abi
from helpers import make_config
from test_pf_host import RATIO, crafted_pf, exp_argument, restate_pf

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
ULPS = 8                                  # what tests/test_gpu_mppi.py allows the same device exp
OUTPUTS = ("logw_out", "index", "est", "weights", "ess", "count", "resampled")
INTS = ("index", "count", "resampled")
# M, S, D: a single lane; a tail lane, S below the chunk count; two workgroups, S the chunk count, the largest D; three
# workgroups with a tail, S no multiple of the chunk count; a full workgroup, S a multiple
GPU_SHAPES = [(1, 1, 1), (63, 3, 10), (65, 8, 12), (130, 19, 10), (64, 64, 5)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _np(dtype):
    return np.float64 if dtype == abi.F64 else np.float32


class Call:
    """One os2rp_pf_update call through ctypes: the inputs of `crafted_pf` on the device, every output between guard bands of PAD
    sentinel elements.  The constructor uploads, run() launches and synchronises."""

    def __init__(self, torch, c, shape, dtype):
        from gym_os2r_amd import pf
        self.torch, self.lib, self.dtype, self.shape = torch, pf.load(), dtype, shape
        M, S, D = shape
        dt = _np(dtype)
        self.dev = torch.device("cuda:0")
        put = lambda x: torch.as_tensor(np.ascontiguousarray(np.asarray(x).astype(dt))).to(self.dev)
        self.inputs = {k: put(c[k]) for k in ("obs", "meas", "prec", "logw", "u")}
        self.sizes = dict(logw_out=S * M, index=S * M, est=M * D, weights=S * M, ess=M, count=M, resampled=M)
        self.bufs = {}
        for name, size in self.sizes.items():
            if name in INTS:
                self.bufs[name] = torch.full((PAD + size + PAD,), IMARK, dtype=torch.int32, device=self.dev)
            else:
                self.bufs[name] = torch.full((PAD + size + PAD,), MARK, dtype=self.inputs["obs"].dtype, device=self.dev)

    def run(self, ratio=RATIO, leave_out=(), null=(), device=0):
        from gym_os2r_amd import control
        M, S, D = self.shape
        lay = control.layout(self.dtype, 3, device, [-1] * D)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        ins = [None if name in null else p(self.inputs[name]) for name in ("obs", "meas", "prec", "logw", "u")]
        outs = [None if name in leave_out else p(self.bufs[name][PAD:]) for name in OUTPUTS]
        self.rc = self.lib.os2rp_pf_update(ctypes.byref(lay), M, S, *ins, ratio, *outs, None)
        self.error = self.lib.os2rp_last_error()
        self.torch.cuda.synchronize()
        self.left_out = leave_out
        return self

    def out(self, name):
        """-> the array the call wrote, after a look at its guard bands (and, if it was left out, at all of it)"""
        M, S, D = self.shape
        host = self.bufs[name].cpu().numpy()
        mark = IMARK if name in INTS else MARK
        assert (host[:PAD] == mark).all() and (host[PAD + self.sizes[name]:] == mark).all(), f"{name}: written outside"
        inner = host[PAD:PAD + self.sizes[name]]
        if name in self.left_out:
            assert (inner == mark).all(), f"{name}: written although left out"
            return None
        shapes = dict(logw_out=(S, M), index=(S * M,), est=(M, D), weights=(S, M), ess=(M,), count=(M,), resampled=(M,))
        return inner.reshape(shapes[name])

    def check(self, c, what, ratio=RATIO, null=()):
        """Everything but the weights against the restatement on the device's own weights, bit for bit; -> the weights"""
        M, S, D = self.shape
        assert self.rc == abi.OK, (what, self.rc, self.error)
        w = self.out("weights")
        want = restate_pf(c["obs"], c["meas"], c["prec"], None if "logw" in null else c["logw"], None if "u" in null else c["u"], S=S,
                          ratio=ratio, dtype=_np(self.dtype), weights=w)
        bits = np.uint64 if self.dtype == abi.F64 else np.uint32
        for name in OUTPUTS:
            got = self.out(name)
            if name in INTS:
                assert got.dtype == np.int32 and np.array_equal(got, want[name]), (what, name, np.argwhere(got != want[name])[:4])
                continue
            assert got.dtype == want[name].dtype, (what, name)
            # the sign of a zero is not part of the contract: +0 and -0 compare as one bit pattern, everything else (NaN of est
            # where the measurement of a lost robot holds one, -inf of logw_out) as its own
            g, e = np.where(got == 0, 0, got).view(bits), np.where(want[name] == 0, 0, want[name]).view(bits)
            if name == "est":
                nan = np.isnan(want[name])
                assert np.array_equal(np.isnan(got), nan), (what, name)
                g, e = g[~nan], e[~nan]
            assert np.array_equal(g, e), (what, name, np.argwhere(g != e)[:4])
        return w


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_weights_within_8_ulp_of_numpy_and_the_rest_bit_for_bit(torch_mod, shape, dtype):
    """The device's weights against numpy's exp of the bit-exact argument: within 8 ulp, exactly 0 on invalid particles and exactly
    1 at the maximum.  With the device's own weights fed to the restatement, logw_out (with its -inf bit patterns), index, est,
    ess, count and resampled are equal to it, and no guard band is touched."""
    M, S, D = shape
    dt = _np(dtype)
    c = crafted_pf(M, S, D, dtype=dt)
    w = Call(torch_mod, c, shape, dtype).run().check(c, f"{shape} {dtype}")
    valid, count, arg = exp_argument(c["obs"], c["meas"], c["prec"], c["logw"], S, dt)
    assert w.dtype == dt and (w[~valid] == 0).all() and (w[valid & (arg == 0)] == 1).all()
    assert ((arg == 0) & valid).any(0)[count > 0].all()
    ref = np.exp(arg.astype(np.float64))                                          # numpy's exp, in double for both dtypes
    ulp = np.spacing(np.maximum(ref, np.finfo(dt).tiny).astype(dt)).astype(np.float64)
    err = np.where(valid, np.abs(w.astype(np.float64) - ref) / ulp, 0)
    print(f"pf weights {shape} {dt.__name__}: worst {err.max():.3f} ulp over {int(valid.sum())} valid particles")
    assert err.max() <= ULPS, (shape, dtype, err.max())
    if S > 1 and M > 8:
        far = valid & (arg < -1e5)
        assert far.any() and (w[far] == 0).all()                                   # the distance that underflows


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("ratio", [0.0, 2.0])
def test_resampling_no_robot_for_its_weights_and_every_robot(torch_mod, ratio, dtype):
    """resample_ratio = 0: only the robots with an invalid particle resample; 2: every robot with a valid particle does."""
    shape = GPU_SHAPES[3]
    M, S, D = shape
    c = crafted_pf(M, S, D, dtype=_np(dtype))
    call = Call(torch_mod, c, shape, dtype).run(ratio=ratio)
    call.check(c, f"ratio {ratio} {dtype}", ratio=ratio)
    count, res = call.out("count"), call.out("resampled")
    assert np.array_equal(res == 1, (count > 0) & (count < S) if ratio == 0 else count > 0)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_null_inputs_and_a_call_without_the_optional_outputs(torch_mod, dtype):
    """Null u_dev (0.5 for every robot) and null logw_in_dev (zeros) against the restatement; without any of the optional outputs
    logw_out and index are the same bits, and what is left out is not written."""
    shape = GPU_SHAPES[3]
    M, S, D = shape
    c = crafted_pf(M, S, D, dtype=_np(dtype))
    for null in (("u",), ("logw",), ("logw", "u")):
        Call(torch_mod, c, shape, dtype).run(null=null).check(c, f"null {null} {dtype}", null=null)
    whole = Call(torch_mod, c, shape, dtype).run()
    whole.check(c, "whole")
    for leave_out in (OUTPUTS[2:], ("est",), ("weights", "ess"), ("count", "resampled")):
        part = Call(torch_mod, c, shape, dtype).run(leave_out=leave_out)
        assert part.rc == abi.OK, part.error
        for name in OUTPUTS:
            if name in leave_out:
                assert part.out(name) is None
            else:
                assert np.array_equal(part.out(name).view(np.uint8), whole.out(name).view(np.uint8)), (leave_out, name)


def test_a_refused_call_writes_nothing(torch_mod):
    shape = GPU_SHAPES[1]
    c = crafted_pf(*shape)
    call = Call(torch_mod, c, shape, abi.F64).run(ratio=float("nan"))
    assert call.rc == abi.ERR_INVALID and call.error == b"os2rp_pf_update: resample_ratio must be finite"
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)
    call = Call(torch_mod, c, shape, abi.F64).run(device=1000)
    assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(b"os2rp_pf_update: "), (call.rc, call.error)
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)


STATE_KEYS = ("q", "qd", "solver_lambda", "solver_flags", "hist0", "hist1", "steps", "episode", "pose")


def test_on_real_handles_the_index_drives_copy_envs_from(torch_mod):
    """M = 3 robots, S = 8 particles, fp64 free_hip with contact: five steps with process noise, pf_update with resample_ratio = 1
    (robot 2's measurement is NaN: it is lost and keeps its lanes), copy_envs_from(self, index).  Every lane with an ancestor
    holds its pre-copy state, solver state and parameters bit for bit, every lane with -1 is unchanged; a second pf_update on the
    copied lanes' observations with null logw counts S valid particles for every robot."""
    torch = torch_mod
    from gym_os2r_amd.sim import HipSim
    M, S = 3, 8
    N = S * M

    def make(num, auto_reset):
        cfg = make_config("free_hip", "BalancingV2", False, num_envs=num, contact=True, seed=5, auto_reset=auto_reset, dtype=abi.F64)[0]
        return HipSim(cfg)
    real, particles = make(M, True), make(N, False)
    D, dev = real.D, real.device
    cpu = lambda t: t.detach().cpu().numpy().copy()
    lane_robot = torch.arange(N, device=dev) % M
    particles.copy_envs_from(real, lane_robot.to(torch.int32))
    rng = np.random.default_rng(3)
    weights = torch.zeros(N, 2, D + 1, dtype=torch.float64, device=dev)
    for k in range(5):
        action = torch.as_tensor(rng.uniform(-0.5, 0.5, (M, 2))).to(dev)
        obs_real = real.step(action)[0]
        weights[:, :, D] = action[lane_robot]
        obs = particles.rollout_policy(1, weights, sigma=0.3, want_outputs=True)[2][0][0]
    torch.cuda.synchronize()
    assert tuple(obs.shape) == (N, D) and np.isfinite(cpu(obs)).all() and len(np.unique(cpu(obs)[:, 0])) > M     # the particles differ
    sigma = 0.05
    prec = torch.full((D,), 1.0 / sigma ** 2, dtype=torch.float64, device=dev)
    meas = obs_real + sigma * torch.as_tensor(rng.normal(0, 1, (M, D))).to(dev)
    meas[2] = float("nan")
    u = torch.as_tensor(rng.uniform(0, 1, M)).to(dev)
    logw, index, est, w, ess, count, resampled = particles.pf_update(obs, meas, prec, particles=S, u=u, resample_ratio=1.0, want_weights=True)
    torch.cuda.synchronize()
    want = restate_pf(cpu(obs), cpu(meas), cpu(prec), None, cpu(u), S=S, ratio=1.0, dtype=np.float64, weights=cpu(w))
    for name, got in (("logw_out", logw), ("index", index), ("ess", ess), ("count", count), ("resampled", resampled)):
        assert np.array_equal(cpu(got), want[name]), name
    assert np.array_equal(cpu(est)[:2], want["est"][:2]) and np.isnan(cpu(est)[2]).all()
    assert cpu(count).tolist() == [S, S, 0] and cpu(resampled).tolist() == [1, 1, 0] and (cpu(logw) == 0).all()
    idx = cpu(index)
    assert (idx.reshape(S, M)[:, 2] == -1).all() and (idx.reshape(S, M)[:, :2] >= 0).all() and (idx[idx >= 0] % M == np.arange(N)[idx >= 0] % M).all()
    before = particles.checkpoint()
    obs2 = particles.copy_envs_from(particles, index, want_obs=True)
    after = particles.checkpoint()
    torch.cuda.synchronize()
    src = torch.where(index >= 0, index, torch.arange(N, device=dev, dtype=torch.int32)).long()
    for key in STATE_KEYS:
        assert torch.equal(after[key], before[key].index_select(-1, src)), key
    for field, values in before["params"].items():
        assert torch.equal(after["params"][field], values.index_select(-1, src)), field
    assert torch.equal(obs2, obs.index_select(0, src))
    again = particles.pf_update(obs2, obs_real, prec, particles=S, resample_ratio=1.0)
    torch.cuda.synchronize()
    assert cpu(again[5]).tolist() == [S, S, S] and np.isfinite(cpu(again[2])).all() and np.isfinite(cpu(again[0])).all()
    third = particles.pf_update(obs2, obs_real, prec, particles=S, logw=again[0], resample_ratio=0.0)       # fed back: the other buffer
    torch.cuda.synchronize()
    assert third[0].data_ptr() != again[0].data_ptr() and cpu(third[6]).tolist() == [0, 0, 0] and (cpu(third[1]) == -1).all()
    real.close()
    particles.close()


def test_example_tracks_three_robots(torch_mod):
    """examples/pf_tracking.py runs to its end for three robots in a fresh child process."""
    import os
    import re
    import subprocess
    import sys
    from conftest import ROOT
    script = os.path.join(ROOT, "examples", "pf_tracking.py")
    out = subprocess.run([sys.executable, script, "--robots", "3", "--particles", "16", "--steps", "5"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "3 robots x 16 particles, 5 control steps" in out.stdout and re.search(r"^control step 5: rms error of the estimate [0-9.]+", out.stdout, re.M)
    assert re.search(r"^rms error [0-9.]+ against a measurement noise of [0-9.]+ over 5 control steps of 3 robots; \d+ resamplings", out.stdout, re.M)
