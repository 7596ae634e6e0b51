"""os2re_ekf_update on the device (libos2r_ekf.so, include/os2r_ekf.h): every output bit for bit against the numpy restatement of
tests/test_ekf_host.py on its crafted inputs, the call without a_dev, without a gate, without the optional outputs and with the
outputs in the inputs' place, a refused call, the update on real handles between linearize and set_state, and the example."""
import ctypes

import numpy as np
import pytest

from gym_os2r_amd import abi
from helpers import make_config
from test_ekf_host import GATE, ROBOTS, crafted_ekf, restate_ekf, same_bits

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
OUTPUTS = ("x", "p", "nis", "used", "refused", "innov")
INTS = ("used", "refused")
# M, nq, D: a single lane; one robot below and one above the 32 of a workgroup, the largest D; two workgroups with a tail; full
# workgroups
GPU_SHAPES = [(1, 2, 1), (31, 3, 6), (33, 5, 12), (65, 4, 8), (64, 5, 10)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _np(dtype):
    return np.float64 if dtype == abi.F64 else np.float32


_crafted = {}


def crafted(shape, dtype):
    """crafted_ekf and its restatements, made once per shape and dtype and left unchanged."""
    key = (shape, dtype)
    if key not in _crafted:
        _crafted[key] = (crafted_ekf(*shape, dtype=_np(dtype)), {})
    return _crafted[key]


def wanted(shape, dtype, gate=GATE, predict=True):
    c, done = crafted(shape, dtype)
    if (gate, predict) not in done:
        done[(gate, predict)] = restate_ekf(c["x_pred"], c["p_in"], c["meas"], c["prec"], c["slot_col"], a=c["a"] if predict else None,
                                            q=c["q"] if predict else None, gate=gate, dtype=_np(dtype))
    return done[(gate, predict)]


class Call:
    """One os2re_ekf_update call through ctypes: the inputs of `crafted_ekf` on the device, every output between guard bands of PAD
    sentinel elements.  The constructor uploads, run() launches and synchronises."""

    def __init__(self, torch, c, shape, dtype):
        from gym_os2r_amd import ekf
        self.torch, self.lib, self.dtype, self.shape, self.c = torch, ekf.load(), dtype, shape, c
        M, nq, D = shape
        n = 2 * nq
        dt = _np(dtype)
        self.dev = torch.device("cuda:0")
        put = lambda x: torch.as_tensor(np.ascontiguousarray(np.asarray(x).astype(dt))).to(self.dev)
        self.inputs = {k: put(c[k]) for k in ("x_pred", "p_in", "a", "meas", "prec")}
        self.q = (ctypes.c_double * (n * n))(*np.asarray(c["q"]).reshape(-1).tolist())
        self.sizes = dict(x=n * M, p=n * n * M, nis=M, used=M, refused=M, innov=M * D)
        self.shapes = dict(x=(n, M), p=(n, n, M), nis=(M,), used=(M,), refused=(M,), innov=(M, D))
        self.bufs = {}
        for name, size in self.sizes.items():
            if name in INTS:
                self.bufs[name] = torch.full((PAD + size + PAD,), IMARK, dtype=torch.int32, device=self.dev)
            else:
                self.bufs[name] = torch.full((PAD + size + PAD,), MARK, dtype=self.inputs["meas"].dtype, device=self.dev)

    def run(self, gate=GATE, predict=True, leave_out=(), in_place=False, device=0):
        """in_place: x_pred and p_in are copied into the output buffers and read there, x_out = x_pred and p_out = p_in"""
        from gym_os2r_amd import control
        M, nq, D = self.shape
        lay = control.layout(self.dtype, nq, device, self.c["slot_col"])
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        outs = [None if name in leave_out else p(self.bufs[name][PAD:]) for name in OUTPUTS]
        xin, pin = p(self.inputs["x_pred"]), p(self.inputs["p_in"])
        if in_place:
            self.bufs["x"][PAD:PAD + self.sizes["x"]] = self.inputs["x_pred"].reshape(-1)
            self.bufs["p"][PAD:PAD + self.sizes["p"]] = self.inputs["p_in"].reshape(-1)
            xin, pin = outs[0], outs[1]
        self.rc = self.lib.os2re_ekf_update(ctypes.byref(lay), M, xin, pin, p(self.inputs["a"]) if predict else None,
                                            self.q if predict else None, p(self.inputs["meas"]), p(self.inputs["prec"]), gate, *outs, None)
        self.error = self.lib.os2re_last_error()
        self.torch.cuda.synchronize()
        self.left_out = leave_out
        return self

    def out(self, name):
        """-> the array the call wrote, after a look at its guard bands (and, if it was left out, at all of it)"""
        host = self.bufs[name].cpu().numpy()
        mark = IMARK if name in INTS else MARK
        assert (host[:PAD] == mark).all() and (host[PAD + self.sizes[name]:] == mark).all(), f"{name}: written outside"
        inner = host[PAD:PAD + self.sizes[name]]
        if name in self.left_out:
            assert (inner == mark).all(), f"{name}: written although left out"
            return None
        return inner.reshape(self.shapes[name])

    def check(self, want, what):
        """Every output against the restatement: the floats by bit pattern (+0 and -0 as one, a NaN as a NaN), the ints exactly"""
        assert self.rc == abi.OK, (what, self.rc, self.error)
        for name in OUTPUTS:
            got = self.out(name)
            if got is None:
                continue
            if name in INTS:
                assert got.dtype == np.int32 and np.array_equal(got, want[name]), (what, name, np.argwhere(got != want[name])[:4])
            else:
                assert same_bits(got, want[name]), (what, name, np.argwhere(~((got == want[name]) | (np.isnan(got) & np.isnan(want[name]))))[:4])
        return self


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_every_output_bit_for_bit_against_the_restatement(torch_mod, shape, dtype):
    """crafted_ekf inputs, gate 9, with the covariance prediction: x_out, p_out, nis, used, refused and innov are equal to the
    restatement, and no guard band is touched."""
    M, nq, D = shape
    assert ROBOTS == 32                                               # the M of GPU_SHAPES lie about the robots of a workgroup
    c, _ = crafted(shape, dtype)
    call = Call(torch_mod, c, shape, dtype).run().check(wanted(shape, dtype), f"{shape} {dtype}")
    if M >= 8:
        used, refused = call.out("used"), call.out("refused")
        assert used.any() and refused.any() and (used & refused == 0).all()


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_without_a_dev_without_a_gate_without_outputs_and_in_place(torch_mod, dtype):
    """On one shape: a_dev null (the measurement update only), gate 0, the optional outputs left out in groups -- what is left out
    is not written and the rest has the same bits --, and x_out = x_pred with p_out = p_in as the same pointers, which gives the
    bits of the call with separate arrays."""
    shape = GPU_SHAPES[3]
    c, _ = crafted(shape, dtype)
    Call(torch_mod, c, shape, dtype).run(predict=False).check(wanted(shape, dtype, predict=False), "a_dev null")
    Call(torch_mod, c, shape, dtype).run(gate=0.0).check(wanted(shape, dtype, gate=0.0), "gate 0")
    Call(torch_mod, c, shape, dtype).run(gate=0.0, predict=False).check(wanted(shape, dtype, gate=0.0, predict=False), "gate 0, a_dev null")
    whole = Call(torch_mod, c, shape, dtype).run().check(wanted(shape, dtype), "whole")
    for leave_out in (OUTPUTS[2:], ("nis",), ("used", "refused"), ("innov",), ("nis", "innov")):
        part = Call(torch_mod, c, shape, dtype).run(leave_out=leave_out)
        assert part.rc == abi.OK, part.error
        for name in OUTPUTS:
            if name in leave_out:
                assert part.out(name) is None
            else:
                assert np.array_equal(part.out(name).view(np.uint8), whole.out(name).view(np.uint8)), (leave_out, name)
    for predict in (True, False):
        apart = Call(torch_mod, c, shape, dtype).run(predict=predict)
        same = Call(torch_mod, c, shape, dtype).run(predict=predict, in_place=True).check(wanted(shape, dtype, predict=predict), "in place")
        for name in OUTPUTS:
            assert np.array_equal(same.out(name).view(np.uint8), apart.out(name).view(np.uint8)), (predict, name)


def test_a_refused_call_writes_nothing(torch_mod):
    shape = GPU_SHAPES[1]
    c, _ = crafted(shape, abi.F64)
    call = Call(torch_mod, c, shape, abi.F64).run(gate=float("nan"))
    assert call.rc == abi.ERR_INVALID and call.error == b"os2re_ekf_update: gate must be finite"
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)
    call = Call(torch_mod, c, shape, abi.F64).run(device=1000)
    assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(b"os2re_ekf_update: "), (call.rc, call.error)
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)


def test_on_real_handles_between_linearize_and_set_state(torch_mod):
    """M = 3 robots, fp64 free_hip with contact, the non-normalised task: a few steps of a real handle, linearize on the estimate
    handle, ekf_update fed with those very tensors (robot 2's measurement is all NaN).  The outputs equal the restatement fed
    with the tensors' host copies, bit for bit; robot 2's state is `next`; set_state takes the two halves, and get_state returns
    their bits."""
    torch = torch_mod
    from gym_os2r_amd.sim import HipSim
    M = 3

    def make(seed, auto_reset):
        cfg = make_config("free_hip", "BalancingV2", False, num_envs=M, contact=True, seed=seed, auto_reset=auto_reset, dtype=abi.F64)[0]
        return HipSim(cfg)
    real, est = make(5, True), make(5, False)
    nq, D, dev = real.nq, real.D, real.device
    n = 2 * nq
    cpu = lambda t: t.detach().cpu().numpy().copy()
    cols = [int(v) for v in est._layout().slot_col[:D]]
    assert any(v >= 0 for v in cols)
    rng = np.random.default_rng(3)
    q, qd = est.get_state()
    est.set_state(q + 0.01 * torch.as_tensor(rng.normal(0, 1, (nq, M))).to(dev), qd)
    P = (0.01 * torch.eye(n, dtype=torch.float64, device=dev)).repeat(M, 1, 1)
    Q = 1e-4 * torch.eye(n, dtype=torch.float64)
    sigma = 0.02
    prec = torch.full((D,), 1.0 / sigma ** 2, dtype=torch.float64, device=dev)
    for k in range(4):
        action = torch.as_tensor(rng.uniform(-0.3, 0.3, (M, 2))).to(dev)
        obs = real.step(action)[0]
        meas = obs + sigma * torch.as_tensor(rng.normal(0, 1, (M, D))).to(dev)
        meas[2] = float("nan")
        nxt_q, nxt_qd, A, _ = est.linearize(action, want_B=False)
        x, P_new, nis, used, refused, innov = est.ekf_update((nxt_q, nxt_qd), P, meas, prec, A=A, Q=Q, gate=0.0, want_innov=True)
        torch.cuda.synchronize()
        x_pred = np.concatenate([cpu(nxt_q), cpu(nxt_qd)])
        want = restate_ekf(x_pred, cpu(P).transpose(1, 2, 0), cpu(meas), cpu(prec), cols, a=cpu(A).transpose(1, 2, 0), q=Q.numpy(),
                           gate=0.0, dtype=np.float64)
        assert same_bits(cpu(x), want["x"]) and same_bits(cpu(P_new).transpose(1, 2, 0), want["p"]) and same_bits(cpu(nis), want["nis"])
        assert np.array_equal(cpu(used), want["used"]) and np.array_equal(cpu(refused), want["refused"]) and same_bits(cpu(innov), want["innov"])
        assert same_bits(cpu(x)[:, 2], x_pred[:, 2]) and cpu(used)[2] == 0 and cpu(used)[0] != 0 and (cpu(refused) == 0).all()
        if k:
            assert P_new.data_ptr() != P.data_ptr()                   # the two kept buffers alternate
        est.set_state(x[:nq], x[nq:])
        q, qd = est.get_state()
        torch.cuda.synchronize()
        assert same_bits(cpu(q), cpu(x)[:nq]) and same_bits(cpu(qd), cpu(x)[nq:])
        P = P_new
    real.close()
    est.close()


def test_example_tracks_three_robots(torch_mod):
    """examples/ekf_tracking.py runs to its end for three robots in a fresh child process."""
    import os
    import re
    import subprocess
    import sys
    from conftest import ROOT
    script = os.path.join(ROOT, "examples", "ekf_tracking.py")
    out = subprocess.run([sys.executable, script, "--robots", "3", "--steps", "5"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "3 robots, 5 control steps" in out.stdout and re.search(r"^control step 5: rms error of the estimate [0-9.e-]+", out.stdout, re.M)
    assert re.search(r"^rms error [0-9.e-]+ against a measurement noise of [0-9.e-]+ over 5 control steps of 3 robots; \d+ slots gated, "
                     r"\d+ refused", out.stdout, re.M)
