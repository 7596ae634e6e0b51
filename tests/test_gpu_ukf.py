"""os2ru_ukf_points and os2ru_ukf_update on the device (libos2r_ukf.so, include/os2r_ukf.h): every output bit for bit against the
numpy restatements of tests/test_ukf_host.py on its crafted inputs, the square root on its own, the calls with fewer outputs and
with p_out in p_in's place, refused calls, step 4 of the update against a separate points launch, one filter step on real
handles between set_state and get_state, and the example."""
import ctypes

import numpy as np
import pytest

from gym_os2r_amd import abi
from helpers import make_config
from test_ekf_host import GATE, ROBOTS, same_bits
from test_ukf_host import crafted_ukf, restate_ukf_points, restate_ukf_update, restated_update

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
POINT_OUTPUTS = ("points", "failed")
UPDATE_OUTPUTS = ("x", "p", "nis", "used", "refused", "innov", "lost", "points", "failed")
INTS = ("used", "refused", "lost", "failed")
D = 10
# M, nq: a single robot of the smallest chain; one robot below and one above the 32 of a workgroup; three workgroups with a tail,
# the largest chain; full workgroups
GPU_SHAPES = [(1, 2), (31, 3), (33, 5), (70, 5), (64, 4)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _np(dtype):
    return np.float64 if dtype == abi.F64 else np.float32


_crafted = {}


def crafted(shape, dtype, variant=0):
    """crafted_ukf and its restatements, made once per shape, dtype and variant and left unchanged."""
    key = (shape, dtype, variant)
    if key not in _crafted:
        _crafted[key] = (crafted_ukf(shape[0], shape[1], D, dtype=_np(dtype), variant=variant), {})
    return _crafted[key]


def wanted(shape, dtype, variant=0, **kw):
    c, made = crafted(shape, dtype, variant)
    key = tuple(sorted(kw.items()))
    if key not in made:
        made[key] = restated_update(c, _np(dtype), **kw)
    return made[key]


def wanted_points(shape, dtype, variant=0):
    c, made = crafted(shape, dtype, variant)
    if "points" not in made:
        made["points"] = restate_ukf_points(c["x"], c["p"], c["scalars"][0], dtype=_np(dtype))
    return made["points"]


class Call:
    """One call of either entry point through ctypes: the inputs of `crafted_ukf` on the device, every output between guard bands
    of PAD sentinel elements.  The constructor uploads, points() / update() launch and synchronise."""

    def __init__(self, torch, c, shape, dtype):
        from gym_os2r_amd import ukf
        self.torch, self.lib, self.dtype, self.shape, self.c = torch, ukf.load(), dtype, shape, c
        M, nq = shape
        n = 2 * nq
        S = 2 * n + 1
        dt = _np(dtype)
        self.dev = torch.device("cuda:0")
        put = lambda x: torch.as_tensor(np.ascontiguousarray(np.asarray(x).astype(dt))).to(self.dev)
        self.inputs = {k: put(c[k]) for k in ("x", "p", "q", "qd", "p_in", "meas", "prec")}
        self.inputs["done"] = torch.as_tensor(np.asarray(c["done"], np.uint8)).to(self.dev)
        self.q_noise = (ctypes.c_double * (n * n))(*np.asarray(c["q_noise"]).reshape(-1).tolist())
        self.sizes = dict(x=n * M, p=n * n * M, nis=M, used=M, refused=M, innov=M * D, lost=M, points=n * S * M, failed=M)
        self.shapes = dict(x=(n, M), p=(n, n, M), nis=(M,), used=(M,), refused=(M,), innov=(M, D), lost=(M,), points=(n, S * M), failed=(M,))
        self.bufs = {}
        for name, size in self.sizes.items():
            if name in INTS:
                self.bufs[name] = torch.full((PAD + size + PAD,), IMARK, dtype=torch.int32, device=self.dev)
            else:
                self.bufs[name] = torch.full((PAD + size + PAD,), MARK, dtype=self.inputs["meas"].dtype, device=self.dev)
        self.left_out = ()

    def _ptr(self, t):
        return ctypes.c_void_p(t.data_ptr())

    def _outs(self, names, leave_out):
        self.left_out = tuple(leave_out) + tuple(k for k in self.bufs if k not in names)
        return [None if name in leave_out else self._ptr(self.bufs[name][PAD:]) for name in names]

    def _layout(self, device):
        from gym_os2r_amd import control
        return control.layout(self.dtype, self.shape[1], device, self.c["slot_col"])

    def points(self, leave_out=(), device=0, gamma=None, x=None, p=None):
        lay = self._layout(device)
        outs = self._outs(POINT_OUTPUTS, leave_out)
        self.rc = self.lib.os2ru_ukf_points(ctypes.byref(lay), self.shape[0], self._ptr(self.inputs["x"] if x is None else x),
                                            self._ptr(self.inputs["p"] if p is None else p), self.c["scalars"][0] if gamma is None else gamma,
                                            *outs, None)
        self.error = self.lib.os2ru_last_error()
        self.torch.cuda.synchronize()
        return self

    def update(self, gate=GATE, done=True, leave_out=(), in_place=False, device=0, scalars=None):
        """in_place: p_in is copied into the output buffer and read there, p_out = p_in"""
        lay = self._layout(device)
        outs = self._outs(UPDATE_OUTPUTS, leave_out)
        pin = self._ptr(self.inputs["p_in"])
        if in_place:
            self.bufs["p"][PAD:PAD + self.sizes["p"]] = self.inputs["p_in"].reshape(-1)
            pin = outs[1]
        self.rc = self.lib.os2ru_ukf_update(ctypes.byref(lay), self.shape[0], self._ptr(self.inputs["q"]), self._ptr(self.inputs["qd"]),
                                            self._ptr(self.inputs["done"]) if done else None, pin, self.q_noise,
                                            *(self.c["scalars"] if scalars is None else scalars), self._ptr(self.inputs["meas"]),
                                            self._ptr(self.inputs["prec"]), gate, *outs, None)
        self.error = self.lib.os2ru_last_error()
        self.torch.cuda.synchronize()
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

    def nothing_written(self):
        self.left_out = tuple(self.bufs)
        return all(self.out(name) is None for name in self.bufs)

    def check(self, want, what):
        """Every output against the restatement: the floats by bit pattern (+0 and -0 as one, a NaN as a NaN), the ints exactly"""
        assert self.rc == abi.OK, (what, self.rc, self.error)
        for name in self.bufs:
            got = self.out(name)
            if got is None:
                continue
            if name in INTS:
                assert got.dtype == np.int32 and np.array_equal(got, want[name]), (what, name, np.argwhere(got != want[name])[:4])
            else:
                assert same_bits(got, want[name]), (what, name, np.argwhere(~((got == want[name]) | (np.isnan(got) & np.isnan(want[name]))))[:4])
        return self


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_every_output_bit_for_bit_against_the_restatement(torch_mod, shape, dtype, variant):
    """crafted_ukf inputs: the points and failed of os2ru_ukf_points, and x_out, p_out, nis, used, refused, innov, lost, the points
    and failed of os2ru_ukf_update at gate 9 with the done flags, are equal to the restatements, and no guard band is touched."""
    M, nq = shape
    assert ROBOTS == 32                                               # the M of GPU_SHAPES lie about the robots of a workgroup
    c, _ = crafted(shape, dtype, variant)
    what = f"{shape} {dtype} variant {variant}"
    call = Call(torch_mod, c, shape, dtype).points().check(wanted_points(shape, dtype, variant), "points " + what)
    if M >= 6:
        assert len(set(call.out("failed").tolist())) == 5             # 0 and the four failing columns
    call = Call(torch_mod, c, shape, dtype).update().check(wanted(shape, dtype, variant), "update " + what)
    if M >= 8:
        used, refused = call.out("used"), call.out("refused")
        assert used.any() and refused.any() and (used & refused == 0).all() and call.out("lost").sum() == sum(m % 8 in (1, 2, 3) for m in range(M))
        assert call.out("failed").any()


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_the_square_root_is_correctly_rounded(torch_mod, dtype):
    """A diagonal P: L[j][j] = sqrt(P[j][j]) and nothing else, so chi_{1+j}[j] - x_j with x = 0 and gamma = 1 is the device's square
    root of 2 n M values spread over the dtype's normal range, against numpy's, bit for bit."""
    M, nq = 257, 5
    n = 2 * nq
    dt = _np(dtype)
    rng = np.random.default_rng(11)
    lo, hi = (-1000, 1000) if dtype == abi.F64 else (-120, 120)
    diag = (rng.uniform(1.0, 4.0, (n, M)) * 2.0 ** rng.integers(lo, hi, (n, M))).astype(dt)
    p = np.zeros((n, n, M), dt)
    for j in range(n):
        p[j, j] = diag[j]
    c = dict(crafted(GPU_SHAPES[3], dtype)[0], slot_col=[0] * D)
    torch = torch_mod
    call = Call(torch, c, (M, nq), dtype)
    x = torch.zeros(n, M, dtype=call.inputs["meas"].dtype, device=call.dev)
    call.points(gamma=1.0, x=x, p=torch.as_tensor(p).to(call.dev))
    assert call.rc == abi.OK, call.error
    cube = call.out("points").reshape(n, 2 * n + 1, M)
    assert (call.out("failed") == 0).all()
    for j in range(n):
        assert np.array_equal(cube[j, 1 + j].view(np.uint8), np.sqrt(diag[j]).view(np.uint8)), j
        assert np.array_equal(cube[j, 1 + n + j], -np.sqrt(diag[j])), j


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_fewer_outputs_no_done_no_gate_and_in_place(torch_mod, dtype):
    """On one shape: done_dev null, gate 0, the optional outputs left out in groups -- what is left out is not written and the rest
    has the same bits --, every nullable output null, and p_out = p_in as the same pointer, which gives the bits of the call
    with separate arrays."""
    shape = GPU_SHAPES[3]
    c, _ = crafted(shape, dtype)
    Call(torch_mod, c, shape, dtype).update(done=False).check(wanted(shape, dtype, done=False), "done_dev null")
    Call(torch_mod, c, shape, dtype).update(gate=0.0).check(wanted(shape, dtype, gate=0.0), "gate 0")
    whole = Call(torch_mod, c, shape, dtype).update().check(wanted(shape, dtype), "whole")
    for leave_out in (UPDATE_OUTPUTS[2:], ("points", "failed"), ("failed",), ("nis",), ("used", "refused", "lost"), ("innov",), ("lost", "innov", "failed")):
        part = Call(torch_mod, c, shape, dtype).update(leave_out=leave_out)
        assert part.rc == abi.OK, part.error
        for name in UPDATE_OUTPUTS:
            if name in leave_out:
                assert part.out(name) is None
            else:
                assert np.array_equal(part.out(name).view(np.uint8), whole.out(name).view(np.uint8)), (leave_out, name)
    same = Call(torch_mod, c, shape, dtype).update(in_place=True).check(wanted(shape, dtype), "in place")
    for name in UPDATE_OUTPUTS:
        assert np.array_equal(same.out(name).view(np.uint8), whole.out(name).view(np.uint8)), name
    whole = Call(torch_mod, c, shape, dtype).points().check(wanted_points(shape, dtype), "points")
    part = Call(torch_mod, c, shape, dtype).points(leave_out=("failed",))
    assert part.rc == abi.OK and part.out("failed") is None
    assert np.array_equal(part.out("points").view(np.uint8), whole.out("points").view(np.uint8))


def test_a_refused_call_writes_nothing(torch_mod):
    shape = GPU_SHAPES[1]
    c, _ = crafted(shape, abi.F64)
    call = Call(torch_mod, c, shape, abi.F64).update(gate=float("nan"))
    assert call.rc == abi.ERR_INVALID and call.error == b"os2ru_ukf_update: gate must be finite" and call.nothing_written()
    call = Call(torch_mod, c, shape, abi.F64).update(scalars=(2.0, 0.0, 2.0, -0.1))
    assert call.rc == abi.ERR_INVALID and call.error == b"os2ru_ukf_update: wi must be > 0" and call.nothing_written()
    call = Call(torch_mod, c, shape, abi.F64).update(device=1000)
    assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(b"os2ru_ukf_update: ") and call.nothing_written(), (call.rc, call.error)
    call = Call(torch_mod, c, shape, abi.F64).points(gamma=0.0)
    assert call.rc == abi.ERR_INVALID and call.error == b"os2ru_ukf_points: gamma must be > 0" and call.nothing_written()
    call = Call(torch_mod, c, shape, abi.F64).points(device=1000)
    assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(b"os2ru_ukf_points: ") and call.nothing_written(), (call.rc, call.error)


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_step_4_is_a_points_launch_on_the_outputs(torch_mod, dtype):
    """os2ru_ukf_update(..., points_out, failed) against os2ru_ukf_points on the x_out and p_out it wrote, on the device: bit for bit."""
    shape = GPU_SHAPES[3]
    c, _ = crafted(shape, dtype, 1)
    up = Call(torch_mod, c, shape, dtype).update()
    assert up.rc == abi.OK, up.error
    n, M = up.shapes["x"]
    x_out = up.bufs["x"][PAD:PAD + n * M].clone()
    p_out = up.bufs["p"][PAD:PAD + n * n * M].clone()
    pts = Call(torch_mod, c, shape, dtype).points(x=x_out, p=p_out)
    assert pts.rc == abi.OK, pts.error
    assert np.array_equal(pts.out("points").view(np.uint8), up.out("points").view(np.uint8)) and np.array_equal(pts.out("failed"), up.out("failed"))
    assert up.out("failed").any() and (up.out("failed") == 0).any()


def test_one_filter_step_on_real_handles(torch_mod):
    """M = 3 robots, fp64 free_hip with contact, the non-normalised task: HipSim.ukf_points, set_state on the sigma handle of
    (4nq + 1) M lanes (which takes the two halves of the points as they are, and get_state returns their bits), step, get_state,
    HipSim.ukf_update.  Every output equals the ctypes call on the same tensors and the restatement fed with their host copies,
    bit for bit; the returned points go into set_state again."""
    torch = torch_mod
    from gym_os2r_amd import ukf
    from gym_os2r_amd.sim import HipSim
    M = 3

    def make(seed, envs):
        cfg = make_config("free_hip", "BalancingV2", False, num_envs=envs, contact=True, seed=seed, auto_reset=False, dtype=abi.F64)[0]
        return HipSim(cfg)
    real = make(5, M)
    nq, D_, dev = real.nq, real.D, real.device
    n, S = 2 * nq, ukf.npoints(real.nq)
    sig = make(5, S * M)
    cpu = lambda t: t.detach().cpu().numpy().copy()
    cols = [int(v) for v in sig._layout().slot_col[:D_]]
    rng = np.random.default_rng(3)
    q, qd = real.get_state()
    x = torch.cat((q + 0.01 * torch.as_tensor(rng.normal(0, 1, (nq, M))).to(dev), qd))
    P = (1e-4 * torch.eye(n, dtype=torch.float64, device=dev)).repeat(M, 1, 1)
    Q = 1e-6 * torch.eye(n, dtype=torch.float64)
    sigma = 0.02
    prec = torch.full((D_,), 1.0 / sigma ** 2, dtype=torch.float64, device=dev)
    scalars = ukf.weights(n)
    points, failed = sig.ukf_points(x, P)
    torch.cuda.synchronize()
    want = restate_ukf_points(cpu(x), cpu(P).transpose(1, 2, 0), scalars[0], dtype=np.float64)
    assert same_bits(cpu(points), want["points"]) and (cpu(failed) == 0).all() and tuple(points.shape) == (n, S * M)
    lib, lay = ukf.load(), sig._layout()
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    for k in range(2):
        sig.set_state(points[:nq], points[nq:])
        sq, sqd = sig.get_state()
        torch.cuda.synchronize()
        assert same_bits(cpu(sq), cpu(points)[:nq]) and same_bits(cpu(sqd), cpu(points)[nq:])
        action = torch.as_tensor(rng.uniform(-0.3, 0.3, (M, 2))).to(dev)
        obs = real.step(action)[0]
        done = sig.step(action.repeat(S, 1))[2]
        state = sig.get_state()
        meas = obs + sigma * torch.as_tensor(rng.normal(0, 1, (M, D_))).to(dev)
        meas[2, 0] = float("nan")
        x, P_new, nis, used, refused, innov, lost, points, failed = sig.ukf_update(state, P, meas, prec, Q=Q, done=done, gate=0.0, want_innov=True)
        torch.cuda.synchronize()
        got = dict(x=x, p=P_new.permute(1, 2, 0), nis=nis, used=used, refused=refused, innov=innov, lost=lost, points=points, failed=failed)
        # the ctypes call on the same tensors
        mine = {k: torch.full_like(v.contiguous(), -7) for k, v in got.items()}
        rc = lib.os2ru_ukf_update(ctypes.byref(lay), M, ptr(state[0]), ptr(state[1]), ptr(done), ptr(P.permute(1, 2, 0).contiguous()),
                                  (ctypes.c_double * (n * n))(*Q.reshape(-1).tolist()), *scalars, ptr(meas), ptr(prec), 0.0,
                                  *[ptr(mine[k]) for k in ("x", "p", "nis", "used", "refused", "innov", "lost", "points", "failed")], None)
        torch.cuda.synchronize()
        assert rc == abi.OK, lib.os2ru_last_error()
        want = restate_ukf_update(cpu(state[0]), cpu(state[1]), cpu(done), cpu(P).transpose(1, 2, 0), Q.numpy(), scalars, cpu(meas), cpu(prec), cols,
                                  gate=0.0, dtype=np.float64)
        for name, t in got.items():
            a = cpu(t)
            assert np.array_equal(a.view(np.uint8), cpu(mine[name]).view(np.uint8)), (k, name)
            assert np.array_equal(a, want[name]) if name in INTS else same_bits(a, want[name]), (k, name)
        assert (cpu(lost) == 0).all() and (cpu(failed) == 0).all() and (cpu(refused) == 0).all() and cpu(used)[0] != 0 and np.isfinite(cpu(x)).all()
        assert cpu(used)[2] & 1 == 0 and (cpu(used)[0] & 1 == 1 or cols[0] < 0)
        if k:
            assert P_new.data_ptr() != P.data_ptr()                   # the two kept buffers alternate
        P = P_new
    sig.set_state(points[:nq], points[nq:])                           # the returned points are accepted
    real.close()
    sig.close()


def test_example_tracks_three_robots(torch_mod):
    """examples/ukf_tracking.py runs to its end for three robots in a fresh child process: both filters on the same seeds, a finite
    printed error and no robot lost on the flat-standing start."""
    import os
    import re
    import subprocess
    import sys
    from conftest import ROOT
    script = os.path.join(ROOT, "examples", "ukf_tracking.py")
    out = subprocess.run([sys.executable, script, "--robots", "3", "--steps", "5", "--filter", "both"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "3 robots, 5 control steps" in out.stdout
    found = {}
    for name in ("ukf", "ekf"):
        m = re.search(rf"^{name}: rms error ([0-9.e-]+) against a measurement noise of [0-9.e-]+ over 5 control steps of 3 robots; \d+ slots gated, "
                      rf"\d+ refused", out.stdout, re.M)
        assert m, out.stdout[-2000:]
        found[name] = float(m.group(1))
    assert all(np.isfinite(v) for v in found.values())
    assert re.search(r"^ukf: 0 robots lost, 0 factors failed", out.stdout, re.M), out.stdout[-2000:]
