"""os2rx_cem_update on the device (libos2r_cem.so, include/os2r_cem.h): every output bit for bit against the numpy restatement of
tests/test_cem_host.py on random and on crafted inputs, the shift and both tails, a call without the optional outputs, sigma
updated in place, the table and the lane sigma against their real consumer -- a second rollout_schedule on real handles --, and
the example."""
import ctypes

import numpy as np
import pytest

from gym_os2r_amd import abi
from helpers import make_config
from test_cem_host import BRANCH_SHAPE, SIGMA_MAX, SIGMA_MIN, crafted_cem, restate_cem

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
D = 10
FLOATS = ("nominal_out", "var", "sigma_out", "applied", "table", "lane_sigma", "threshold")
OUTPUTS = ("nominal_out", "var", "sigma_out", "applied", "table", "lane_sigma", "elite", "threshold", "count")      # the header's order
OPTIONAL = OUTPUTS[3:]
# K, M, S, E: the smallest case; three workgroups with a tail, S no multiple of 8; E = S; empty partials; many samples per lane
GPU_SHAPES = [(1, 1, 1, 1), (2, 130, 19, 5), (7, 70, 11, 11), (7, 70, 3, 2), (5, 3, 256, 32)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _np(dtype):
    return np.float64 if dtype == abi.F64 else np.float32


def random_cem(K, M, S, seed=1):
    """Inputs in float64 (the caller rounds): returns of both signs with a few exact repeats, actions, nominal and sigma as
    crafted_cem draws them."""
    rng = np.random.default_rng(seed)
    r = rng.normal(0.0, 3.0, (S, M))
    r[rng.uniform(size=(S, M)) < 0.1] = 0.5
    return dict(returns=r.reshape(-1), actions=rng.uniform(-1.0, 1.0, (K, S * M, 2)), nominal=rng.uniform(-1.0, 1.0, (K, M, 2)),
                sigma=rng.uniform(0.1, 0.4, (2, M)))


class Call:
    """One os2rx_cem_update call through ctypes: the inputs of `crafted_cem` on the device, every output between guard bands of
    PAD sentinel elements, the table filled with the sentinel.  The constructor uploads, run() launches and synchronises."""

    def __init__(self, torch, c, shape, dtype):
        from gym_os2r_amd import cem
        self.torch, self.lib, self.dtype, self.shape = torch, cem.load(), dtype, shape
        K, M, S, E = shape
        N = S * M
        dt = _np(dtype)
        self.dev = torch.device("cuda:0")
        put = lambda x: torch.as_tensor(np.ascontiguousarray(np.asarray(x).astype(dt))).to(self.dev)
        self.inputs = [put(c["returns"]), put(c["actions"]), put(c["nominal"]), put(c["sigma"])]
        self.sizes = dict(nominal_out=K * M * 2, var=K * M * 2, sigma_out=2 * M, applied=M * 2, table=K * 2 * (D + 1) * N, lane_sigma=2 * N,
                          elite=S * M, threshold=M, count=M)
        self.shapes = dict(nominal_out=(K, M, 2), var=(K, M, 2), sigma_out=(2, M), applied=(M, 2), table=(K, 2, D + 1, N), lane_sigma=(2, N),
                           elite=(S, M), threshold=(M,), count=(M,))
        self.bufs = {}
        for name, size in self.sizes.items():
            if name in FLOATS:
                self.bufs[name] = torch.full((PAD + size + PAD,), MARK, dtype=self.inputs[0].dtype, device=self.dev)
            else:
                self.bufs[name] = torch.full((PAD + size + PAD,), IMARK, dtype=torch.int32, device=self.dev)

    def run(self, shift=1, tail_zero=False, gain=1.0, sigma_gain=1.0, sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX, leave_out=(), device=0,
            in_place=False):
        from gym_os2r_amd import control
        K, M, S, E = self.shape
        lay = control.layout(self.dtype, 3, device, [-1] * D)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        outs = [None if name in leave_out else p(self.bufs[name][PAD:]) for name in OUTPUTS]
        if in_place:
            outs[2] = p(self.inputs[3])
        self.rc = self.lib.os2rx_cem_update(ctypes.byref(lay), K, M, S, E, *[p(t) for t in self.inputs], gain, sigma_gain, sigma_min, sigma_max,
                                            shift, 1 if tail_zero else 0, *outs, None)
        self.error = self.lib.os2rx_last_error()
        self.torch.cuda.synchronize()
        self.left_out = tuple(leave_out) + (("sigma_out",) if in_place else ())
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

    def check(self, c, what, **kw):
        """Every output against the restatement; every entry of the table but the bias entries still holds the sentinel."""
        K, M, S, E = self.shape
        assert self.rc == abi.OK, (what, self.rc, self.error)
        want = restate_cem(c["returns"], c["actions"], c["nominal"], c["sigma"], S=S, E=E, dtype=_np(self.dtype),
                           **dict(dict(sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX), **kw))
        for name, key in (("count", "count"), ("elite", "elite"), ("threshold", "threshold"), ("var", "var"), ("nominal_out", "nominal_out"),
                          ("applied", "applied"), ("sigma_out", "sigma_out"), ("lane_sigma", "lane_sigma")):
            got = self.out(name)
            assert got.dtype == want[key].dtype and np.array_equal(got, want[key]), (what, name, np.argwhere(got != want[key])[:4])
        table = self.out("table")
        assert np.array_equal(table[:, :, D, :], want["bias"]), (what, "bias")
        assert (table[:, :, :D, :] == MARK).all(), (what, "the weight columns of the table were touched")
        return want


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("inputs", [random_cem, crafted_cem])
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_every_output_bit_for_bit(torch_mod, shape, inputs, dtype):
    """count, elite, threshold, var, nominal_out, applied, sigma_out, lane_sigma and every bias entry of the table are equal to the
    restatement, with both gains 1 and both 0.5; every other entry of the table still holds the sentinel."""
    K, M, S, E = shape
    c = inputs(K, M, S)
    for gain, sigma_gain in ((1.0, 1.0), (0.5, 0.5)):
        kw = dict(gain=gain, sigma_gain=sigma_gain)
        want = Call(torch_mod, c, shape, dtype).run(**kw).check(c, f"{shape} {dtype} {inputs.__name__} {kw}", **kw)
        assert (want["elite"].sum(0) == np.minimum(E, want["count"])).all()
    if inputs is crafted_cem and M > 8 and S > 2:
        assert (want["count"] == 0).sum() == 1 and (want["count"] < S).sum() > 2 and (want["threshold"][4::9] == 0).all()


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("tail_zero", [False, True])
@pytest.mark.parametrize("shift", [0, 1, BRANCH_SHAPE[0]])
def test_the_shift_and_both_tails(torch_mod, shift, tail_zero, dtype):
    c = crafted_cem(*BRANCH_SHAPE[:3])
    call = Call(torch_mod, c, BRANCH_SHAPE, dtype).run(shift=shift, tail_zero=tail_zero)
    want = call.check(c, f"shift {shift} tail_zero {tail_zero} {dtype}", shift=shift, tail_zero=tail_zero)
    out = call.out("nominal_out")
    if shift and tail_zero:
        assert (out[-shift:] == 0).all() and (call.out("applied") != 0).any() and (call.out("var") != 0).any()
    if shift == 1:
        assert np.array_equal(out[:-1], want["mean"][1:]) and (out[:-1] != 0).any()


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_a_call_without_the_optional_outputs_gives_the_same_bits(torch_mod, dtype):
    """No applied, table, lane_sigma, elite, threshold or count: nominal_out, var and sigma_out are the same bits."""
    c = crafted_cem(*BRANCH_SHAPE[:3])
    whole = Call(torch_mod, c, BRANCH_SHAPE, dtype).run(gain=0.5, sigma_gain=0.5)
    whole.check(c, "whole", gain=0.5, sigma_gain=0.5)
    part = Call(torch_mod, c, BRANCH_SHAPE, dtype).run(gain=0.5, sigma_gain=0.5, leave_out=OPTIONAL)
    assert part.rc == abi.OK, part.error
    for name in OUTPUTS[:3]:
        assert np.array_equal(part.out(name).view(np.uint8), whole.out(name).view(np.uint8)), name
    assert all(part.out(name) is None for name in OPTIONAL)
    some = Call(torch_mod, c, BRANCH_SHAPE, dtype).run(gain=0.5, sigma_gain=0.5, leave_out=("table", "elite", "count"))
    assert some.rc == abi.OK, some.error
    for name in ("nominal_out", "var", "sigma_out", "applied", "lane_sigma", "threshold"):
        assert np.array_equal(some.out(name).view(np.uint8), whole.out(name).view(np.uint8)), name


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_sigma_in_place_gives_the_bits_of_the_out_of_place_call(torch_mod, dtype):
    """sigma_out_dev == sigma_in_dev is allowed: the array then holds what the out-of-place call wrote, the lane sigma too."""
    shape = GPU_SHAPES[1]
    c = crafted_cem(*shape[:3])
    apart = Call(torch_mod, c, shape, dtype).run(sigma_gain=0.5)
    apart.check(c, "apart", sigma_gain=0.5)
    same = Call(torch_mod, c, shape, dtype).run(sigma_gain=0.5, in_place=True)
    assert same.rc == abi.OK, same.error
    assert same.out("sigma_out") is None                                          # the buffer of the out-of-place call was not written
    assert np.array_equal(same.inputs[3].cpu().numpy().view(np.uint8), apart.out("sigma_out").view(np.uint8))
    assert not np.array_equal(apart.inputs[3].cpu().numpy(), apart.out("sigma_out"))
    for name in ("lane_sigma", "nominal_out", "var"):
        assert np.array_equal(same.out(name).view(np.uint8), apart.out(name).view(np.uint8)), name


def test_refusals_on_the_device(torch_mod):
    shape = GPU_SHAPES[3]
    c = crafted_cem(*shape[:3])
    call = Call(torch_mod, c, shape, abi.F64).run(device=1000)
    assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(b"os2rx_cem_update: "), (call.rc, call.error)
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)                        # a refused call wrote nothing
    call = Call(torch_mod, c, shape, abi.F64).run(gain=float("nan"))
    assert call.rc == abi.ERR_INVALID and call.error == b"os2rx_cem_update: gain must be finite"
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)
    call = Call(torch_mod, c, shape, abi.F64).run(sigma_min=0.5, sigma_max=0.25)
    assert call.rc == abi.ERR_INVALID and call.error == b"os2rx_cem_update: sigma_min must be <= sigma_max"
    call.left_out = OUTPUTS
    assert all(call.out(name) is None for name in OUTPUTS)


def test_on_real_handles_the_written_table_and_lane_sigma_drive_the_next_rollout(torch_mod):
    """M = 3 robots, S = 16 samples, K = 5 knots, E = 4 elites, fp64 free_hip with contact: copy_envs_from(real, index), the noisy
    scheduled rollout, cem_update.  The outputs equal the restatement on what the rollout returned; a second rollout_schedule with
    the written table and the returned lane sigma applies, in lane s M + m, exactly clip(nominal_out[k][m] + sigma_out[m] eps) of
    the noise it returns, and takes the lane sigma without a copy; the handle's two nominal buffers alternate."""
    torch = torch_mod
    from gym_os2r_amd.sim import HipSim
    M, S, K, E = 3, 16, 5, 4
    N = S * M

    def make(num, auto_reset):
        cfg = make_config("free_hip", "BalancingV2", False, num_envs=num, contact=True, seed=5, auto_reset=auto_reset, dtype=abi.F64)[0]
        return HipSim(cfg)
    real, planner = make(M, True), make(N, False)
    Dn, dev = real.D, real.device
    cpu = lambda t: t.detach().cpu().numpy().copy()
    index = (torch.arange(N, device=dev) % M).to(torch.int32)
    rng = np.random.default_rng(3)
    nominal = torch.as_tensor(rng.uniform(-0.3, 0.3, (K, M, 2))).to(dev)
    sigma = torch.as_tensor(rng.uniform(0.2, 0.4, (M, 2))).to(dev)
    table = torch.zeros(K, 2, Dn + 1, N, dtype=torch.float64, device=dev)
    table[:, :, Dn, :] = nominal.permute(0, 2, 1)[:, :, index.long()]
    table = table.permute(3, 0, 1, 2)                                             # [N, K, 2, D+1], as rollout_schedule takes it
    planner.copy_envs_from(real, index)
    ret, _, _, (act, _) = planner.rollout_schedule(K, table, sigma=sigma[index.long()], first_episode=True, want_actions=True)
    kw = dict(gain=0.75, sigma_gain=0.5, sigma_min=0.01, sigma_max=0.6)
    applied, new, table2, sig, lane, var, elite, thr, count = planner.cem_update(ret, act, nominal, sigma, samples=S, elites=E, table=table,
                                                                                 want_elite=True, **kw)
    torch.cuda.synchronize()
    assert table2.data_ptr() == table.data_ptr() and tuple(table2.shape) == (N, K, 2, Dn + 1) and new.data_ptr() != nominal.data_ptr()
    assert tuple(sig.shape) == (M, 2) and tuple(lane.shape) == (N, 2) and sig.t().is_contiguous() and lane.t().is_contiguous()
    want = restate_cem(cpu(ret), cpu(act), cpu(nominal), cpu(sigma).T, S=S, E=E, shift=1, tail_zero=False, dtype=np.float64, **kw)
    for name, got in (("nominal_out", new), ("applied", applied), ("var", var), ("elite", elite), ("threshold", thr), ("count", count),
                      ("sigma_out", sig.t()), ("lane_sigma", lane.t())):
        assert np.array_equal(cpu(got), want[name]), name
    assert (cpu(count) == S).all() and (cpu(elite).sum(0) == E).all() and len(np.unique(cpu(ret))) > M
    kernel_view = cpu(table2.permute(1, 2, 3, 0))
    assert np.array_equal(kernel_view[:, :, Dn, :], want["bias"]) and (kernel_view[:, :, :Dn, :] == 0).all()
    # the real consumer: the same start, the written table and the returned lane sigma
    planner.copy_envs_from(real, index)
    assert planner._sigma(lane)[0].data_ptr() == lane.t().data_ptr()              # no copy on the way into the rollout
    _, _, _, (act2, eps) = planner.rollout_schedule(K, table2, sigma=lane, want_actions=True, want_noise=True)
    torch.cuda.synchronize()
    lanes = cpu(index)
    drawn = np.clip(want["nominal_out"][:, lanes] + want["sigma_out"].T[lanes][None] * cpu(eps), -1.0, 1.0)
    assert np.array_equal(cpu(act2), drawn) and (cpu(eps) != 0).all() and (np.abs(cpu(act2)) < 1).any()
    obs, rew, done, _ = real.step(applied)
    torch.cuda.synchronize()
    assert tuple(obs.shape) == (M, Dn) and np.isfinite(cpu(obs)).all() and np.isfinite(cpu(rew)).all()
    # fed back, the nominal goes to the other buffer and sigma goes on without a copy; table=True is the handle's own table, kept
    fed = cpu(new)                                                               # (the third call writes this buffer again)
    second = planner.cem_update(ret, act, new, sig, samples=S, elites=E, shift=0, tail="zero", table=True, want_variance=False, **kw)
    third = planner.cem_update(ret, act, second[1], second[3], samples=S, elites=E, table=True, **kw)
    torch.cuda.synchronize()
    assert second[1].data_ptr() not in (new.data_ptr(), nominal.data_ptr()) and third[1].data_ptr() == new.data_ptr()
    assert third[2].data_ptr() == second[2].data_ptr() != table.data_ptr() and (cpu(second[2].permute(1, 2, 3, 0))[:, :, :Dn, :] == 0).all()
    assert second[5] is None and second[6] is None and third[5] is not None
    again = restate_cem(cpu(ret), cpu(act), fed, want["sigma_out"], S=S, E=E, shift=0, tail_zero=True, dtype=np.float64, **kw)
    assert np.array_equal(cpu(second[1]), again["mean"]) and np.array_equal(cpu(second[3]).T, again["sigma_out"])
    real.close()
    planner.close()


def test_example_plans_for_three_robots(torch_mod):
    """examples/cem_balancing.py runs to its end for three robots: its sigmas lie within the bounds, its returns are finite."""
    import os
    import re
    import subprocess
    import sys
    from conftest import ROOT
    script = os.path.join(ROOT, "examples", "cem_balancing.py")
    out = subprocess.run([sys.executable, script, "--robots", "3", "--lanes", "32", "--elites", "4", "--horizon", "10", "--iters", "2",
                          "--steps", "5"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "3 robots x 32 lanes (4 elites) x horizon 10 x 2 iterations" in out.stdout
    bounds = re.search(r"sigma in \[([0-9.e+-]+), ([0-9.e+-]+)\]", out.stdout)
    lo, hi = float(bounds.group(1)), float(bounds.group(2))
    steps = re.findall(r"^control step (\d+): mean return so far +([-+0-9.e]+), mean sigma per iteration ((?:[0-9.e+-]+ ?)+)$", out.stdout, re.M)
    assert [int(s[0]) for s in steps] == [1, 2, 3, 4, 5], out.stdout[-2000:]
    for _, so_far, sigmas in steps:
        values = [float(v) for v in sigmas.split()]
        assert len(values) == 2 and all(lo <= v <= hi for v in values) and np.isfinite(float(so_far))
    last = re.search(r"^return per robot: ((?:[-+0-9.e]+ ?)+)$", out.stdout, re.M)
    assert last and len(last.group(1).split()) == 3 and all(np.isfinite(float(v)) for v in last.group(1).split()), out.stdout[-2000:]
