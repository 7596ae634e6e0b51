"""os2ri_perturb and os2ri_update on the device (libos2r_sysid.so, include/os2r_sysid.h): every output bit for bit against the numpy
restatement of tests/sysid_ref.py, in both dtypes, at the shapes where the kernels take another path (one, two and twenty-one
parameters: one wave, one pair, eleven pairs and a tile of three slots; 1, 64, 65 and 130 segments per set: the few-segments sum,
its last shape, the wave sum and its third round; one and three sets; one and three steps); the crafted sets of
tests/test_sysid_host.py, which reach every branch of the update, a held parameter and a failing pivot; os2ri_perturb against the
restatement and through set_params / get_params; the two identification problems of the host test on a HipSim, the device loop
against the restatement fed the device's observations in every iteration; and the `_into` forms (no allocation, nothing written
that was not asked for)."""
import ctypes

import numpy as np
import pytest

import sysid_ref as R
from gym_os2r_amd import abi
from test_sysid_host import check_roles

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
INTEGER = {"status": np.int32, "iters": np.int32, "valid": np.int32, "accepted": np.uint8, "failed": np.int32, "counts": np.int32}
OUTPUTS = R.STATE + ("theta_next", "cost", "valid", "accepted", "failed", "delta", "sums", "counts")        # the header's order
OPTIONAL = ("cost", "valid", "accepted", "failed", "delta")
D_TASK = 10


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _np(dtype):
    return np.float64 if dtype == abi.F64 else np.float32


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dbl(v):
    return (ctypes.c_double * len(v))(*[float(x) for x in v])


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Guarded:
    """Device buffers between guard bands of PAD sentinel elements."""

    def __init__(self, torch, real, shapes):
        self.shapes = shapes
        self.sizes = {k: int(np.prod(v)) for k, v in shapes.items()}
        kind = lambda k: {np.int32: torch.int32, np.uint8: torch.uint8}[INTEGER[k]] if k in INTEGER else real
        self.mark = {k: (IMARK if INTEGER.get(k) is np.int32 else 200 if k in INTEGER else MARK) for k in shapes}
        self.bufs = {k: torch.full((PAD + n + PAD,), self.mark[k], dtype=kind(k), device="cuda:0") for k, n in self.sizes.items()}

    def ptr(self, name):
        return _p(self.bufs[name][PAD:])

    def out(self, name, written=True):
        host, mark, n = self.bufs[name].cpu().numpy(), self.mark[name], self.sizes[name]
        assert (host[:PAD] == mark).all() and (host[PAD + n:] == mark).all(), f"{name}: written outside"
        if not written:
            assert (host[PAD:PAD + n] == mark).all(), f"{name}: written although not asked for"
            return None
        return host[PAD:PAD + n].reshape(self.shapes[name])


def _dev(torch, a, kind):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, kind))).to("cuda:0")


def update(torch, dtype, c, *, wanted=OPTIONAL, with_done=True):
    """One os2ri_update call through ctypes on the problem c -> (status, error text, dict of the outputs on the host)."""
    from gym_os2r_amd import control, sysid
    real, kind = (torch.float64 if dtype == abi.F64 else torch.float32), _np(dtype)
    T, P, M = c["T"], c["P"], c["M"]
    E = R.nsums(P)
    shapes = dict(theta_best=(T, P), cost_best=(T,), hess=(T, P, P), grad=(T, P), lam=(T,), status=(T,), iters=(T,), theta_next=(T, P), cost=(T,),
                  valid=(T,), accepted=(T,), failed=(T,), delta=(T, P), sums=(E * (M + T),), counts=(M + T,))
    g = Guarded(torch, real, shapes)
    ins = [_dev(torch, c["obs"], kind), _dev(torch, c["meas"], kind), _dev(torch, c["done"], np.uint8) if with_done else None, _dev(torch, c["prec"], kind),
           _dev(torch, c["theta"], kind)] + [_dev(torch, c["state"][n], np.int32 if n in ("status", "iters") else kind) for n in R.STATE]
    lay = control.layout(dtype, 5, 0, [-1] * c["D"])
    k = sysid.constants(**c["consts"])
    lib = sysid.load()
    opt = lambda name: g.ptr(name) if name in wanted else None
    rc = lib.os2ri_update(ctypes.byref(lay), P, T, M, c["K"], _dbl(c["h"]), _dbl(c["lo"]), _dbl(c["hi"]), ctypes.byref(k), *[_p(t) for t in ins],
                          *[g.ptr(n) for n in R.STATE], g.ptr("theta_next"), *[opt(n) for n in OPTIONAL], g.ptr("sums"), g.ptr("counts"), None)
    err = lib.os2ri_last_error()
    torch.cuda.synchronize()
    return rc, err, {n: g.out(n, rc == abi.OK and (n not in OPTIONAL or n in wanted)) for n in OUTPUTS}


def against_the_restatement(c, out, want, what):
    """Every output of the device against the restatement, bit for bit; the scratch too (the sums of the segments, their verdicts,
    the totals of the sets that ran)."""
    T, M, E = c["T"], c["M"], R.nsums(c["P"])
    for n in R.STATE + ("theta_next", "cost", "valid", "accepted", "failed", "delta"):
        assert _same(out[n], want[n]), (what, n, out[n], want[n])
    seg = out["sums"][:E * M].reshape(E, M)
    assert np.array_equal(out["counts"][:M], want["seg_valid"]) and np.array_equal(out["counts"][M:], want["valid"]), what
    ok = want["seg_valid"] != 0
    assert _same(seg[:, ok], want["sums"][:, ok]), what                  # (a segment that is not valid holds NaNs, whose bits are free)
    ran = want["valid"] > 0
    assert _same(out["sums"][E * M:].reshape(E, T)[:, ran], want["totals"][:, ran]), what


# ---------------------------------------------------------------------------------------
# bit for bit at the shapes where the kernels take another path
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("P", [1, 2, 21])
def test_every_output_against_the_restatement(torch_mod, P, T, dtype):
    kind = _np(dtype)
    for Q in (1, 64, 65, 130):
        for K in (1, 3):
            c = R.shaped_problem(T, Q, K, P, D_TASK, kind)
            rc, err, out = update(torch_mod, dtype, c)
            assert rc == abi.OK, (Q, K, err)
            want = R.restate(c, kind)
            against_the_restatement(c, out, want, (P, T, Q, K))
            assert want["accepted"][0] == 1 and want["valid"][0] == Q
            if T == 3:
                assert want["accepted"][1] == 0 and want["valid"][2] == Q - 1 and (Q == 1 or want["accepted"][2] == 1)


# ---------------------------------------------------------------------------------------
# the crafted sets
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_the_crafted_sets_on_the_device(torch_mod, dtype):
    """Accept, reject, the freezes by tol, cost_floor and lam_max, a set without a valid segment, a done byte in a minus lane, a NaN in
    a plus lane and at the nominal, a skipped reading, dropped slots, a one-sided quotient, a frozen set that passes through bit for
    bit; then a held parameter and a failing pivot; then the call without its optional outputs and without done."""
    kind = _np(dtype)
    c = R.crafted_roles(kind)
    rc, err, out = update(torch_mod, dtype, c)
    assert rc == abi.OK, err
    want = R.restate(c, kind)
    against_the_restatement(c, out, want, "roles")
    check_roles(c, out, kind)
    for make in (R.crafted_held, R.crafted_pivot):
        d = make(kind)
        rc, err, got = update(torch_mod, dtype, d)
        assert rc == abi.OK, err
        against_the_restatement(d, got, R.restate(d, kind), make.__name__)
    assert got["failed"][0] == 1 and not got["delta"].any()
    rc, err, bare = update(torch_mod, dtype, c, wanted=(), with_done=False)
    assert rc == abi.OK, err
    c2 = dict(c, done=np.zeros_like(c["done"]))
    want2 = R.restate(c2, kind)
    for n in R.STATE + ("theta_next",):
        assert _same(bare[n], want2[n]), n
    assert want2["valid"][c["role"]["no_valid"]] == 2
    # a refusal on the device's side of the checks writes nothing either
    from gym_os2r_amd import control, sysid
    lib = sysid.load()
    lay = control.layout(dtype, 5, 0, [-1] * c["D"])
    t = torch_mod.zeros(64, dtype=torch_mod.float64, device="cuda:0")
    assert lib.os2ri_perturb(ctypes.byref(lay), 1, 1, 1, (ctypes.c_int32 * 2)(4, 0), _dbl([0.1]), _dbl([0]), _dbl([1]), _p(t), _p(t[8:]), _p(t[8:]), None) \
        == abi.ERR_INVALID
    assert lib.os2ri_last_error() == b"os2ri_perturb: params_dev overlaps base_dev" and not t.any()


# ---------------------------------------------------------------------------------------
# the HipSim methods
# ---------------------------------------------------------------------------------------
def _cpu(t):
    return t.detach().cpu().numpy().copy()


def _handle(c, n, dtype=abi.F64):
    from gym_os2r_amd.sim import HipSim
    return HipSim(c["config"](n, dtype)[0])


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_perturb_against_the_restatement_and_through_set_params(torch_mod, oracle, dtype):
    """Every lane of os2ri_perturb equals the restatement, bound hits included; the unidentified rows equal base; and the blocks of
    the packed array, handed to set_params and read back with get_params, come back bit for bit."""
    torch = torch_mod
    from gym_os2r_amd import sysid
    kind = _np(dtype)
    c = R.loop_case("B", oracle)
    P, M, nq, T = 3, c["M"], c["nq"], 2
    S = 2 * P + 1
    sim = _handle(c, S * M, dtype)
    rng = np.random.default_rng(5)
    base = sysid.pack({f: sim.get_params(f)[:, :M].contiguous() for f in sysid.FIELDS}, nq)
    base = base * torch.as_tensor(rng.uniform(0.9, 1.1, tuple(base.shape))).to(base)
    theta = torch.as_tensor(np.array([[1.0, 0.001, 1.0], [0.1, 0.04995, 1.4999]])).to(base)         # set 1 sits at or next to its bounds
    params = sim.sysid_perturb(theta, base, sel=c["sel"], h=c["h"], lo=c["lo"], hi=c["hi"])
    want = R.restate_perturb(_cpu(theta), _cpu(base), c["rows"], c["h"], c["lo"], c["hi"], kind)
    assert tuple(params.shape) == (4 * nq + 1, S * M) and _same(_cpu(params), want)
    lanes = _cpu(params).reshape(4 * nq + 1, S, M)
    free = [r for r in range(4 * nq + 1) if r not in c["rows"]]
    assert (lanes[free] == _cpu(base)[free][:, None, :]).all()
    assert lanes[c["rows"][0], 1 + P, 1] == kind(0.1) and lanes[c["rows"][1], 2, 1] == kind(0.05) and lanes[c["rows"][2], 3, 1] == kind(1.5)
    for f in sysid.FIELDS:
        block = sysid.field_view(params, nq, f)
        assert block.is_contiguous() and block.data_ptr() == params[f * nq].data_ptr()
        sim.set_params(f, block)
        assert torch.equal(sim.get_params(f), block), f
    sim.close()


def device_loop(torch, c):
    """The identification loop on a HipSim: the log is made by a handle that holds the truth; then perturb -> set_params x 5 ->
    set_state -> rollout -> update, six times, every iteration compared with the restatement fed the device's observations and
    state.  -> (the device's outputs per iteration, the relative errors at the end)."""
    from gym_os2r_amd import sysid
    P, M, K, nq = len(c["sel"]), c["M"], c["K"], c["nq"]
    S = 2 * P + 1
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")
    real = _handle(c, M)
    base = sysid.pack({f: real.get_params(f) for f in sysid.FIELDS}, nq)
    truth = base.clone()
    for r, v in zip(c["rows"], c["truth"]):
        truth[r] = v
    for f in sysid.FIELDS:
        real.set_params(f, sysid.field_view(truth, nq, f))
    real.set_state(dev(c["q0"]), dev(c["qd0"]))
    meas = real.rollout(K, dev(c["actions"]))[0]
    real.close()
    sim = _handle(c, S * M)
    q0, qd0, actions = dev(np.tile(c["q0"], (1, S))), dev(np.tile(c["qd0"], (1, S))), dev(np.tile(c["actions"], (1, S, 1)))      # once
    prec = torch.ones(sim.D, dtype=torch.float64, device="cuda:0")
    theta = dev(np.array([c["start"]]))
    state = sim.sysid_init(theta, R.LOOP_LAM0)
    steps = dict(h=c["h"], lo=c["lo"], hi=c["hi"])
    history = []
    for it in range(R.LOOP_ITERS):
        params = sim.sysid_perturb(theta, base, sel=c["sel"], **steps)
        for f in sysid.FIELDS:
            sim.set_params(f, sysid.field_view(params, nq, f))
        sim.set_state(q0, qd0)
        obs, _, done, _, _ = sim.rollout(K, actions)
        new, theta_next, info = sim.sysid_update(obs, meas, prec, theta, state, done=done, **steps)
        host = dict(zip(R.STATE, (_cpu(t) for t in state)))
        want = R.restate_update(_cpu(obs), _cpu(meas), _cpu(done), _cpu(prec), _cpu(theta), c["h"], c["lo"], c["hi"], host, R.DEFAULTS, np.float64)
        got = dict(zip(R.STATE + ("theta_next", "cost", "valid", "accepted", "failed", "delta"), (_cpu(t) for t in new + (theta_next,) + info)))
        for n in got:
            assert _same(got[n], want[n]), (it, n, got[n], want[n])
        history.append(got)
        state, theta = new, theta_next
    sim.close()
    true = np.array(c["truth"])
    return history, np.abs(history[-1]["theta_best"][0] - true) / np.abs(true)


@pytest.mark.parametrize("name", ["A", "B"])
def test_the_loop_identifies_the_parameters_on_the_device(torch_mod, oracle, name):
    """Cases A and B of tests/test_sysid_host.py on a HipSim in fp64: theta_next, lam, status and accepted of every iteration (and
    every other output) equal the restatement fed the device's observations, bit for bit; cost_best never rises; every parameter
    ends within 1e-4 relative of the truth."""
    c = R.loop_case(name, oracle)
    history, err = device_loop(torch_mod, c)
    best = [h["cost_best"][0] for h in history]
    print(name, "cost_best", best, "relative error", err, "valid", [int(h["valid"][0]) for h in history], "accepted", [int(h["accepted"][0]) for h in history])
    assert all(b <= a for a, b in zip(best, best[1:])) and (err <= R.LOOP_BOUND).all(), err


def test_into_forms_allocate_nothing_and_write_what_was_asked(torch_mod, oracle):
    torch = torch_mod
    from gym_os2r_amd import sysid
    c = R.loop_case("A", oracle)
    sim = _handle(c, 8)
    p = R.crafted_roles(np.float64, D=sim.D)
    T, P, M, K, D = p["T"], p["P"], p["M"], p["K"], p["D"]
    N, E, dev, i32, u8 = (2 * P + 1) * M, R.nsums(P), sim.device, torch.int32, torch.uint8
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    obs, meas, done, prec, theta = (to(p[k]) for k in ("obs", "meas", "done", "prec", "theta"))
    state = tuple(to(p["state"][n]) for n in R.STATE)
    z = lambda *s, dtype=sim.dtype: torch.full(s, -3, dtype=dtype, device=dev)
    new = (z(T, P), z(T), z(T, P, P), z(T, P), z(T), z(T, dtype=i32), z(T, dtype=i32))
    nxt, sums, counts = z(T, P), z(E * (M + T)), z(M + T, dtype=i32)
    cost, valid, accepted, failed, delta = z(T), z(T, dtype=i32), torch.full((T,), 9, dtype=u8, device=dev), z(T, dtype=i32), z(T, P)
    base, params = to(np.arange(sysid.rows(sim.nq) * M, dtype=np.float64).reshape(-1, M)), z(sysid.rows(sim.nq), N)
    sel = [(abi.PARAM_DAMPING, 0), (abi.PARAM_MU, 1), (abi.PARAM_GRAVITY, 0)]
    steps, k = dict(h=p["h"], lo=p["lo"], hi=p["hi"]), sysid.constants(**p["consts"])
    sim.sysid_perturb_into(theta, base, params, sel=sel, **steps)                                  # (the loader and the layout, once)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    sim.sysid_perturb_into(theta, base, params, sel=sel, **steps)
    sim.sysid_update_into(obs, meas, prec, theta, state, new, nxt, sums, counts, constants=k, done=done, **steps)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before
    assert (cost == -3).all() and (valid == -3).all() and (accepted == 9).all() and (failed == -3).all() and (delta == -3).all()
    sim.sysid_update_into(obs, meas, prec, theta, state, new, nxt, sums, counts, constants=k, done=done, accepted=accepted, delta=delta, **steps)
    torch.cuda.synchronize()
    assert (cost == -3).all() and (valid == -3).all() and (failed == -3).all() and not (accepted == 9).any()
    want = R.restate(p, np.float64)
    for have, n in zip(new + (nxt, accepted, delta), R.STATE + ("theta_next", "accepted", "delta")):
        assert _same(_cpu(have), want[n]), n
    rows = [sysid.row(sim.nq, f, i) for f, i in sel]
    assert _same(_cpu(params), R.restate_perturb(p["theta"], _cpu(base), rows, p["h"], p["lo"], p["hi"], np.float64))
    # the allocating forms return the same bits
    assert torch.equal(sim.sysid_perturb(theta, base, sel=sel, **steps), params)
    new2, nxt2, info = sim.sysid_update(obs, meas, prec, theta, state, constants=k, done=done, **steps)
    assert all(torch.equal(a, b) for a, b in zip(new2 + (nxt2,), new + (nxt,))) and len(info) == 5
    for have, n in zip(info, ("cost", "valid", "accepted", "failed", "delta")):
        assert _same(_cpu(have), want[n]), n
    assert sim.sysid_update(obs, meas, prec, theta, state, constants=k, done=done, want_info=False, **steps)[2] is None
    fresh = sim.sysid_init(theta)
    assert torch.equal(fresh[0], theta) and torch.isinf(fresh[1]).all() and (fresh[4] == 1e-3).all() and not fresh[5].any()
    sim.close()
