"""os2ra_es_perturb and os2ra_es_update on the device (libos2r_es.so, include/os2r_es.h): the directions against Box-Muller on the
oracle's uniform2 with the documented counter words; the weights bit for bit against the header's formula on the device's own
directions; every output of the update bit for bit against the numpy restatement of tests/test_es_host.py fed with those
directions -- which proves that the update regenerated the bits the perturbation added --, for every top, with ties at the cut,
NaN and infinite returns, a population without a valid direction and one on which sigma_floor binds; the `_into` forms (no
allocation, nothing written that was not asked for); refusals that write nothing; and the calls around their real consumer:
es_perturb -> rollout_policy -> es_update on a handle of 48 environments."""
import ctypes

import numpy as np
import pytest

from gym_os2r_amd import abi
from helpers import make_config
from test_es_host import FLAT, FLOOR, NONE_VALID, NU, SHAPES, STEP, cpu_directions, crafted_es, restate_perturb, restate_update, tops

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
SEED, OFFSET, GENERATION = 0x1234567890abcdef, 2 ** 32 - 100, 2 ** 32 - 1
# Device libm and numpy differ in the last bits of log, sin and cos.  The directions are the device normal2 the exploration
# noise is drawn with, whose distance from numpy was measured on the MI355X as max |dE| / max(|E|, 1) = 2.454e-16
# (tests/test_gpu_policy_noise.py); the bound is 8 x that, restated here (anything above 1e-12 would be a wrong stream or a float
# evaluation).
NOISE_STREAM_TOL = 8 * 2.454e-16
UPDATE_OUTPUTS = ("theta_new", "sigma_r", "count", "used", "grad", "kept", "score")   # the header's order
INTEGER = ("count", "used", "kept")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _np(dtype):
    return np.float64 if dtype == abi.F64 else np.float32


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Guarded:
    """Device buffers between guard bands of PAD sentinel elements."""

    def __init__(self, torch, real, shapes):
        self.torch, self.shapes = torch, shapes
        self.sizes = {k: int(np.prod(v)) for k, v in shapes.items()}
        self.bufs = {k: torch.full((PAD + n + PAD,), IMARK if k in INTEGER else MARK, dtype=torch.int32 if k in INTEGER else real,
                                   device="cuda:0") for k, n in self.sizes.items()}

    def ptr(self, name):
        return _p(self.bufs[name][PAD:])

    def out(self, name, written=True):
        host = self.bufs[name].cpu().numpy()
        mark = IMARK if name in INTEGER else MARK
        n = self.sizes[name]
        assert (host[:PAD] == mark).all() and (host[PAD + n:] == mark).all(), f"{name}: written outside"
        if not written:
            assert (host[PAD:PAD + n] == mark).all(), f"{name}: written although not asked for"
            return None
        return host[PAD:PAD + n].reshape(self.shapes[name])


def perturb(torch, dtype, M, S, D, theta, *, nu=NU, seed=SEED, offset=OFFSET, generation=GENERATION, want_delta=True, device=0):
    """One os2ra_es_perturb call through ctypes -> (status, error text, weights | None, delta | None) on the host."""
    from gym_os2r_amd import control, es
    real = torch.float64 if dtype == abi.F64 else torch.float32
    g = Guarded(torch, real, dict(weights=(2 * S * M, 2, D + 1), delta=(S * M, 2, D + 1)))
    th = torch.as_tensor(np.asarray(theta, _np(dtype))).to("cuda:0")
    lay = control.layout(dtype, 3, device, [-1] * D)
    lib = es.load()
    rc = lib.os2ra_es_perturb(ctypes.byref(lay), M, S, 0, seed, offset, generation, _p(th), nu, g.ptr("weights"),
                              g.ptr("delta") if want_delta else None, None)
    err = lib.os2ra_last_error()
    torch.cuda.synchronize()
    return rc, err, g.out("weights", rc == abi.OK), g.out("delta", rc == abi.OK and want_delta)


def update(torch, dtype, M, S, D, returns, theta, top, *, step_size=STEP, sigma_floor=FLOOR, seed=SEED, offset=OFFSET, generation=GENERATION,
           want_grad=True, device=0):
    """One os2ra_es_update call through ctypes -> (status, error text, dict of the outputs on the host); an output that was not
    asked for (grad; score where top does not select) must still hold its sentinel."""
    from gym_os2r_amd import control, es
    real = torch.float64 if dtype == abi.F64 else torch.float32
    SM = S * M
    g = Guarded(torch, real, dict(theta_new=(M, 2, D + 1), sigma_r=(M,), count=(M,), used=(M,), grad=(M, 2, D + 1), kept=(SM,), score=(SM,)))
    r = torch.as_tensor(np.asarray(returns, _np(dtype))).to("cuda:0")
    th = torch.as_tensor(np.asarray(theta, _np(dtype))).to("cuda:0")
    lay = control.layout(dtype, 3, device, [-1] * D)
    lib = es.load()
    rc = lib.os2ra_es_update(ctypes.byref(lay), M, S, top, 0, seed, offset, generation, _p(r), _p(th), step_size, sigma_floor,
                             g.ptr("theta_new"), g.ptr("sigma_r"), g.ptr("count"), g.ptr("used"), g.ptr("grad") if want_grad else None,
                             g.ptr("kept"), g.ptr("score"), None)
    err = lib.os2ra_last_error()
    torch.cuda.synchronize()
    ok = rc == abi.OK
    out = {name: g.out(name, ok and (name != "grad" or want_grad)) for name in UPDATE_OUTPUTS if name != "score"}
    select = 0 < top < S
    host = g.bufs["score"].cpu().numpy()                  # scratch: written where top selects (its contents are not part of the contract)
    assert (host[:PAD] == MARK).all() and (host[PAD + SM:] == MARK).all() and (select and ok or (host == MARK).all())
    return rc, err, out


@pytest.fixture(scope="module")
def device_directions(torch_mod):
    """delta of every shape, D and dtype as es_perturb wrote it, with the weights of the same call; made once and left unchanged."""
    made = {}
    for (M, S) in SHAPES:
        for D in (10, 3):
            for dtype in (abi.F64, abi.F32):
                theta = crafted_es(M, S, D, _np(dtype))["theta"]
                rc, err, weights, delta = perturb(torch_mod, dtype, M, S, D, theta)
                assert rc == abi.OK, (M, S, D, dtype, err)
                made[(M, S, D, dtype)] = (weights, delta)
    return made


# ---------------------------------------------------------------------------------------
# the stream
# ---------------------------------------------------------------------------------------
def test_directions_are_stream_6_of_the_counter_rng(torch_mod, device_directions, oracle):
    """f64: delta against Box-Muller on the oracle's uniform2(seed, (pop_offset + m) mod 2^32, 6, generation, 16 s + (e >> 1)) at
    a pop_offset that wraps inside the 257 populations and generation 2^32 - 1, for one-thread and wave shapes at both D.  f32:
    the same directions rounded once to float, bit for bit.  A different generation, population or direction is a different
    draw; pop_offset = a at population m is pop_offset = 0 at population a + m."""
    from gym_os2r_amd import es
    assert es.STREAM == 6
    worst = 0.0
    for (M, S, D) in ((3, 65, 10), (257, 2, 10), (5, 64, 3), (1, 1, 3)):
        d64, d32 = device_directions[(M, S, D, abi.F64)][1], device_directions[(M, S, D, abi.F32)][1]
        ref = cpu_directions(oracle, SEED, OFFSET, GENERATION, M, S, D)
        worst = max(worst, float(np.max(np.abs(d64 - ref) / np.maximum(np.abs(ref), 1.0))))
        assert d32.dtype == np.float32 and np.array_equal(d32.view(np.uint32), d64.astype(np.float32).view(np.uint32)), (M, S, D)
    print(f"[es stream] max |d delta| / max(|delta|, 1) = {worst:.3e} (bound {NOISE_STREAM_TOL:.3e})")
    assert worst <= NOISE_STREAM_TOL <= 1e-12, worst
    M, S, D = 3, 65, 10
    theta = crafted_es(M, S, D, np.float64)["theta"]
    base = device_directions[(M, S, D, abi.F64)][1].reshape(S, M, 2, D + 1)
    other = perturb(torch_mod, abi.F64, M, S, D, theta, generation=GENERATION - 1)[3].reshape(S, M, 2, D + 1)
    assert np.max(np.abs(other - base)) > 1.0                                        # another generation
    assert np.max(np.abs(base[:, 1] - base[:, 0])) > 1.0 and np.max(np.abs(base[1] - base[0])) > 1.0   # another population, direction
    assert np.max(np.abs(perturb(torch_mod, abi.F64, M, S, D, theta, seed=SEED + 1)[3].reshape(base.shape) - base)) > 1.0
    # (... and on the CPU: the counter words are the documented ones, so the other draws differ there too)
    assert np.max(np.abs(cpu_directions(oracle, SEED, OFFSET, GENERATION - 1, M, 2, D) - cpu_directions(oracle, SEED, OFFSET, GENERATION, M, 2, D))) > 1.0
    # a shard: populations a .. a + M - 1 of a call at pop_offset 0 are those of a call at pop_offset a
    a = 2
    wide_theta = np.concatenate([np.zeros((a, 2, D + 1)), theta])
    for dtype in (abi.F64, abi.F32):
        _, _, w_wide, d_wide = perturb(torch_mod, dtype, a + M, S, D, wide_theta, offset=0)
        _, _, w_shard, d_shard = perturb(torch_mod, dtype, M, S, D, theta, offset=a)
        assert np.array_equal(d_wide.reshape(S, a + M, -1)[:, a:], d_shard.reshape(S, M, -1))
        assert np.array_equal(w_wide.reshape(2 * S, a + M, -1)[:, a:], w_shard.reshape(2 * S, M, -1))


# ---------------------------------------------------------------------------------------
# the perturbation
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("D", [10, 3])
def test_weights_are_the_headers_formula_on_the_devices_directions(torch_mod, device_directions, D, dtype):
    """weights = theta +- nu delta with the product rounded on its own, plus lanes first, lane (h S + s) M + m; without delta_dev
    the weights are the same and nothing else is written."""
    for (M, S) in SHAPES:
        theta = crafted_es(M, S, D, _np(dtype))["theta"]
        weights, delta = device_directions[(M, S, D, dtype)]
        want = restate_perturb(theta, delta, NU, S=S, dtype=_np(dtype))
        assert weights.dtype == want.dtype and np.array_equal(weights, want), (M, S, np.argwhere(weights != want)[:4])
        plus, minus = weights[:S * M].reshape(S, M, -1), weights[S * M:].reshape(S, M, -1)
        moved = np.float64(NU).astype(_np(dtype)) * delta.reshape(S, M, -1)
        assert np.array_equal(plus, theta.reshape(1, M, -1) + moved) and np.array_equal(minus, theta.reshape(1, M, -1) - moved)
    M, S = SHAPES[3]
    rc, err, bare, none = perturb(torch_mod, dtype, M, S, D, crafted_es(M, S, D, _np(dtype))["theta"], want_delta=False)
    assert rc == abi.OK and none is None and np.array_equal(bare, device_directions[(M, S, D, dtype)][0])


# ---------------------------------------------------------------------------------------
# the update
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("D", [10, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_of_the_update_against_the_restatement(torch_mod, device_directions, shape, D, dtype):
    """theta_new, sigma_r, count, used, grad and kept equal the restatement on the device's own delta for top in {0, 1, ceil(S / 2),
    S, 2 S}: the update regenerated the bits the perturbation added.  The crafted returns tie at the cut, carry NaN and +-inf,
    a population without a valid direction and one whose returns are all equal."""
    M, S = shape
    real = _np(dtype)
    c = crafted_es(M, S, D, real)
    delta = device_directions[(M, S, D, dtype)][1]
    seen = set()
    for top in tops(S):
        rc, err, got = update(torch_mod, dtype, M, S, D, c["returns"], c["theta"], top)
        assert rc == abi.OK, (top, err)
        want = restate_update(c["returns"], c["theta"], delta, S=S, dtype=real, top=top)
        for name in ("theta_new", "sigma_r", "count", "used", "grad", "kept"):
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), \
                (shape, D, top, name, np.argwhere(got[name] != want[name])[:4])
        seen.add(want["kept"].tobytes())
        if M > 3:
            assert want["count"][NONE_VALID] == 0 == want["sigma_r"][NONE_VALID] and np.array_equal(want["theta_new"][NONE_VALID], c["theta"][NONE_VALID])
            assert want["sigma_r"][FLAT] == real(FLOOR) and want["used"][FLAT] > 0
    if S >= 64:
        assert len(seen) >= 3                                                        # the tops differ in what they keep
    # without grad_dev the other outputs are the same and grad is not written
    rc, err, bare = update(torch_mod, dtype, M, S, D, c["returns"], c["theta"], tops(S)[2], want_grad=False)
    want = restate_update(c["returns"], c["theta"], delta, S=S, dtype=real, top=tops(S)[2])
    assert rc == abi.OK and bare["grad"] is None and all(np.array_equal(bare[k], want[k]) for k in ("theta_new", "sigma_r", "count", "used", "kept"))


def test_a_larger_floor_and_a_zero_step(torch_mod, device_directions):
    """sigma_floor above every deviation binds in every population; step_size 0 keeps theta and still reports grad."""
    M, S, D = 5, 64, 10
    c = crafted_es(M, S, D, np.float64)
    delta = device_directions[(M, S, D, abi.F64)][1]
    for kw in (dict(sigma_floor=100.0), dict(step_size=0.0), dict(sigma_floor=0.0)):
        rc, err, got = update(torch_mod, abi.F64, M, S, D, c["returns"], c["theta"], 7, **kw)
        want = restate_update(c["returns"], c["theta"], delta, S=S, dtype=np.float64, top=7, **kw)
        assert rc == abi.OK and all(np.array_equal(got[k], want[k], equal_nan=k in ("theta_new", "grad")) for k in want), kw
    # (floor 0: the population whose returns are all equal divides 0 by 0, as the header says; the others do not notice)
    assert (want["sigma_r"][[FLAT, NONE_VALID]] == 0).all() and np.isnan(want["grad"][FLAT]).all() and np.isfinite(want["theta_new"][[0, 1, 2, 4]]).all()


def test_refusals_on_the_device(torch_mod):
    M, S, D = 3, 65, 10
    c = crafted_es(M, S, D, np.float64)
    rc, err, weights, delta = perturb(torch_mod, abi.F64, M, S, D, c["theta"], device=1000)
    assert rc == abi.ERR_NO_DEVICE and err.startswith(b"os2ra_es_perturb: ") and weights is None and delta is None
    rc, err, weights, delta = perturb(torch_mod, abi.F64, M, S, D, c["theta"], nu=float("nan"))
    assert rc == abi.ERR_INVALID and err == b"os2ra_es_perturb: nu must be finite" and weights is None
    rc, err, out = update(torch_mod, abi.F64, M, S, D, c["returns"], c["theta"], 3, device=1000)
    assert rc == abi.ERR_NO_DEVICE and err.startswith(b"os2ra_es_update: ") and all(v is None for v in out.values())
    rc, err, out = update(torch_mod, abi.F64, M, S, D, c["returns"], c["theta"], 3, step_size=-1.0)
    assert rc == abi.ERR_INVALID and err == b"os2ra_es_update: step_size must be >= 0" and all(v is None for v in out.values())
    rc, err, out = update(torch_mod, abi.F64, M, S, D, c["returns"], c["theta"], -1)
    assert rc == abi.ERR_INVALID and err == b"os2ra_es_update: top must be >= 0" and all(v is None for v in out.values())


# ---------------------------------------------------------------------------------------
# the HipSim methods: the _into forms, and the real consumer
# ---------------------------------------------------------------------------------------
M_REAL, S_REAL, K_REAL = 3, 8, 20
N_REAL = 2 * S_REAL * M_REAL


def _cpu(t):
    return t.detach().cpu().numpy().copy()


def _handle():
    from gym_os2r_amd.sim import HipSim
    return HipSim(make_config("free_hip", "BalancingV2", False, num_envs=N_REAL, contact=True, seed=5, auto_reset=True, dtype=abi.F64)[0])


def test_into_forms_allocate_nothing_and_write_what_was_asked(torch_mod):
    torch = torch_mod
    sim = _handle()
    D, dev, i32 = sim.D, sim.device, torch.int32
    M, S = 5, 64
    SM = S * M
    c = crafted_es(M, S, D, np.float64)
    theta, returns = torch.as_tensor(c["theta"]).to(dev), torch.as_tensor(c["returns"]).to(dev)
    z = lambda *s, dtype=sim.dtype: torch.full(s, -3, dtype=dtype, device=dev)
    weights, delta = z(2 * SM, 2, D + 1), z(SM, 2, D + 1)
    theta_new, sigma_r, count, used, kept = z(M, 2, D + 1), z(M), z(M, dtype=i32), z(M, dtype=i32), z(SM, dtype=i32)
    grad, score = z(M, 2, D + 1), z(SM)
    sim.es_perturb_into(theta, weights, directions=S, nu=NU, generation=4, delta=delta)          # (the loader and the layout, once)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    sim.es_perturb_into(theta, weights, directions=S, nu=NU, generation=4)
    sim.es_update_into(returns, theta, theta_new, sigma_r, count, used, kept, directions=S, generation=4, step_size=STEP)
    sim.es_update_into(returns, theta, theta_new, sigma_r, count, used, kept, directions=S, generation=4, step_size=STEP, top=9, score=score)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before
    assert (grad == -3).all()                                                        # not asked for, not written
    want = restate_update(c["returns"], c["theta"], _cpu(delta), S=S, dtype=np.float64, top=9)
    for have, name in ((theta_new, "theta_new"), (sigma_r, "sigma_r"), (count, "count"), (used, "used"), (kept, "kept")):
        assert np.array_equal(_cpu(have), want[name]), name
    # the allocating forms return the same bits; seed None is the handle's seed
    w2, d2 = sim.es_perturb(theta, S, NU, 4, want_delta=True)
    w3, none = sim.es_perturb(theta, S, NU, 4, seed=int(sim.cfg.seed))
    assert none is None and torch.equal(w2, weights) and torch.equal(w3, weights) and torch.equal(d2, delta)
    out = sim.es_update(returns, theta, S, 4, STEP, top=9, want_grad=True, want_kept=True)
    assert len(out) == 6 and torch.equal(out[0], theta_new) and torch.equal(out[1], sigma_r) and torch.equal(out[2], count) and torch.equal(out[3], used)
    assert np.array_equal(_cpu(out[4]), want["grad"]) and torch.equal(out[5], kept)
    bare = sim.es_update(returns, theta, S, 4, STEP)
    assert bare[4] is None and bare[5] is None and not torch.equal(bare[0], theta_new)
    # top = 0 leaves the scratch alone
    score.fill_(-3)
    sim.es_update_into(returns, theta, theta_new, sigma_r, count, used, kept, directions=S, generation=4, step_size=STEP, top=S, score=score)
    torch.cuda.synchronize()
    assert (score == -3).all() and torch.equal(theta_new, bare[0])
    sim.close()


def test_real_consumer_perturb_rollout_update(torch_mod):
    """M = 3 populations x S = 8 directions on a handle of 48 environments, K = 20 steps: the returns of rollout_policy on
    es_perturb's weights equal, bit for bit, those of a twin handle on theta +- nu delta built in torch from the returned
    delta; es_update on them matches the restatement, and theta_new goes into the next generation as it is."""
    torch = torch_mod
    a, b = _handle(), _handle()
    D, dev = a.D, a.device
    rng = np.random.default_rng(11)
    theta = torch.as_tensor(rng.normal(0, 0.3, (M_REAL, 2, D + 1))).to(dev)
    nu, gen, off = 0.05, 7, 40
    weights, delta = a.es_perturb(theta, S_REAL, nu, gen, pop_offset=off, want_delta=True)
    assert tuple(weights.shape) == (N_REAL, 2, D + 1) and tuple(delta.shape) == (S_REAL * M_REAL, 2, D + 1)
    moved = nu * delta                                                                # the product, rounded on its own
    tiled = theta.repeat(S_REAL, 1, 1)                                                # row s M + m is theta[m]
    by_hand = torch.cat([tiled + moved, tiled - moved])
    assert torch.equal(by_hand, weights)
    a.reset()
    b.reset()
    ret, length, _ = a.rollout_policy(K_REAL, weights, first_episode=True)
    ret_b, length_b, _ = b.rollout_policy(K_REAL, by_hand, first_episode=True)
    torch.cuda.synchronize()
    assert np.array_equal(_cpu(ret).view(np.uint64), _cpu(ret_b).view(np.uint64)) and torch.equal(length, length_b)
    assert np.isfinite(_cpu(ret)).all() and not np.array_equal(_cpu(ret)[:N_REAL // 2], _cpu(ret)[N_REAL // 2:])   # plus and minus lanes differ
    theta_new, sigma_r, count, used, grad, kept = a.es_update(ret, theta, S_REAL, gen, STEP, top=3, pop_offset=off, want_grad=True, want_kept=True)
    torch.cuda.synchronize()
    want = restate_update(_cpu(ret), _cpu(theta), _cpu(delta), S=S_REAL, dtype=np.float64, top=3)
    for have, name in ((theta_new, "theta_new"), (sigma_r, "sigma_r"), (count, "count"), (used, "used"), (grad, "grad"), (kept, "kept")):
        assert np.array_equal(_cpu(have), want[name]), name
    assert _cpu(count).tolist() == [S_REAL] * M_REAL and _cpu(used).tolist() == [3] * M_REAL and (_cpu(sigma_r) > 0).all()
    assert not torch.equal(theta_new, theta)
    # the next generation: other directions, and theta_new goes in as it is
    w2, _ = a.es_perturb(theta_new, S_REAL, nu, gen + 1, pop_offset=off)
    a.reset()
    ret2, _, _ = a.rollout_policy(K_REAL, w2, first_episode=True)
    torch.cuda.synchronize()
    assert np.isfinite(_cpu(ret2)).all() and not torch.equal(w2 - theta_new.repeat(2 * S_REAL, 1, 1), weights - theta.repeat(2 * S_REAL, 1, 1))
    a.close(); b.close()
