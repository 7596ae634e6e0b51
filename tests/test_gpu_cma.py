"""os2rk_cma_sample and os2rk_cma_update on the device (libos2r_cma.so, include/os2r_cma.h): the normals against Box-Muller on the
oracle's uniform2 with the documented counter words; factor, failed and weights bit for bit against the numpy restatement of
tests/test_cma_host.py fed with the device's own normals; growth within 8 ulp of numpy's exp, and every other output of the update
bit for bit against the restatement fed with those normals and that growth -- which proves that the update regenerated the bits the
sample call used --, with NaN and infinite returns, ties, -0 and +0, too few valid lanes, factors that fail at column 0 and later,
a step size of 0, a stalled path and a step size clamped at either bound; the `_into` forms (no allocation, nothing written that was
not asked for); refusals that write nothing; and the calls around their real consumer: cma_sample -> rollout_policy -> cma_update
for three generations on a handle of 16 environments."""
import ctypes

import numpy as np
import pytest

from gym_os2r_amd import abi
from helpers import make_config
from test_cma_host import (CLAMPED_HIGH, CLAMPED_LOW, SHAPES, SIGMA_MAX, SIGMA_MIN, STALLED, STATE, cpu_normals, crafted_cma, restate_sample,
                           restate_update, role)

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
SEED, OFFSET, GENERATION = 0x1234567890abcdef, 2 ** 32 - 100, 2 ** 32 - 1
# Device libm and numpy differ in the last bits of log, sin and cos.  The normals are the device normal2 the exploration noise and
# the evolution-strategy directions are drawn with, whose distance from numpy was measured on the MI355X as
# max |dE| / max(|E|, 1) = 2.454e-16 (tests/test_gpu_policy_noise.py); the bound is 8 x that, as in tests/test_gpu_es.py
# (anything above 1e-12 would be a wrong stream or a float evaluation).
NOISE_STREAM_TOL = 8 * 2.454e-16
EXP_ULP = 8                                           # include/os2r_cma.h, step 8
SAMPLE_OUTPUTS = ("factor", "failed", "weights", "z")
UPDATE_OUTPUTS = ("mean", "sigma", "cov", "p_sigma", "p_c", "count", "status", "rank", "yw", "ps_norm", "growth")   # the header's order
INTEGER = ("failed", "count", "status", "rank")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _np(dtype):
    return np.float64 if dtype == abi.F64 else np.float32


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


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


def _dev(torch, a, dtype):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, _np(dtype)))).to("cuda:0")


def sample(torch, dtype, M, S, D, c, *, seed=SEED, offset=OFFSET, generation=GENERATION, want_z=True, device=0, flags=0):
    """One os2rk_cma_sample call through ctypes -> (status, error text, dict of the outputs on the host)."""
    from gym_os2r_amd import cma, control
    real = torch.float64 if dtype == abi.F64 else torch.float32
    E = 2 * (D + 1)
    g = Guarded(torch, real, dict(factor=(M, E, E), failed=(M,), weights=(S * M, 2, D + 1), z=(S * M, 2, D + 1)))
    ins = [_dev(torch, c[k], dtype) for k in ("mean", "sigma", "cov")]
    lay = control.layout(dtype, 3, device, [-1] * D)
    lib = cma.load()
    rc = lib.os2rk_cma_sample(ctypes.byref(lay), M, S, flags, seed, offset, generation, *[_p(t) for t in ins], g.ptr("factor"), g.ptr("failed"),
                              g.ptr("weights"), g.ptr("z") if want_z else None, None)
    err = lib.os2rk_last_error()
    torch.cuda.synchronize()
    return rc, err, {name: g.out(name, rc == abi.OK and (name != "z" or want_z)) for name in SAMPLE_OUTPUTS}


def update(torch, dtype, M, S, D, c, factor, failed, *, seed=SEED, offset=OFFSET, generation=GENERATION, wanted=("yw", "ps_norm", "growth"),
           device=0, consts=None, mu=None):
    """One os2rk_cma_update call through ctypes -> (status, error text, dict of the outputs on the host); an output that was not
    asked for must still hold its sentinel."""
    from gym_os2r_amd import cma, control
    real = torch.float64 if dtype == abi.F64 else torch.float32
    E, SM = 2 * (D + 1), S * M
    g = Guarded(torch, real, dict(mean=(M, 2, D + 1), sigma=(M,), cov=(M, E, E), p_sigma=(M, E), p_c=(M, E), count=(M,), status=(M,), rank=(SM,),
                                  yw=(M, 2, D + 1), ps_norm=(M,), growth=(M,)))
    ins = [_dev(torch, c[k], dtype) for k in ("returns", "rankw") + STATE] + [_dev(torch, factor, dtype), torch.as_tensor(np.asarray(failed, np.int32)).to("cuda:0")]
    lay = control.layout(dtype, 3, device, [-1] * D)
    lib = cma.load()
    opt = lambda name: g.ptr(name) if name in wanted else None
    rc = lib.os2rk_cma_update(ctypes.byref(lay), M, S, len(c["rankw"]) if mu is None else mu, 0, seed, offset, generation, *[_p(t) for t in ins],
                              ctypes.byref(consts or c["consts"]), *[g.ptr(k) for k in UPDATE_OUTPUTS[:8]], opt("yw"), opt("ps_norm"), opt("growth"), None)
    err = lib.os2rk_last_error()
    torch.cuda.synchronize()
    return rc, err, {name: g.out(name, rc == abi.OK and (name in UPDATE_OUTPUTS[:8] or name in wanted)) for name in UPDATE_OUTPUTS}


@pytest.fixture(scope="module")
def device_samples(torch_mod):
    """The crafted populations of every shape, D and dtype with what cma_sample made of them; made once and left unchanged."""
    made = {}
    for (M, S) in SHAPES:
        for D in (10, 3):
            for dtype in (abi.F64, abi.F32):
                c = crafted_cma(M, S, D, _np(dtype))
                rc, err, out = sample(torch_mod, dtype, M, S, D, c)
                assert rc == abi.OK, (M, S, D, dtype, err)
                made[(M, S, D, dtype)] = (c, out)
    return made


# ---------------------------------------------------------------------------------------
# the stream
# ---------------------------------------------------------------------------------------
def test_normals_are_stream_7_of_the_counter_rng(torch_mod, device_samples, oracle):
    """f64: z against Box-Muller on the oracle's uniform2(seed, (pop_offset + m) mod 2^32, 7, generation, 16 s + (e >> 1)) at a
    pop_offset that wraps inside the 257 populations and generation 2^32 - 1.  f32: the same normals rounded once to float, bit
    for bit.  A different generation, population, sample or seed is a different draw; pop_offset = a at population m is
    pop_offset = 0 at population a + m."""
    from gym_os2r_amd import cma, es
    assert cma.STREAM == 7 == es.STREAM + 1
    worst = 0.0
    for (M, S, D) in ((3, 65, 10), (257, 4, 10), (5, 64, 3), (1, 2, 3)):
        z64, z32 = device_samples[(M, S, D, abi.F64)][1]["z"], device_samples[(M, S, D, abi.F32)][1]["z"]
        ref = cpu_normals(oracle, SEED, OFFSET, GENERATION, M, S, D)
        worst = max(worst, float(np.max(np.abs(z64 - ref) / np.maximum(np.abs(ref), 1.0))))
        assert z32.dtype == np.float32 and np.array_equal(_bits(z32), _bits(z64.astype(np.float32))), (M, S, D)
    print(f"[cma stream] max |dz| / max(|z|, 1) = {worst:.3e} (bound {NOISE_STREAM_TOL:.3e})")
    assert worst <= NOISE_STREAM_TOL <= 1e-12, worst
    M, S, D = 3, 65, 10
    c, out = device_samples[(M, S, D, abi.F64)]
    base = out["z"].reshape(S, M, 2, D + 1)
    other = sample(torch_mod, abi.F64, M, S, D, c, generation=GENERATION - 1)[2]["z"].reshape(base.shape)
    assert np.max(np.abs(other - base)) > 1.0                                        # another generation
    assert np.max(np.abs(base[:, 1] - base[:, 0])) > 1.0 and np.max(np.abs(base[1] - base[0])) > 1.0   # another population, sample
    assert np.max(np.abs(sample(torch_mod, abi.F64, M, S, D, c, seed=SEED + 1)[2]["z"].reshape(base.shape) - base)) > 1.0
    # a shard: populations a .. a + M - 1 of a call at pop_offset 0 are those of a call at pop_offset a
    a = 2
    wide = {k: np.concatenate([c[k][:a], c[k]]) for k in ("mean", "sigma", "cov")}
    for dtype in (abi.F64, abi.F32):
        w = sample(torch_mod, dtype, a + M, S, D, wide, offset=0)[2]
        s = sample(torch_mod, dtype, M, S, D, c, offset=a)[2]
        assert np.array_equal(w["z"].reshape(S, a + M, -1)[:, a:], s["z"].reshape(S, M, -1))
        assert np.array_equal(w["weights"].reshape(S, a + M, -1)[:, a:], s["weights"].reshape(S, M, -1))


# ---------------------------------------------------------------------------------------
# the factor and the samples
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("D", [10, 3])
def test_factor_failed_and_weights_against_the_restatement(torch_mod, device_samples, D, dtype):
    """factor, failed and weights equal the restatement on the device's own normals, bit for bit, crafted populations included: a
    failed population has a zero factor and the mean in every lane.  Without z_dev the other outputs are the same and nothing
    else is written."""
    E = 2 * (D + 1)
    for (M, S) in SHAPES:
        c, out = device_samples[(M, S, D, dtype)]
        want = restate_sample(c, out["z"], S=S, dtype=_np(dtype))
        for name in ("factor", "failed", "weights"):
            assert out[name].dtype == want[name].dtype and np.array_equal(out[name], want[name]), (M, S, name, np.argwhere(out[name] != want[name])[:4])
        assert np.isfinite(out["weights"]).all() and (np.triu(out["factor"], 1) == 0).all()
        bad = np.flatnonzero(out["failed"])
        assert (out["factor"][bad] == 0).all()
        assert np.array_equal(out["weights"].reshape(S, M, E)[:, bad], np.broadcast_to(c["mean"].reshape(1, M, E)[:, bad], (S, len(bad), E)))
        if M >= 5:
            assert set(out["failed"].tolist()) == {0, 1, 4, E + 1}
    M, S = SHAPES[3]
    c, out = device_samples[(M, S, D, dtype)]
    rc, err, bare = sample(torch_mod, dtype, M, S, D, c, want_z=False)
    assert rc == abi.OK and bare["z"] is None and all(np.array_equal(bare[k], out[k]) for k in ("factor", "failed", "weights"))


# ---------------------------------------------------------------------------------------
# the update
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("D", [10, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_of_the_update_against_the_restatement(torch_mod, device_samples, shape, D, dtype):
    """growth is within 8 ulp of numpy's exp of the restatement's argument; mean, sigma, cov, p_sigma, p_c, count, status, rank, yw
    and ps_norm equal the restatement on the device's own normals and growth, bit for bit: the update regenerated the bits the
    sample call used.  Where status is not 0 the state outputs are the inputs, bit for bit (NaNs above the diagonal included)."""
    M, S = shape
    real = _np(dtype)
    c, smp = device_samples[(M, S, D, dtype)]
    rc, err, got = update(torch_mod, dtype, M, S, D, c, smp["factor"], smp["failed"])
    assert rc == abi.OK, err
    own = restate_update(c["returns"], c["rankw"], c, smp["factor"], smp["failed"], smp["z"], c["consts"], S=S, dtype=real)
    ran = own["status"] == 0
    ulps = np.abs(got["growth"][ran].astype(np.float64) - own["growth"][ran]) / np.spacing(np.abs(own["growth"][ran])).astype(np.float64)
    print(f"[cma growth] {shape} D={D} {real.__name__}: at most {ulps.max() if ulps.size else 0:.1f} ulp from numpy's exp")
    assert (ulps <= EXP_ULP).all(), ulps.max()
    want = restate_update(c["returns"], c["rankw"], c, smp["factor"], smp["failed"], smp["z"], c["consts"], S=S, dtype=real, growth=got["growth"])
    for name in ("count", "status", "rank"):
        assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), (shape, D, name, np.argwhere(got[name] != want[name])[:4])
    for name in ("mean", "sigma", "cov", "p_sigma", "p_c", "yw", "ps_norm", "growth"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name][ran], want[name][ran]), \
            (shape, D, name, np.argwhere(got[name][ran] != want[name][ran])[:4])
    assert np.array_equal(got["cov"][ran], np.swapaxes(got["cov"][ran], 1, 2)) and np.isfinite(got["cov"][ran]).all()
    stay = ~ran
    for name in STATE:
        assert np.array_equal(_bits(got[name][stay]), _bits(c[name][stay])), (shape, D, name)
    assert (got["yw"][stay] == 0).all() and (got["ps_norm"][stay] == 0).all() and (got["growth"][stay] == 1).all()
    assert ran.any() and sorted(got["rank"].reshape(S, M)[:, 0].tolist()) == list(range(S))
    if M >= 5:
        assert set(got["status"].tolist()) == {0, 1, 2}
    if M > 8:                                                                        # every role: the stalled path, the clamps
        roles = np.array([role(m, M) for m in range(M)])
        assert not want["h"][ran & (roles == STALLED)].any() and (got["sigma"][roles == CLAMPED_HIGH] == real(SIGMA_MAX)).all()
        assert (got["sigma"][roles == CLAMPED_LOW] == real(SIGMA_MIN)).sum() > (roles == CLAMPED_LOW).sum() // 2
    # without the optional outputs the others are the same and those are not written
    rc, err, bare = update(torch_mod, dtype, M, S, D, c, smp["factor"], smp["failed"], wanted=())
    assert rc == abi.OK and bare["yw"] is None and bare["ps_norm"] is None and bare["growth"] is None
    assert all(np.array_equal(_bits(bare[k]), _bits(got[k])) for k in UPDATE_OUTPUTS[:8])


def test_fewer_parents_and_other_constants(torch_mod, device_samples):
    """mu = 1 and mu = S, and constants without covariance learning: the restatement still holds."""
    from gym_os2r_amd import cma
    M, S, D = 3, 65, 10
    E = 2 * (D + 1)
    c, smp = device_samples[(M, S, D, abi.F64)]
    for mu, kw in ((1, {}), (S, {}), (7, dict(c_1=0.0, c_mu=0.0, k0_moving=1.0, k0_stalled=1.0))):
        rankw, consts = cma.constants(E, S, parents=mu, age=0)
        for name, v in kw.items():
            setattr(consts, name, v)
        cc = dict(c, rankw=np.asarray(rankw), consts=consts)
        rc, err, got = update(torch_mod, abi.F64, M, S, D, cc, smp["factor"], smp["failed"])
        assert rc == abi.OK, err
        want = restate_update(c["returns"], rankw, c, smp["factor"], smp["failed"], smp["z"], consts, S=S, dtype=np.float64, growth=got["growth"])
        ran = want["status"] == 0
        for name in UPDATE_OUTPUTS:
            full = name in ("count", "status", "rank")
            assert np.array_equal(got[name] if full else got[name][ran], want[name] if full else want[name][ran]), (mu, name)
        # (the second population has one valid lane, the third no factor; with mu = S the invalid lanes make count < mu in the first too)
        assert got["status"].tolist() == [1 if mu == S else 0, 0 if mu == 1 else 1, 2]
    assert np.array_equal(np.tril(got["cov"]), np.tril(c["cov"]))                   # no learning rate, no change


def test_refusals_on_the_device(torch_mod, device_samples):
    M, S, D = 3, 65, 10
    c, smp = device_samples[(M, S, D, abi.F64)]
    rc, err, out = sample(torch_mod, abi.F64, M, S, D, c, device=1000)
    assert rc == abi.ERR_NO_DEVICE and err.startswith(b"os2rk_cma_sample: ") and all(v is None for v in out.values())
    rc, err, out = sample(torch_mod, abi.F64, M, S, D, c, flags=4)
    assert rc == abi.ERR_INVALID and err == b"os2rk_cma_sample: unknown flag bits" and all(v is None for v in out.values())
    rc, err, out = update(torch_mod, abi.F64, M, S, D, c, smp["factor"], smp["failed"], device=1000)
    assert rc == abi.ERR_NO_DEVICE and err.startswith(b"os2rk_cma_update: ") and all(v is None for v in out.values())
    rc, err, out = update(torch_mod, abi.F64, M, S, D, c, smp["factor"], smp["failed"], mu=S + 1)
    assert rc == abi.ERR_INVALID and err == b"os2rk_cma_update: mu must be <= nsamples" and all(v is None for v in out.values())
    from gym_os2r_amd import cma
    broken = cma.Os2rkCmaConstants.from_buffer_copy(c["consts"])
    broken.chi = float("inf")
    rc, err, out = update(torch_mod, abi.F64, M, S, D, c, smp["factor"], smp["failed"], consts=broken)
    assert rc == abi.ERR_INVALID and err == b"os2rk_cma_update: constants->chi must be finite" and all(v is None for v in out.values())


# ---------------------------------------------------------------------------------------
# the HipSim methods: the _into forms, and the real consumer
# ---------------------------------------------------------------------------------------
M_REAL, S_REAL, K_REAL, GENERATIONS = 2, 8, 20, 3
AGE_REAL = 2                                          # of the update of the allocating form: not the generation
N_REAL = S_REAL * M_REAL


def _cpu(t):
    return t.detach().cpu().numpy().copy()


def _handle():
    from gym_os2r_amd.sim import HipSim
    return HipSim(make_config("free_hip", "BalancingV2", False, num_envs=N_REAL, contact=True, seed=5, auto_reset=True, dtype=abi.F64)[0])


def test_into_forms_allocate_nothing_and_write_what_was_asked(torch_mod):
    torch = torch_mod
    from gym_os2r_amd import cma
    sim = _handle()
    D, dev, i32 = sim.D, sim.device, torch.int32
    M, S = 5, 64
    E, N = 2 * (D + 1), S * M
    c = crafted_cma(M, S, D, np.float64)
    state = tuple(torch.as_tensor(c[k]).to(dev) for k in STATE)
    returns, rankw = torch.as_tensor(c["returns"]).to(dev), torch.as_tensor(c["rankw"]).to(dev)
    z = lambda *s, dtype=sim.dtype: torch.full(s, -3, dtype=dtype, device=dev)
    factor, failed, weights, normals = z(M, E, E), z(M, dtype=i32), z(N, 2, D + 1), z(N, 2, D + 1)
    new = (z(M, 2, D + 1), z(M), z(M, E, E), z(M, E), z(M, E))
    count, status, rank = z(M, dtype=i32), z(M, dtype=i32), z(N, dtype=i32)
    yw, ps_norm, growth = z(M, 2, D + 1), z(M), z(M)
    sim.cma_sample_into(state, factor, failed, weights, samples=S, generation=4, z=normals)            # (the loader and the layout, once)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    sim.cma_sample_into(state, factor, failed, weights, samples=S, generation=4)
    sim.cma_update_into(returns, state, factor, failed, new, count, status, rank, samples=S, generation=4, rankw=rankw, constants=c["consts"])
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before
    assert (yw == -3).all() and (ps_norm == -3).all() and (growth == -3).all()       # not asked for, not written
    sim.cma_update_into(returns, state, factor, failed, new, count, status, rank, samples=S, generation=4, rankw=rankw, constants=c["consts"],
                        growth=growth)
    torch.cuda.synchronize()
    assert (yw == -3).all() and (ps_norm == -3).all() and not (growth == -3).any()
    smp = restate_sample(c, _cpu(normals), S=S, dtype=np.float64)
    assert np.array_equal(_cpu(factor), smp["factor"]) and np.array_equal(_cpu(failed), smp["failed"]) and np.array_equal(_cpu(weights), smp["weights"])
    want = restate_update(c["returns"], c["rankw"], c, smp["factor"], smp["failed"], _cpu(normals), c["consts"], S=S, dtype=np.float64, growth=_cpu(growth))
    ran = want["status"] == 0
    for have, name in zip(new, STATE):
        assert np.array_equal(_cpu(have)[ran], want[name][ran]) and np.array_equal(_bits(_cpu(have)[~ran]), _bits(c[name][~ran])), name
    for have, name in ((count, "count"), (status, "status"), (rank, "rank")):
        assert np.array_equal(_cpu(have), want[name]), name
    # the allocating forms return the same bits; seed None is the handle's seed
    w2, f2, bad2, z2 = sim.cma_sample(state, S, 4, want_z=True)
    w3, f3, bad3, none = sim.cma_sample(state, S, 4, seed=int(sim.cfg.seed))
    assert none is None and torch.equal(w2, weights) and torch.equal(w3, weights) and torch.equal(z2, normals) and torch.equal(f2, factor) and torch.equal(bad3, failed)
    plain = tuple(torch.as_tensor(c[k][:1]).to(dev) for k in STATE)                  # one population that runs, Hansen's constants
    w1, f1, bad1, z1 = sim.cma_sample(plain, S, 4, want_z=True)
    out = sim.cma_update(returns.reshape(S, M)[:, 0].contiguous(), plain, f1, bad1, S, 4, age=AGE_REAL, want_yw=True, want_norm=True, want_growth=True)
    rw, k = cma.constants(E, S, None, AGE_REAL, 1e-8, 1.0)
    one = {n: c[n][:1] for n in STATE}
    want = restate_update(c["returns"].reshape(S, M)[:, 0], rw, one, _cpu(f1), _cpu(bad1), _cpu(z1), k, S=S, dtype=np.float64, growth=_cpu(out[6]))
    assert len(out) == 7 and len(out[0]) == 5 and all(np.array_equal(_cpu(t), want[n]) for t, n in zip(out[0], STATE))
    assert all(np.array_equal(_cpu(t), want[n]) for t, n in zip(out[1:], ("count", "status", "rank", "yw", "ps_norm", "growth")))
    bare = sim.cma_update(returns.reshape(S, M)[:, 0].contiguous(), plain, f1, bad1, S, 4, age=AGE_REAL)
    assert bare[4] is None and bare[5] is None and bare[6] is None and all(torch.equal(a, b) for a, b in zip(bare[0], out[0]))
    sim.close()


def test_real_consumer_sample_rollout_update(torch_mod):
    """M = 2 populations x S = 8 samples on a handle of 16 environments, K = 20 steps, three generations: the returns of
    rollout_policy on cma_sample's weights equal, bit for bit, those of a twin handle given the restatement's weights; the state
    after every cma_update equals the restatement's, and goes into the next generation as it is."""
    torch = torch_mod
    from gym_os2r_amd import cma
    a, b = _handle(), _handle()
    D, dev = a.D, a.device
    E = 2 * (D + 1)
    rng = np.random.default_rng(11)
    theta = torch.as_tensor(rng.normal(0, 0.3, (M_REAL, 2, D + 1))).to(dev)
    off = 40
    state = a.cma_init(theta, 0.1)
    host = dict(zip(STATE, (_cpu(t) for t in state)))
    assert np.array_equal(host["cov"], np.tile(np.eye(E), (M_REAL, 1, 1))) and (host["p_sigma"] == 0).all() and (host["sigma"] == 0.1).all()
    for gen in range(GENERATIONS):
        weights, factor, failed, z = a.cma_sample(state, S_REAL, gen, pop_offset=off, want_z=True)
        assert tuple(weights.shape) == (N_REAL, 2, D + 1) and _cpu(failed).tolist() == [0] * M_REAL
        smp = restate_sample(host, _cpu(z), S=S_REAL, dtype=np.float64)
        assert np.array_equal(_cpu(weights), smp["weights"]) and np.array_equal(_cpu(factor), smp["factor"])
        a.reset()
        b.reset()
        ret, length, _ = a.rollout_policy(K_REAL, weights, first_episode=True)
        ret_b, length_b, _ = b.rollout_policy(K_REAL, torch.as_tensor(smp["weights"]).to(dev), first_episode=True)
        torch.cuda.synchronize()
        assert np.array_equal(_cpu(ret).view(np.uint64), _cpu(ret_b).view(np.uint64)) and torch.equal(length, length_b)
        assert np.isfinite(_cpu(ret)).all() and len(set(_cpu(ret).tolist())) > N_REAL // 2
        state, count, status, rank, yw, ps_norm, growth = a.cma_update(ret, state, factor, failed, S_REAL, gen, pop_offset=off, want_yw=True,
                                                                       want_norm=True, want_growth=True)
        torch.cuda.synchronize()
        rankw, k = cma.constants(E, S_REAL, None, gen, 1e-8, 1.0)
        want = restate_update(_cpu(ret), rankw, host, smp["factor"], smp["failed"], _cpu(z), k, S=S_REAL, dtype=np.float64, growth=_cpu(growth))
        for have, name in zip(state, STATE):
            assert np.array_equal(_cpu(have), want[name]), (gen, name)
        for have, name in ((count, "count"), (status, "status"), (rank, "rank"), (yw, "yw"), (ps_norm, "ps_norm")):
            assert np.array_equal(_cpu(have), want[name]), (gen, name)
        assert _cpu(count).tolist() == [S_REAL] * M_REAL and _cpu(status).tolist() == [0] * M_REAL
        assert not np.array_equal(want["mean"], host["mean"]) and not np.array_equal(want["cov"], host["cov"])
        host = {name: want[name] for name in STATE}
    a.close(); b.close()
