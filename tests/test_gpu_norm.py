"""os2rz_obs_stats, os2rz_fold and os2rz_unfold on the device (libos2r_norm.so, include/os2r_norm.h): every output of the
statistics bit for bit against the numpy restatement of tests/test_norm_host.py, scratch included, for shapes that cross a wave
inside a lane's D threads, the 64-partial boundary and a policy count that is a multiple of nothing, on crafted inputs (lengths
of 0, below 0, above K and null; a NaN and an infinity inside a length and beyond it; a policy without a valid lane; a NaN at
the pivot; empty and non-empty states; obs0 given and null); the fold and the unfold in both layouts, per lane and per policy,
bit for bit; the `_into` forms (no allocation, nothing written that was not asked for); refusals that write nothing; and the
calls around their real consumer, an ARS V2 generation on a handle of 48 environments."""
import ctypes

import numpy as np
import pytest

from gym_os2r_amd import abi
from helpers import make_config
from test_norm_host import FLOOR, crafted_obs, restate_fold, restate_stats, restate_unfold

pytestmark = pytest.mark.gpu

PAD, MARK, IMARK = 64, -12345.5, -77
SHAPES = [(1, 1), (3, 65), (5, 64), (257, 2), (1, 130)]      # (P, S)
STEPS = (1, 7, 70)
INT32, INT64 = ("steps", "valid", "lane_count"), ("count",)
STATS_OUTPUTS = ("count", "mean", "m2", "steps", "valid", "lane_sum", "lane_count")   # the header's order


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
        kind = lambda k: torch.int32 if k in INT32 else (torch.int64 if k in INT64 else real)
        self.marks = {k: MARK if kind(k) is real else IMARK for k in shapes}
        self.bufs = {k: torch.full((PAD + n + PAD,), self.marks[k], dtype=kind(k), device="cuda:0") for k, n in self.sizes.items()}

    def ptr(self, name):
        return _p(self.bufs[name][PAD:])

    def out(self, name, written=True):
        host = self.bufs[name].cpu().numpy()
        mark, n = self.marks[name], self.sizes[name]
        assert (host[:PAD] == mark).all() and (host[PAD + n:] == mark).all(), f"{name}: written outside"
        if not written:
            assert (host[PAD:PAD + n] == mark).all(), f"{name}: written although not asked for"
            return None
        return host[PAD:PAD + n].reshape(self.shapes[name])


def _dev(torch, a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to("cuda:0")


def stats(torch, dtype, P, S, K, D, obs, *, obs0=None, length=None, state=None, want_counts=True, device=0, flags=0):
    """One os2rz_obs_stats call through ctypes -> (status, error text, dict of the outputs on the host); an output that was not
    asked for must still hold its sentinel."""
    from gym_os2r_amd import control, norm
    real, T = (torch.float64 if dtype == abi.F64 else torch.float32), _np(dtype)
    N = S * P
    g = Guarded(torch, real, dict(count=(P,), mean=(P, D), m2=(P, D), steps=(P,), valid=(P,), lane_sum=(2 * D, N), lane_count=(2, N)))
    o, o0, ln = _dev(torch, obs, T), _dev(torch, obs0, T), _dev(torch, length, np.int32)
    st = (None,) * 3 if state is None else (_dev(torch, state[0], np.int64), _dev(torch, state[1], T), _dev(torch, state[2], T))
    lay = control.layout(dtype, 3, device, [-1] * D)
    lib = norm.load()
    rc = lib.os2rz_obs_stats(ctypes.byref(lay), K, P, S, flags, _p(o), _p(o0), _p(ln), _p(st[0]), _p(st[1]), _p(st[2]), g.ptr("count"),
                             g.ptr("mean"), g.ptr("m2"), g.ptr("steps") if want_counts else None, g.ptr("valid") if want_counts else None,
                             g.ptr("lane_sum"), g.ptr("lane_count"), None)
    err = lib.os2rz_last_error()
    torch.cuda.synchronize()
    ok = rc == abi.OK
    return rc, err, {name: g.out(name, ok and (want_counts or name not in ("steps", "valid"))) for name in STATS_OUTPUTS}


def fold(torch, dtype, P, D, source, state, *, lanes=None, fastest=False, unfold=False, std_floor=FLOOR, device=0, flags=None):
    """One os2rz_fold or os2rz_unfold call through ctypes on `source` [Q, rows, D+1] (laid out [rows, D+1, Q] on the device with
    `fastest`) -> (status, error text, the output [Q, rows, D+1] on the host | None)."""
    from gym_os2r_amd import control, norm
    real, T = (torch.float64 if dtype == abi.F64 else torch.float32), _np(dtype)
    source = np.asarray(source, T)
    Q, rows, n = source.shape
    g = Guarded(torch, real, dict(out=(rows, n, Q) if fastest else (Q, rows, n)))
    src = _dev(torch, source.transpose(1, 2, 0) if fastest else source)
    st = (None,) * 3 if state is None else (_dev(torch, state[0], np.int64), _dev(torch, state[1], T), _dev(torch, state[2], T))
    lay = control.layout(dtype, 3, device, [-1] * D)
    lib = norm.load()
    if flags is None:
        flags = (norm.POLICY_FASTEST if fastest else 0) | (norm.PER_LANE if lanes is not None else 0)
    if unfold:
        rc = lib.os2rz_unfold(ctypes.byref(lay), P, rows, flags, _p(st[0]), _p(st[1]), _p(st[2]), std_floor, _p(src), g.ptr("out"), None)
    else:
        rc = lib.os2rz_fold(ctypes.byref(lay), P, lanes or 0, rows, flags, _p(st[0]), _p(st[1]), _p(st[2]), std_floor, _p(src), g.ptr("out"), None)
    err = lib.os2rz_last_error()
    torch.cuda.synchronize()
    out = g.out("out", rc == abi.OK)
    return rc, err, (out.transpose(2, 0, 1) if fastest and out is not None else out)


def _same(got, want, where):
    for name in STATS_OUTPUTS:
        assert got[name].dtype == want[name].dtype, (where, name, got[name].dtype)
        assert np.array_equal(got[name], want[name], equal_nan=name == "lane_sum"), (where, name, np.argwhere(got[name] != want[name])[:4])


# ---------------------------------------------------------------------------------------
# the statistics
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("D", [10, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_of_the_statistics_against_the_restatement(torch_mod, shape, D, dtype):
    """count, mean, m2, steps, valid and the scratch equal the restatement for K in {1, 7, 70}: first with obs0, the crafted
    lengths and an empty state (the pivot is the first observation; 0 where that is a NaN), then the same batch without obs0
    and without lengths merged into the state the first call returned (the pivot is the running mean; a policy without a valid
    lane passes its state on)."""
    P, S = shape
    T = _np(dtype)
    for K in STEPS:
        c = crafted_obs(P, S, K, D, T)
        rc, err, got = stats(torch_mod, dtype, P, S, K, D, c["obs"], obs0=c["obs0"], length=c["length"])
        assert rc == abi.OK, (K, err)
        want = restate_stats(c["obs"], P=P, dtype=T, obs0=c["obs0"], length=c["length"])
        _same(got, want, (shape, D, K, "empty"))
        if S > 3:
            assert want["valid"].max() > 0 and (want["lane_count"][1] == 0).any() and np.isfinite(want["mean"]).all()
        if P > 2:
            assert want["valid"][2] == 0 == want["count"][2] and want["count"][0] > 0
        state = (got["count"], got["mean"], got["m2"])
        rc, err, again = stats(torch_mod, dtype, P, S, K, D, c["obs"], state=state)
        assert rc == abi.OK, (K, err)
        want = restate_stats(c["obs"], P=P, dtype=T, state=state)
        _same(again, want, (shape, D, K, "merged"))
        assert (again["lane_count"][0] == K).all()
        if P > 2:
            assert again["count"][2] == 0 and (again["count"][[0, 1]] >= state[0][[0, 1]]).all()
    # without steps_dev and valid_dev the state is the same and neither is written; a length alone, and obs0 alone
    rc, err, bare = stats(torch_mod, dtype, P, S, K, D, c["obs"], state=state, want_counts=False)
    assert rc == abi.OK and bare["steps"] is None and bare["valid"] is None and all(np.array_equal(bare[k], again[k]) for k in ("count", "mean", "m2"))
    rc, err, got = stats(torch_mod, dtype, P, S, K, D, c["obs"], length=c["length"], state=state)
    _same(got, restate_stats(c["obs"], P=P, dtype=T, length=c["length"], state=state), (shape, D, K, "length alone"))
    rc, err, got = stats(torch_mod, dtype, P, S, K, D, c["obs"], obs0=c["obs0"])
    _same(got, restate_stats(c["obs"], P=P, dtype=T, obs0=c["obs0"]), (shape, D, K, "obs0 alone"))


def test_a_state_that_is_empty_for_some_policies(torch_mod):
    """count 0 and below 0 are empty (their mean and m2 are not read), count 1 is not; a large running count in both dtypes."""
    P, S, K, D = 5, 64, 7, 10
    rng = np.random.default_rng(3)
    for dtype in (abi.F64, abi.F32):
        T = _np(dtype)
        c = crafted_obs(P, S, K, D, T)
        state = (np.array([0, 1, 9, -4, 2 ** 40 + 12345], np.int64), rng.normal(10, 30, (P, D)).astype(T), rng.uniform(1, 2, (P, D)).astype(T))
        state[1][[0, 3]] = np.nan
        rc, err, got = stats(torch_mod, dtype, P, S, K, D, c["obs"], obs0=c["obs0"], length=c["length"], state=state)
        assert rc == abi.OK, err
        want = restate_stats(c["obs"], P=P, dtype=T, obs0=c["obs0"], length=c["length"], state=state)
        _same(got, want, dtype)
        nb = [int(v) for v in want["steps"]]
        assert want["count"].tolist() == [nb[0], 1 + nb[1], 9, nb[3], 2 ** 40 + 12345 + nb[4]] and nb[2] == 0 and min(nb[0], nb[1], nb[3], nb[4]) > 0
        assert np.isfinite(want["mean"]).all() and np.array_equal(want["mean"][2], state[1][2])


# ---------------------------------------------------------------------------------------
# the fold and the unfold
# ---------------------------------------------------------------------------------------
def _a_state(P, D, T, seed=5):
    """A state with a policy that has seen one observation (the identity), an empty one where P reaches them, and a constant
    component on which std_floor binds."""
    rng = np.random.default_rng(seed + P)
    count = rng.integers(50, 5000, P).astype(np.int64)
    mean, m2 = rng.uniform(-50, 50, (P, D)).astype(T), (rng.uniform(0.1, 5, (P, D)) ** 2 * count[:, None]).astype(T)
    m2[0, D - 1] = 0
    if P > 1:
        count[1] = 1
    if P > 3:
        count[3] = 0
    return count, mean, m2


@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("D", [10, 3])
def test_fold_and_unfold_against_the_restatements(torch_mod, D, dtype):
    """Both layouts, one and two rows, per policy and per lane (257 policies: two workgroups and a remainder), bit for bit."""
    T = _np(dtype)
    rng = np.random.default_rng(7)
    for P, lanes in ((1, None), (5, None), (257, None), (1, 130), (3, 195), (257, 514)):
        state = _a_state(P, D, T)
        Q = lanes or P
        for rows in (2, 1):
            theta = rng.normal(0, 0.5, (Q, rows, D + 1)).astype(T)
            want = restate_fold(theta, state, dtype=T)
            for fastest in (False, True):
                rc, err, got = fold(torch_mod, dtype, P, D, theta, state, lanes=lanes, fastest=fastest)
                assert rc == abi.OK, (P, lanes, rows, fastest, err)
                assert got.dtype == want.dtype and np.array_equal(got, want), (P, lanes, rows, fastest, np.argwhere(got != want)[:4])
                if lanes is None:
                    back = restate_unfold(theta, state, dtype=T)
                    rc, err, got = fold(torch_mod, dtype, P, D, theta, state, fastest=fastest, unfold=True)
                    assert rc == abi.OK and np.array_equal(got, back), (P, rows, fastest, err)
        assert np.array_equal(want[0, :, D - 1], theta[0, :, D - 1] * (T(1) / np.float64(FLOOR).astype(T)))     # the floor binds
        if P > 1:
            assert np.array_equal(want[1], theta[1]) and not np.array_equal(want[0], theta[0])              # count < 2: the identity
    # a null state is empty: everything is copied through; another floor is another scale
    rc, err, got = fold(torch_mod, dtype, 5, D, theta[:5], None)
    assert rc == abi.OK and np.array_equal(got, theta[:5])
    state = _a_state(5, D, T)
    rc, err, got = fold(torch_mod, dtype, 5, D, theta[:5], state, std_floor=3.0)
    assert rc == abi.OK and np.array_equal(got, restate_fold(theta[:5], state, dtype=T, std_floor=3.0))
    assert not np.array_equal(got, restate_fold(theta[:5], state, dtype=T))


def test_refusals_on_the_device(torch_mod):
    P, S, K, D = 3, 65, 7, 10
    c = crafted_obs(P, S, K, D, np.float64)
    none = lambda out: all(v is None for v in out.values())
    rc, err, out = stats(torch_mod, abi.F64, P, S, K, D, c["obs"], obs0=c["obs0"], device=1000)
    assert rc == abi.ERR_NO_DEVICE and err.startswith(b"os2rz_obs_stats: ") and none(out)
    rc, err, out = stats(torch_mod, abi.F64, P, S, K, D, c["obs"], obs0=c["obs0"], flags=1)
    assert rc == abi.ERR_INVALID and err == b"os2rz_obs_stats: unknown flag bits" and none(out)
    state = _a_state(P, D, np.float64)
    theta = np.ones((P, 2, D + 1))
    rc, err, out = fold(torch_mod, abi.F64, P, D, theta, state, device=1000)
    assert rc == abi.ERR_NO_DEVICE and err.startswith(b"os2rz_fold: ") and out is None
    rc, err, out = fold(torch_mod, abi.F64, P, D, theta, state, std_floor=0.0)
    assert rc == abi.ERR_INVALID and err == b"os2rz_fold: std_floor must be > 0" and out is None
    rc, err, out = fold(torch_mod, abi.F64, P, D, theta, state, unfold=True, device=1000)
    assert rc == abi.ERR_NO_DEVICE and err.startswith(b"os2rz_unfold: ") and out is None
    rc, err, out = fold(torch_mod, abi.F64, P, D, theta, state, unfold=True, std_floor=float("nan"))
    assert rc == abi.ERR_INVALID and err == b"os2rz_unfold: std_floor must be finite" and out is None
    rc, err, out = fold(torch_mod, abi.F64, P, D, theta, state, unfold=True, flags=1)
    assert rc == abi.ERR_INVALID and err == b"os2rz_unfold: OS2RZ_PER_LANE is os2rz_fold's (a gradient is per policy)" and out is None


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
    D, dev, i32, i64 = sim.D, sim.device, torch.int32, torch.int64
    P, S, K = 5, 64, 7
    N = S * P
    c = crafted_obs(P, S, K, D, np.float64)
    obs, obs0, length = (torch.as_tensor(c[k]).to(dev) for k in ("obs", "obs0", "length"))
    z = lambda *s, dtype=sim.dtype: torch.full(s, -3, dtype=dtype, device=dev)
    count, mean, m2, lane_sum, lane_count = z(P, dtype=i64), z(P, D), z(P, D), z(2 * D, N), z(2, N, dtype=i32)
    count2, mean2, m22, steps, valid = z(P, dtype=i64), z(P, D), z(P, D), z(P, dtype=i32), z(P, dtype=i32)
    theta, weights, weights_t, grad_theta = torch.as_tensor(np.random.default_rng(1).normal(0, 1, (P, 2, D + 1))).to(dev), z(P, 2, D + 1), z(2, D + 1, P), z(2, D + 1, P)
    lanes, lane_w = theta.repeat(S, 1, 1).contiguous(), z(N, 2, D + 1)
    theta_t = theta.permute(1, 2, 0).contiguous()
    sim.obs_stats_into(obs, count, mean, m2, lane_sum, lane_count, policies=P, obs0=obs0, length=length)   # (the loader and the layout, once)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    sim.obs_stats_into(obs, count2, mean2, m22, lane_sum, lane_count, policies=P, state=(count, mean, m2))
    sim.norm_fold_into(theta, (count2, mean2, m22), weights)
    sim.norm_fold_into(theta_t, (count2, mean2, m22), weights_t, policy_fastest=True)
    sim.norm_fold_into(lanes, (count2, mean2, m22), lane_w, lanes=N, std_floor=0.5)
    sim.norm_unfold_into(theta_t, (count2, mean2, m22), grad_theta, policy_fastest=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) == before
    assert (steps == -3).all() and (valid == -3).all()                               # not asked for, not written
    first = restate_stats(c["obs"], P=P, dtype=np.float64, obs0=c["obs0"], length=c["length"])
    state = (first["count"], first["mean"], first["m2"])
    for have, name in ((count, "count"), (mean, "mean"), (m2, "m2")):
        assert np.array_equal(_cpu(have), first[name]), name
    second = restate_stats(c["obs"], P=P, dtype=np.float64, state=state)
    for have, name in ((count2, "count"), (mean2, "mean"), (m22, "m2")):
        assert np.array_equal(_cpu(have), second[name]), name
    state2 = (second["count"], second["mean"], second["m2"])
    assert np.array_equal(_cpu(weights), restate_fold(_cpu(theta), state2, dtype=np.float64))
    assert torch.equal(weights_t.permute(2, 0, 1), weights)
    assert np.array_equal(_cpu(lane_w), restate_fold(_cpu(lanes), state2, dtype=np.float64, std_floor=0.5))
    assert np.array_equal(_cpu(grad_theta.permute(2, 0, 1)), restate_unfold(_cpu(theta), state2, dtype=np.float64))
    # the allocating forms return the same bits, in the layout they were given
    (c3, m3, q3), st3, v3 = sim.obs_stats(obs, policies=P, state=(count, mean, m2))
    assert torch.equal(c3, count2) and torch.equal(m3, mean2) and torch.equal(q3, m22)
    assert np.array_equal(_cpu(st3), second["steps"]) and np.array_equal(_cpu(v3), second["valid"])
    assert torch.equal(sim.norm_fold(theta, (c3, m3, q3)), weights)
    as_grad = theta_t.permute(2, 0, 1)                                               # what policy_gradient returns: a view of [2, D+1, P]
    w_view = sim.norm_fold(as_grad, (c3, m3, q3))
    assert torch.equal(w_view, weights) and w_view.permute(1, 2, 0).is_contiguous()
    assert torch.equal(sim.norm_fold(lanes, (c3, m3, q3), lanes=N, std_floor=0.5), lane_w)
    g_view = sim.norm_unfold(as_grad, (c3, m3, q3))
    assert torch.equal(g_view, grad_theta.permute(2, 0, 1)) and g_view.permute(1, 2, 0).is_contiguous()
    value_w = theta_t[0].t()                                                         # [P, D+1], a view of [D+1, P] as value_fit returns it
    w_value = sim.norm_fold(value_w, (c3, m3, q3))
    assert tuple(w_value.shape) == (P, D + 1) and torch.equal(w_value, weights[:, 0]) and w_value.t().is_contiguous()
    sim.close()


def test_real_consumer_an_ars_v2_generation(torch_mod):
    """M = 3 policies x S = 8 directions on a handle of 48 environments, K = 20 steps: reset -> es_perturb -> norm_fold(lanes) ->
    rollout_policy(want_outputs) -> obs_stats -> es_update.  The rollout's returns equal, bit for bit, those of a twin handle
    given restate_fold's weights; the new state equals restate_stats on the returned observations; a second generation merges
    into it, and its fold is no longer the identity."""
    torch = torch_mod
    a, b = _handle(), _handle()
    D, dev = a.D, a.device
    rng = np.random.default_rng(11)
    theta = torch.as_tensor(rng.normal(0, 0.3, (M_REAL, 2, D + 1))).to(dev)
    nu, state, seen = 0.05, None, []
    for gen in (1, 2):
        weights, _ = a.es_perturb(theta, S_REAL, nu, gen)
        if state is None:
            folded = weights                                                          # nothing seen yet: the fold is the identity
            empty = (torch.zeros(M_REAL, dtype=torch.int64, device=dev), torch.zeros(M_REAL, D, dtype=a.dtype, device=dev), torch.zeros(M_REAL, D, dtype=a.dtype, device=dev))
            assert torch.equal(a.norm_fold(weights, empty, lanes=N_REAL), weights)
            by_hand = weights
        else:
            folded = a.norm_fold(weights, state, lanes=N_REAL)
            by_hand = torch.as_tensor(restate_fold(_cpu(weights), tuple(_cpu(t) for t in state), dtype=np.float64)).to(dev)
            assert torch.equal(folded, by_hand) and not torch.equal(folded, weights)
        obs0, obs0_b = a.reset(), b.reset()
        ret, length, outs = a.rollout_policy(K_REAL, folded, first_episode=True, want_outputs=True)
        ret_b, length_b, _ = b.rollout_policy(K_REAL, by_hand, first_episode=True)
        torch.cuda.synchronize()
        assert torch.equal(obs0, obs0_b) and np.array_equal(_cpu(ret).view(np.uint64), _cpu(ret_b).view(np.uint64)) and torch.equal(length, length_b)
        new_state, steps, valid = a.obs_stats(outs[0], policies=M_REAL, obs0=obs0, length=length, state=state)
        want = restate_stats(_cpu(outs[0]), P=M_REAL, dtype=np.float64, obs0=_cpu(obs0), length=_cpu(length),
                             state=None if state is None else tuple(_cpu(t) for t in state))
        for have, name in zip(new_state + (steps, valid), ("count", "mean", "m2", "steps", "valid")):
            assert np.array_equal(_cpu(have), want[name]), (gen, name)
        assert _cpu(valid).tolist() == [2 * S_REAL] * M_REAL and (_cpu(steps) > 2 * S_REAL).all() and np.isfinite(want["mean"]).all()
        theta = a.es_update(ret, theta, S_REAL, gen, 0.02, top=3)[0]
        seen.append(_cpu(new_state[0]))
        state = new_state
    assert (seen[1] > seen[0]).all() and (seen[0] > 1).all()
    a.close(); b.close()
