"""os2r_copy_envs (include/os2r.h) on the MI355X: environment e of a handle becomes environment index[e] of another handle, or
of the same one, in one launch.  The yardstick is always the path that existed before -- HipSim.checkpoint(), index_select,
torch.where for the kept lanes, HipSim.restore() --, never the new code against itself; every comparison is torch.equal."""
import ctypes

import pytest

from helpers import make_config
from gym_os2r_amd import abi

pytestmark = pytest.mark.gpu

PARAMS = (abi.PARAM_MASS_SCALE, abi.PARAM_DAMPING, abi.PARAM_FRICTION, abi.PARAM_MU, abi.PARAM_GRAVITY)
STATE_KEYS = ("q", "qd", "solver_lambda", "solver_flags", "hist0", "hist1", "steps", "episode", "pose")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def HipSim(torch_mod):
    from gym_os2r_amd.sim import HipSim
    return HipSim


def _make(HipSim, n, dtype=abi.F64, seed=5, preroll=0, mode="fixed_hip_simple", normalized=True, max_episode_steps=100_000,
          binding=None, **kw):
    """Monopod-balance-v1 (fixed_hip_simple, BalancingV1) under the randomizer, ground contact on; `preroll` env-steps with
    device-drawn actions: robots on the ground, solver state populated, several episodes old."""
    cfg = make_config(mode, "BalancingV1", normalized, reset_mode=abi.RESET_RANDOM, randomize_params=True, num_envs=n,
                      contact=True, seed=seed, max_episode_steps=max_episode_steps, dtype=dtype, **kw)[0]
    sim = HipSim(cfg, binding=binding)
    obs = sim.reset()
    for _ in range(preroll):
        obs = sim.step(None)[0]
    return sim, obs


def _flat(ck):
    out = {k: ck[k] for k in STATE_KEYS}
    out.update({f"param{f}": ck["params"][f] for f in PARAMS})
    return out


def _assert_same(torch, a, b, what, keys=None):
    """two checkpoints (or flattened ones), array by array"""
    fa, fb = (_flat(a) if "params" in a else a), (_flat(b) if "params" in b else b)
    for k in (keys or fa):
        assert fa[k].dtype == fb[k].dtype and torch.equal(fa[k], fb[k]), (what, k)


def _index(torch, n_dst, n_src, seed, keep=0.1):
    """random source environments with repeats, about `keep` of the entries negative"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n_src, (n_dst,), generator=g, dtype=torch.int32)
    neg = torch.rand(n_dst, generator=g) < keep
    idx = torch.where(neg, torch.where(torch.rand(n_dst, generator=g) < 0.5, -1, -12345).to(torch.int32), idx)
    return idx.cuda()


def _composed(torch, dst, src, index, state=True, params=True):
    """What existed before: checkpoint / index_select / where / restore (about 28 launches and nine host synchronisations)."""
    cs, cd = src.checkpoint(), dst.checkpoint()
    ix = index.long()
    take = (ix >= 0) & (ix < src.N)
    g = ix.clamp(0, src.N - 1)
    pick = lambda s, d: torch.where(take, s.index_select(-1, g), d)
    new = {k: pick(cs[k], cd[k]) if state else cd[k] for k in STATE_KEYS}
    new["params"] = {f: pick(cs["params"][f], cd["params"][f]) if params else cd["params"][f] for f in PARAMS}
    new["step_count"] = cd["step_count"]
    dst.restore(new)
    return take


@pytest.mark.parametrize("n_dst", [1000, 4096])
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
def test_cross_handle_copy_equals_the_composed_path(HipSim, torch_mod, dtype, n_dst):
    torch = torch_mod
    src, _ = _make(HipSim, 4096, dtype, seed=5, preroll=300)
    a, _ = _make(HipSim, n_dst, dtype, seed=11)
    b, _ = _make(HipSim, n_dst, dtype, seed=11)
    ck = src.checkpoint()
    if dtype == abi.F64:      # (fp32 handles carry the solver's state but never write it: include/os2r.h, os2r_get_solver_state)
        assert bool((ck["solver_flags"] != 0).any()) and bool((ck["solver_lambda"] != 0).any())     # the solver's state is populated
    index = _index(torch, n_dst, src.N, seed=1)
    assert bool((index < 0).any()) and index.unique().numel() < n_dst
    assert a.copy_envs_from(src, index) is None
    _composed(torch, b, src, index)
    assert a.step_count == b.step_count
    _assert_same(torch, a.checkpoint(), b.checkpoint(), "after the copy")
    _assert_same(torch, src.checkpoint(), ck, "the source is untouched")
    gen = torch.Generator(device="cuda").manual_seed(3)
    for k in range(50):
        act = torch.rand(n_dst, 2, dtype=a.dtype, device="cuda", generator=gen) * 2 - 1
        oa, ob = a.step(act), b.step(act)
        for x, y, name in zip(oa, ob, ("obs", "reward", "done", "terminal_obs")):
            assert torch.equal(x, y), (k, name)
    _assert_same(torch, a.checkpoint(), b.checkpoint(), "after 50 steps")
    assert a.step_count == b.step_count
    for s in (src, a, b):
        s.close()


@pytest.mark.parametrize("binding", ["ctypes", "pybind11"])
def test_fork_of_one_environment_into_a_planner(HipSim, torch_mod, binding):
    """A 1-env "real" handle copied into every lane of a 256-env planner: lane 0 of the planner's rollout is the real handle's
    own future under lane 0's actions, bit for bit -- seed, env_offset 0 and step counter agree, so the resets inside the
    window (TimeLimit 7) coincide too."""
    torch = torch_mod
    real, _ = _make(HipSim, 1, seed=9, preroll=150, max_episode_steps=7, binding=binding)
    planner, _ = _make(HipSim, 256, seed=9, max_episode_steps=7, binding=binding)
    planner.step_count = real.step_count
    planner.copy_envs_from(real, 0)
    ck = _flat(planner.checkpoint())
    for k, v in _flat(real.checkpoint()).items():
        assert torch.equal(ck[k], v.expand_as(ck[k])), k
    gen = torch.Generator(device="cuda").manual_seed(4)
    actions = torch.rand(10, 256, 2, dtype=real.dtype, device="cuda", generator=gen) * 2 - 1
    obs, rew, done, term, _ = planner.rollout(10, actions, want_terminal=True)
    seen = 0
    for k in range(10):
        o, r, d, t = real.step(actions[k, 0:1])
        assert torch.equal(o[0], obs[k, 0]) and torch.equal(r[0], rew[k, 0]) and torch.equal(d[0], done[k, 0]), k
        assert torch.equal(t[0], term[k, 0]), k
        seen += int(d[0] != 0)
    assert seen >= 1, "a reset was meant to fall inside the window"
    real.close(); planner.close()


def test_in_place_permutation_inverse_and_fork(HipSim, torch_mod):
    torch = torch_mod
    n = 1000
    x, _ = _make(HipSim, n, seed=5, preroll=200)
    y, _ = _make(HipSim, n, seed=5, preroll=200)
    before = x.checkpoint()
    _assert_same(torch, before, y.checkpoint(), "twins")
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2)).to(torch.int32).cuda()
    x.copy_envs_from(x, perm)
    _composed(torch, y, y, perm)
    after = x.checkpoint()
    _assert_same(torch, after, y.checkpoint(), "in-place permutation")
    assert not torch.equal(after["q"], before["q"])
    inv = torch.argsort(perm.long()).to(torch.int32)
    x.copy_envs_from(x, inv)
    _assert_same(torch, x.checkpoint(), before, "permutation, then its inverse")
    # a partial in-place map with repeats and kept lanes: all reads precede all writes
    index = _index(torch, n, n, seed=6, keep=0.3)
    x.copy_envs_from(x, index)
    y.restore(before)
    _composed(torch, y, y, index)
    _assert_same(torch, x.checkpoint(), y.checkpoint(), "in-place partial map")
    x.restore(before)
    x.copy_envs_from(x, 7)
    for k, v in _flat(x.checkpoint()).items():
        col = _flat(before)[k][..., 7:8]
        assert torch.equal(v, col.expand_as(v)), k
    # the identity map within one handle changes nothing
    x.restore(before)
    x.copy_envs_from(x)
    _assert_same(torch, x.checkpoint(), before, "identity in place")
    x.close(); y.close()


def test_selection_of_state_and_parameters(HipSim, torch_mod):
    torch = torch_mod
    src, _ = _make(HipSim, 512, seed=5, preroll=200)
    dst, _ = _make(HipSim, 300, seed=6, preroll=20)
    index = _index(torch, 300, 512, seed=8)
    take = (index >= 0)
    cs, c0 = _flat(src.checkpoint()), _flat(dst.checkpoint())
    want = {k: torch.where(take, cs[k].index_select(-1, index.long().clamp(0)), c0[k]) for k in c0}
    params = [f"param{f}" for f in PARAMS]
    dst.copy_envs_from(src, index, state=True, params=False)
    c1 = _flat(dst.checkpoint())
    _assert_same(torch, c1, c0, "parameters untouched", keys=params)
    _assert_same(torch, c1, want, "state copied", keys=STATE_KEYS)
    assert not torch.equal(c1["q"], c0["q"])
    dst.restore(dict(dst.checkpoint(), **{k: c0[k] for k in STATE_KEYS}))
    dst.copy_envs_from(src, index, state=False, params=True)
    c2 = _flat(dst.checkpoint())
    _assert_same(torch, c2, c0, "state untouched", keys=STATE_KEYS)
    _assert_same(torch, c2, want, "parameters copied", keys=params)
    assert not torch.equal(c2["param0"], c0["param0"])
    src.close(); dst.close()


@pytest.mark.parametrize("dtype,normalized", [(abi.F64, True), (abi.F64, False), (abi.F32, True)])
def test_observation_after_the_copy(HipSim, torch_mod, dtype, normalized):
    """Equal tasks: the observation of a copied lane is the one the source's last step returned for that environment, the
    observation of a kept lane the destination's own last one; also for a no_norm task (a run-time observation layout)."""
    torch = torch_mod
    src, obs_src = _make(HipSim, 640, dtype, seed=5, preroll=120, normalized=normalized)
    dst, obs_dst = _make(HipSim, 1000, dtype, seed=6, preroll=30, normalized=normalized)
    index = _index(torch, 1000, 640, seed=9, keep=0.25)
    take = index >= 0
    obs = dst.copy_envs_from(src, index, want_obs=True)
    assert obs.shape == (1000, dst.D) and obs.dtype == dst.dtype
    want = torch.where(take[:, None], obs_src.index_select(0, index.long().clamp(0)), obs_dst)
    assert torch.equal(obs, want)
    # identity map, whole batch, through a twin of the source
    twin, _ = _make(HipSim, 640, dtype, seed=77, normalized=normalized)
    assert torch.equal(twin.copy_envs_from(src, want_obs=True), obs_src)
    for s in (src, dst, twin):
        s.close()


def test_out_of_range_index_keeps_the_environment(HipSim, torch_mod):
    torch = torch_mod
    src, _ = _make(HipSim, 128, seed=5, preroll=50)
    a, _ = _make(HipSim, 256, seed=6, preroll=10)
    b, _ = _make(HipSim, 256, seed=6, preroll=10)
    index = _index(torch, 256, 128, seed=3)
    index[5] = 128                       # == src.N
    index[6] = 2 ** 31 - 1               # far above
    index[7] = 129
    index[200] = 1 << 20
    a.copy_envs_from(src, index)
    kept = _composed(torch, b, src, index)
    assert not bool(kept[5]) and not bool(kept[6]) and not bool(kept[200])
    _assert_same(torch, a.checkpoint(), b.checkpoint(), "entries past the source are kept lanes")
    with pytest.raises(ValueError, match=">= the source"):
        a.copy_envs_from(src, index, check=True)
    index[index >= 128] = -1
    a.copy_envs_from(src, index, check=True)       # nothing out of range: goes through
    with pytest.raises(ValueError):
        a.copy_envs_from(src, index.long())         # dtype
    with pytest.raises(ValueError):
        a.copy_envs_from(src, index[:100])          # shape
    with pytest.raises(ValueError):
        a.copy_envs_from(src, index.cpu())          # device
    with pytest.raises(ValueError):
        a.copy_envs_from(src, 128)                  # an int names one environment of the source
    for s in (src, a, b):
        s.close()


def test_refusals_name_their_cause(HipSim, torch_mod):
    from gym_os2r_amd.sim import Os2rError
    torch = torch_mod
    f64, _ = _make(HipSim, 64, abi.F64)
    f32, _ = _make(HipSim, 64, abi.F32)
    other, _ = _make(HipSim, 64, abi.F64, mode="free_hip")
    small, _ = _make(HipSim, 32, abi.F64)
    before = f64.checkpoint()
    with pytest.raises(Os2rError, match="dtype"):
        f64.copy_envs_from(f32)
    with pytest.raises(Os2rError, match="robot model"):
        f64.copy_envs_from(other)
    with pytest.raises(Os2rError, match="what == 0"):
        f64.copy_envs_from(small, 0, state=False, params=False)
    idx = torch.zeros(64, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for what, msg in ((8, b"unknown bits"), (abi.COPY_STATE | 4, b"unknown bits"), (0, b"what == 0")):
        rc = f64._lib.os2r_copy_envs(f64._h, small._h, ctypes.c_void_p(idx.data_ptr()), what, None, st)
        assert rc == abi.ERR_INVALID and msg in f64._lib.os2r_last_error(f64._h), what
    with pytest.raises(Os2rError, match="equal num_envs"):
        f64.copy_envs_from(small)
    torch.cuda.synchronize()
    _assert_same(torch, f64.checkpoint(), before, "a refused call changes nothing")
    f64.copy_envs_from(small, idx)                  # unequal sizes with an index are the normal case
    for s in (f64, f32, other, small):
        s.close()


def test_copy_and_step_can_be_captured_in_a_hip_graph(HipSim, torch_mod):
    """After one eager warm-up call, copy_envs_from(real, idx) followed by step_into on one stream goes into a HIP graph (a
    linear chain); replayed after every step of the real handle it equals the eager sequence on a twin planner."""
    torch = torch_mod
    n = 256
    real, _ = _make(HipSim, 1, seed=9, preroll=60, max_episode_steps=9)
    graphed, _ = _make(HipSim, n, seed=9, max_episode_steps=9)
    eager, _ = _make(HipSim, n, seed=9, max_episode_steps=9)
    dt = real.dtype
    idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    act = torch.zeros(n, 2, dtype=dt, device="cuda")
    obs = torch.empty(n, real.D, dtype=dt, device="cuda"); rew = torch.empty(n, dtype=dt, device="cuda")
    done = torch.empty(n, dtype=torch.uint8, device="cuda"); term = torch.empty_like(obs)
    gen = torch.Generator(device="cuda").manual_seed(3)
    actions = [torch.rand(n, 2, dtype=dt, device="cuda", generator=gen) * 2 - 1 for _ in range(12)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        act.copy_(actions[0]); graphed.copy_envs_from(real, idx); graphed.step_into(act, obs, rew, done, term)   # warm-up
    torch.cuda.current_stream().wait_stream(side)
    eager.copy_envs_from(real, idx); ref = eager.step(actions[0])
    assert torch.equal(ref[0], obs)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.copy_envs_from(real, idx)
        graphed.step_into(act, obs, rew, done, term)
    for k in range(1, 12):
        real.step(actions[k][0:1])
        act.copy_(actions[k]); graph.replay()
        eager.copy_envs_from(real, idx)
        o, r, d, t = eager.step(actions[k])
        assert torch.equal(o, obs) and torch.equal(r, rew) and torch.equal(d, done) and torch.equal(t, term), k
    _assert_same(torch, graphed.checkpoint(), eager.checkpoint(), "after the replays")
    for s in (real, graphed, eager):
        s.close()
