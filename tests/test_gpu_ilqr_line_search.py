"""os2rs_ilqr_line_search (include/os2r_search.h) on the MI355X: the line search of iLQR in one launch.  The yardstick is a plain
numpy restatement of the header's steps 1-8 (`restate` below), written in the header's order: every product rounded on its own,
every sum of products ((x0 y0 + x1 y1) + x2 y2) + ..., in the layout's dtype.  The kernel must reproduce it bit for bit (the sign
of a zero aside: it is not part of the contract).  `restate` and `crafted` need no device: tests/test_ilqr_line_search_host.py
imports them."""
import ctypes

import numpy as np
import pytest

from helpers import make_config
from gym_os2r_amd import abi
from test_gpu_lqr_gains import R_COST, _bits, _dot

pytestmark = pytest.mark.gpu

NOMINAL = ("cost", "act_nom", "obs_nom", "end_nom", "lx", "lu", "p_final")
# nq, D, K, M, nalpha, always: the shapes of the issue
SHAPES = ((5, 10, 3, 70, 4, False),     # two workgroups, a tail of 6; K < nalpha leaves idle write-back waves
          (2, 4, 1, 1, 1, True),        # ACCEPT_ALWAYS
          (3, 12, 5, 65, 16, False),    # the widest workgroup, a tail of 1
          (4, 7, 9, 64, 3, False))      # K no multiple of nalpha


# ---------------------------------------------------------------------------------------
# the restatement (needs no device)
# ---------------------------------------------------------------------------------------
def restate(knot_obs, end_obs, act, target, Q, R, cols, dtype, done=None, Qf=None, always=False, nominal=None):
    """Kernel layouts: knot_obs [K, N, D], end_obs [N, D], act [K, N, 2], done [K, N] uint8 or None, target [M, D], Q [n, n],
    R [2, 2], Qf [n, n] or None (Q), cols the layout's slot_col [D]; nominal: dict of cost [M], act_nom [K, M, 2],
    obs_nom [K, M, D], end_nom [M, D], lx [n, K M], lu [2, K M], p_final [n, M] (each but cost may be missing: not written)
    -> dict of choice [M] int32, index [K M] int32, cand_cost [nalpha, M] and the nominal after the call (copies)."""
    K, N, D = knot_obs.shape
    M = target.shape[0]
    nalpha, L, n = N // M, K * M, Q.shape[0]
    knot_obs, end_obs, act, target = (np.asarray(x).astype(dtype) for x in (knot_obs, end_obs, act, target))
    Q, R = np.asarray(Q, np.float64).astype(dtype), np.asarray(R, np.float64).astype(dtype)     # rounded once
    Qf = Q if Qf is None else np.asarray(Qf, np.float64).astype(dtype)
    half, zero = dtype(0.5), np.zeros(N, dtype)
    tgt = np.tile(target, (nalpha, 1))                      # lane j = i M + m reads the target of trajectory m

    def err(o):
        # 2.
        e = []
        for c in range(n):
            shows = [d for d in range(D) if cols[d] == c]
            e.append(o[:, shows[0]] - tgt[:, shows[0]] if shows else zero)
        return e

    def quad(mat, e):
        # 3. (and 6. with Qf)
        g = [_dot([mat[r, c] for c in range(n)], e) for r in range(n)]
        return g, half * _dot(e, g)
    gx, gu, a = [], [], []
    with np.errstate(all="ignore"):
        J = zero
        for k in range(K):
            # 1.
            o = knot_obs[k]
            ak = np.clip(act[k], dtype(-1), dtype(1))
            g, sx = quad(Q, err(o))
            # 4.
            u = [R[c, 0] * ak[:, 0] + R[c, 1] * ak[:, 1] for c in range(2)]
            su = half * (ak[:, 0] * u[0] + ak[:, 1] * u[1])
            # 5.
            J = (J + sx) + su
            gx.append(g), gu.append(u), a.append(ak)
        # 6.
        gf, sf = quad(Qf, err(end_obs))
        J = J + sf
        # 7.
        nom = {k: np.array(v, dtype=dtype) for k, v in (nominal or {}).items()}
        ok = np.isfinite(J)
        if done is not None:
            ok &= ~(np.asarray(done) != 0).any(0)
        if not always:
            ok &= J < np.tile(nom["cost"], nalpha)
    Jc, okc = J.reshape(nalpha, M), ok.reshape(nalpha, M)
    choice = np.full(M, -1, np.int32)
    best = np.zeros(M, dtype)
    for i in range(nalpha):
        take = okc[i] & ((choice < 0) | (Jc[i] < best))
        choice[take], best[take] = i, Jc[i][take]
    # 8.
    index = np.full(L, -1, np.int32)
    for m in np.nonzero(choice >= 0)[0]:
        j = choice[m] * M + m
        if "cost" in nom:
            nom["cost"][m] = J[j]
        for k in range(K):
            index[k * M + m] = k * N + j
            if "act_nom" in nom:
                nom["act_nom"][k, m] = a[k][j]
            if "obs_nom" in nom:
                nom["obs_nom"][k, m] = knot_obs[k, j]
            if "lx" in nom:
                nom["lx"][:, k * M + m] = [gx[k][r][j] for r in range(n)]
            if "lu" in nom:
                nom["lu"][:, k * M + m] = [gu[k][c][j] for c in range(2)]
        if "end_nom" in nom:
            nom["end_nom"][m] = end_obs[j]
        if "p_final" in nom:
            nom["p_final"][:, m] = [gf[r][j] for r in range(n)]
    return dict(choice=choice, index=index, cand_cost=Jc.copy(), nominal=nom)


def crafted(nq, D, K, M, nalpha, seed=0):
    """The inputs of both test files (float64; a test rounds them to its dtype): random candidates around random targets, a
    layout with an unshown column, a slot that shows nothing and (D >= 3) two slots that show the same column, and by trajectory
      m % 3 == 0   a nominal cost of 0, below every candidate: nothing is acceptable
      m % 5 == 1   all candidates identical: the lowest index wins
      m % 5 == 2   (nalpha >= 3) candidates 1 and 2 identical and close to the target: 1 wins
      m % 7 == 3   a NaN in a slot of candidate 0 that is read
      m % 7 == 4   (D >= 3) a NaN in the higher of candidate 0's two slots that show the same column: it is not read
      m % 7 == 5   the last candidate sits on the target with zero actions (J = 0) but an episode ended inside it
    and a random nominal that the call must leave alone wherever nothing was accepted."""
    rng = np.random.default_rng(seed)
    n, N = 2 * nq, nalpha * M
    cols = [d % n for d in range(D)]
    if D >= 3:
        cols[1], cols[D - 1] = -1, cols[0]
    target = rng.standard_normal((M, D))
    tgt = np.tile(target, (nalpha, 1))
    knot_obs = tgt[None] + rng.standard_normal((K, N, D))
    end_obs = tgt + rng.standard_normal((N, D))
    act = rng.uniform(-1.3, 1.3, (K, N, 2))              # some outside [-1, 1]: clamped
    done = np.zeros((K, N), np.uint8)
    cost = np.full(M, 1e6)
    shown = [d for d in range(D) if cols[d] >= 0]
    for m in range(M):
        lanes = [i * M + m for i in range(nalpha)]
        if m % 3 == 0:
            cost[m] = 0.0
        if m % 5 == 1:
            for j in lanes[1:]:
                knot_obs[:, j], end_obs[j], act[:, j] = knot_obs[:, lanes[0]], end_obs[lanes[0]], act[:, lanes[0]]
        if m % 5 == 2 and nalpha >= 3:
            j1, j2 = lanes[1], lanes[2]
            knot_obs[:, j1] = target[m] + 0.01 * rng.standard_normal((K, D))
            end_obs[j1] = target[m] + 0.01 * rng.standard_normal(D)
            act[:, j1] = 0.01 * rng.standard_normal((K, 2))
            knot_obs[:, j2], end_obs[j2], act[:, j2] = knot_obs[:, j1], end_obs[j1], act[:, j1]
        if m % 7 == 3:
            knot_obs[K // 2, lanes[0], shown[0]] = np.nan
        if m % 7 == 4 and D >= 3:
            knot_obs[K // 2, lanes[0], D - 1] = np.nan
        if m % 7 == 5:
            knot_obs[:, lanes[-1]], end_obs[lanes[-1]], act[:, lanes[-1]] = target[m], target[m], 0.0
            done[K - 1, lanes[-1]] = 1
    g, gf = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    Q, Qf = g @ g.T / n + 0.1 * np.eye(n), 2.0 * (gf @ gf.T / n) + 0.1 * np.eye(n)
    Q, Qf = 0.5 * (Q + Q.T), 0.5 * (Qf + Qf.T)
    nominal = dict(cost=cost, act_nom=rng.standard_normal((K, M, 2)), obs_nom=rng.standard_normal((K, M, D)),
                   end_nom=rng.standard_normal((M, D)), lx=rng.standard_normal((n, K * M)), lu=rng.standard_normal((2, K * M)),
                   p_final=rng.standard_normal((n, M)))
    return dict(knot_obs=knot_obs, end_obs=end_obs, act=act, done=done, target=target, Q=Q, R=R_COST, Qf=Qf, cols=cols, nominal=nominal)


def restate_crafted(c, dtype, always=False, **kw):
    return restate(c["knot_obs"], c["end_obs"], c["act"], c["target"], c["Q"], c["R"], c["cols"], dtype, done=c["done"], Qf=c["Qf"],
                   always=always, nominal=c["nominal"], **kw)


def _same_bits(got, want, what, zero_sign_free=True):
    """Bit for bit, NaNs included (a copied NaN keeps its bits); a zero equals a zero of the other sign."""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else got
    got = np.ascontiguousarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    if zero_sign_free:
        bad &= ~((got == 0) & (want == 0))
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


# ---------------------------------------------------------------------------------------
# the raw call on torch tensors
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


PAD, MARK, IMARK = 64, -12345.5, -77


class Call:
    """One os2rs_ilqr_line_search call through ctypes: the inputs of `crafted` on the device, every nominal and output array
    between guard bands of PAD sentinel elements.  The constructor uploads, run() launches."""

    def __init__(self, torch, c, nq, dtype):
        from gym_os2r_amd import control, search
        self.torch, self.lib, self.nq, self.dtype, self.c = torch, search.load(), nq, dtype, c
        dt = np.float64 if dtype == abi.F64 else np.float32
        K, N, D = c["knot_obs"].shape
        M = c["target"].shape[0]
        self.dims = (K, M, N // M)
        dev = torch.device("cuda:0")
        put = lambda x, t=dt: torch.as_tensor(np.ascontiguousarray(np.asarray(x).astype(t))).to(dev)
        self.inputs = [put(c[k]) for k in ("knot_obs", "end_obs", "act")] + [put(c["done"], np.uint8), put(c["target"])]
        self.bufs, self.inner = {}, {}
        for name in NOMINAL:
            x = np.asarray(c["nominal"][name]).astype(dt)
            band = np.full(PAD, MARK, dt)
            self.bufs[name] = put(np.concatenate([band, x.reshape(-1), band]))
            self.inner[name] = self.bufs[name][PAD:-PAD].view(*x.shape)
        for name, shape, t in (("choice", (M,), np.int32), ("index", (K * M,), np.int32), ("cand_cost", (N // M, M), dt)):
            size = int(np.prod(shape))
            self.bufs[name] = put(np.full(PAD + size + PAD, IMARK if t is np.int32 else MARK, t), t)
            self.inner[name] = self.bufs[name][PAD:-PAD].view(*shape)
        self.before = {k: v.clone() for k, v in self.bufs.items()}

    def run(self, always=False, leave_out=(), stream=None, device=0, no_done=False):
        from gym_os2r_amd import control, search
        torch, c, n = self.torch, self.c, 2 * self.nq
        K, M, nal = self.dims
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        arg = lambda name: None if name in leave_out else p(self.inner[name])
        lay = control.layout(self.dtype, self.nq, device, c["cols"])
        q = (ctypes.c_double * (n * n))(*c["Q"].reshape(-1))
        r = (ctypes.c_double * 4)(*c["R"].reshape(-1))
        qf = (ctypes.c_double * (n * n))(*c["Qf"].reshape(-1))
        st = stream if stream is not None else torch.cuda.current_stream()
        ins = [p(t) for t in self.inputs]
        if no_done:
            ins[3] = None
        self.rc = self.lib.os2rs_ilqr_line_search(ctypes.byref(lay), K, M, nal, search.ACCEPT_ALWAYS if always else 0, *ins, q, r, qf,
                                                  p(self.inner["cost"]), *[arg(k) for k in NOMINAL[1:]], p(self.inner["choice"]),
                                                  arg("index"), arg("cand_cost"), ctypes.c_void_p(st.cuda_stream))
        self.error = self.lib.os2rs_last_error()
        return self

    def check(self, want, what, leave_out=()):
        torch = self.torch
        assert self.rc == abi.OK, self.error
        torch.cuda.synchronize()
        for name, buf in self.bufs.items():
            mark = IMARK if buf.dtype == torch.int32 else MARK
            assert bool((buf[:PAD] == mark).all()) and bool((buf[-PAD:] == mark).all()), (what, name)      # the guard bands
            if name in leave_out:
                assert torch.equal(buf, self.before[name]), (what, name)
                continue
            ref = want[name] if name in ("choice", "index", "cand_cost") else want["nominal"][name]
            _same_bits(self.inner[name], ref, f"{what}: {name}")
        # the nominal of a trajectory that accepted nothing: byte for byte what it was
        K, M, _ = self.dims
        refused = torch.as_tensor(want["choice"] < 0).to(self.bufs["cost"].device)
        for name, where in (("cost", refused), ("act_nom", refused.repeat(K)), ("obs_nom", refused.repeat(K)), ("end_nom", refused)):
            rows = self.inner[name].reshape(where.numel(), -1)
            was = self.before[name][PAD:-PAD].reshape(where.numel(), -1)
            assert torch.equal(was[where].contiguous().view(torch.uint8), rows[where].contiguous().view(torch.uint8)), (what, name)
        for name, where in (("lx", refused.repeat(K)), ("lu", refused.repeat(K)), ("p_final", refused)):
            cols = self.inner[name]
            was = self.before[name][PAD:-PAD].view(*cols.shape)
            assert torch.equal(was[:, where].contiguous().view(torch.uint8), cols[:, where].contiguous().view(torch.uint8)), (what, name)


# ---------------------------------------------------------------------------------------
# 1. + 2. bit for bit against the restatement, nothing outside the outputs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [abi.F64, abi.F32])
@pytest.mark.parametrize("nq,D,K,M,nalpha,always", SHAPES)
def test_equals_the_restatement_bit_for_bit_and_writes_nothing_else(torch_mod, dtype, nq, D, K, M, nalpha, always):
    """Every output and the whole nominal against `restate`; the guard bands around every buffer are as they were, and so is
    every nominal byte of a trajectory that accepted nothing."""
    c = crafted(nq, D, K, M, nalpha)
    want = restate_crafted(c, np.float64 if dtype == abi.F64 else np.float32, always=always)
    if M > 1:
        assert (want["choice"] >= 0).any() and (want["choice"] < 0).any()
    Call(torch_mod, c, nq, dtype).run(always=always).check(want, f"{(nq, D, K, M, nalpha)} {dtype}")


# ---------------------------------------------------------------------------------------
# 3. every nullable argument left out in turn
# ---------------------------------------------------------------------------------------
def test_each_nullable_output_left_out_leaves_the_others_as_they_are(torch_mod):
    nq, D, K, M, nalpha, _ = SHAPES[3]
    c = crafted(nq, D, K, M, nalpha)
    want = restate_crafted(c, np.float64)
    every = NOMINAL[1:] + ("index", "cand_cost")
    for name in every:
        Call(torch_mod, c, nq, abi.F64).run(leave_out=(name,)).check(want, f"without {name}", leave_out=(name,))
    Call(torch_mod, c, nq, abi.F64).run(leave_out=every).check(want, "choice and cost alone", leave_out=every)
    # done is nullable too: without it the candidates that sit on the target win
    want2 = restate_crafted(dict(c, done=np.zeros_like(c["done"])), np.float64)
    assert not np.array_equal(want2["choice"], want["choice"])
    Call(torch_mod, c, nq, abi.F64).run(no_done=True).check(want2, "without done")


# ---------------------------------------------------------------------------------------
# 4. stream order
# ---------------------------------------------------------------------------------------
def test_the_call_is_ordered_on_the_stream_it_is_given(torch_mod):
    """The device holds saturating actions; on a non-default stream a fill with 0.25 is enqueued and the call right behind it,
    with nothing between them but the stream's order: the call sees the filled actions."""
    torch = torch_mod
    nq, D, K, M, nalpha, _ = SHAPES[0]
    c = crafted(nq, D, K, M, nalpha)
    want = restate_crafted(dict(c, act=np.full_like(c["act"], 0.25)), np.float64)
    c_dev = dict(c, act=np.full_like(c["act"], 7.0))
    assert not np.array_equal(restate_crafted(c_dev, np.float64)["cand_cost"], want["cand_cost"])
    call = Call(torch, c_dev, nq, abi.F64)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        call.inputs[2].fill_(0.25)
    call.run(stream=side).check(want, "side stream")


# ---------------------------------------------------------------------------------------
# 5. error paths
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(torch_mod):
    from gym_os2r_amd.sim import HipSim
    cfg = make_config("free_hip", "BalancingV1", False, num_envs=8, contact=True, seed=5, auto_reset=False, dtype=abi.F64)[0]
    s = HipSim(cfg)
    yield s
    s.close()


def test_refusals_on_the_device(torch_mod, sim):
    torch = torch_mod
    nq, D, K, M, nalpha, _ = SHAPES[1]
    c = crafted(nq, D, K, M, nalpha)
    call = Call(torch, c, nq, abi.F64).run(device=1000)
    assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(b"os2rs_ilqr_line_search: "), (call.rc, call.error)
    torch.cuda.synchronize()
    assert all(torch.equal(call.bufs[k], call.before[k]) for k in call.bufs)       # a refused call wrote nothing
    bad = dict(c, Q=np.where(np.eye(2 * nq, k=1) > 0, 0.5, c["Q"]))
    call = Call(torch, bad, nq, abi.F64).run()
    assert call.rc == abi.ERR_INVALID and call.error == b"os2rs_ilqr_line_search: Q must be exactly symmetric"
    # through HipSim: refused in Python before the library is reached, or by the library with its own text
    n, D, dt, dev = 2 * sim.nq, sim.D, sim.dtype, sim.device
    z = lambda *shape, dtype=dt: torch.zeros(*shape, dtype=dtype, device=dev)
    K, M, nal = 2, 3, 2
    Q, R = np.eye(n), 0.1 * np.eye(2)
    good = dict(knot_obs=z(K, nal * M, D), end_obs=z(nal * M, D), actions=z(K, nal * M, 2), target=z(M, D))
    kw = dict(cost=z(M), choice=z(M, dtype=torch.int32))
    sim.ilqr_line_search_into(*good.values(), Q, R, **kw)
    torch.cuda.synchronize()
    assert kw["choice"].tolist() == [-1] * M                                       # J = 0 is not below a cost of 0
    for name, t in (("knot_obs", z(K, nal * M + 1, D)), ("end_obs", z(nal * M, D + 1)), ("actions", z(K, nal * M, 2).float()),
                    ("target", z(M, D + 1))):
        with pytest.raises(ValueError, match="^ilqr_line_search: "):
            sim.ilqr_line_search_into(*dict(good, **{name: t}).values(), Q, R, **kw)
    for more in (dict(index=z(K * M)), dict(lx=z(K * M, n)), dict(cand_cost=z(M, nal)), dict(done=z(K, nal * M)),
                 dict(Q_final=np.eye(n + 1)), dict(choice=z(M))):
        with pytest.raises(ValueError, match="^ilqr_line_search: "):
            sim.ilqr_line_search_into(*good.values(), Q, R, **dict(kw, **more))
    with pytest.raises(ValueError, match="^ilqr_line_search: Q must be exactly symmetric"):
        sim.ilqr_line_search_into(*good.values(), np.where(np.eye(n, k=1) > 0, 0.5, Q), R, **kw)


# ---------------------------------------------------------------------------------------
# 6. integration: recorded candidates -> line search -> the accepted knots -> the backward pass
# ---------------------------------------------------------------------------------------
def test_recorded_candidates_through_the_line_search_into_the_knots_and_the_backward_pass(torch_mod):
    torch = torch_mod
    from gym_os2r_amd.control import slot_columns
    from gym_os2r_amd.sim import HipSim
    K, M, alphas = 4, 4, (1.0, 0.5)
    nal = len(alphas)
    N = nal * M

    def make(num):
        cfg = make_config("free_hip", "BalancingV1", False, num_envs=num, contact=True, seed=5, auto_reset=False, dtype=abi.F64)[0]
        return HipSim(cfg)
    cand, cand_knots, knots, knots_ref = make(N), make(K * N), make(K * M), make(K * M)
    D, n, dev = cand.D, 2 * cand.nq, cand.device
    cols = slot_columns(cand.cfg.task, cand.nq)
    g = torch.Generator().manual_seed(4)
    # the candidates: open-loop actions as the bias of a zero-gain table, smaller for the second step size
    table = torch.zeros(N, K, 2, D + 1, dtype=torch.float64)
    bias = torch.rand(M, K, 2, generator=g, dtype=torch.float64) * 1.6 - 0.8
    for i, al in enumerate(alphas):
        table[i * M:(i + 1) * M, :, :, D] = al * bias
    # (odd trajectories take the two scalings the other way round, so that not every trajectory prefers the same candidate)
    table[1:M:2, :, :, D], table[M + 1:2 * M:2, :, :, D] = alphas[1] * bias[1::2], alphas[0] * bias[1::2]
    table = table.to(dev)
    _, _, (obs, _, done, _, _), (act, _), kobs = cand.rollout_schedule(K, table, want_outputs=True, want_actions=True, knots=cand_knots,
                                                                       want_knot_obs=True)
    target = kobs[0, :M].clone()
    qdiag = np.array([0.0 if c not in cols else (1.0 if c < cand.nq else 0.01) for c in range(n)])
    Q, R = np.diag(qdiag), 0.1 * np.eye(2)
    choice, index, cand_cost, nom = cand.ilqr_line_search(kobs, obs[K - 1], act, target, Q, R, done=done)
    torch.cuda.synchronize()
    want = restate(kobs.cpu().numpy(), obs[K - 1].cpu().numpy(), act.cpu().numpy(), target.cpu().numpy(), Q, R, cols, np.float64,
                   done=done.cpu().numpy(), always=True,
                   nominal={k: np.zeros(tuple(nom[v].shape)) for k, v in zip(NOMINAL, ("cost", "actions", "obs", "end_obs", "lx", "lu", "p_final"))})
    _same_bits(choice, want["choice"], "choice")
    _same_bits(index, want["index"], "index")
    _same_bits(cand_cost, want["cand_cost"], "cand_cost")
    for k, v in zip(NOMINAL, ("cost", "actions", "obs", "end_obs", "lx", "lu", "p_final")):
        _same_bits(nom[v], want["nominal"][k], v)
    assert (want["choice"] >= 0).all() and len(set(want["choice"].tolist())) == 2        # both candidates are somebody's choice
    # a second call on the nominal it returned: nothing is lower than the best, nothing moves
    cost_was = nom["cost"].clone()
    choice2, index2, _, nom2 = cand.ilqr_line_search(kobs, obs[K - 1], act, target, Q, R, nominal=nom, done=done, want_cand_cost=False)
    torch.cuda.synchronize()
    assert nom2 is nom and bool((choice2 == -1).all()) and bool((index2 == -1).all()) and torch.equal(nom["cost"], cost_was)
    # the accepted knots, moved by the index as it came, against per-lane selection with a hand-built index
    knots.copy_envs_from(cand_knots, index)
    lane = torch.arange(K * M, device=dev)
    hand = ((lane // M) * N + choice.long()[lane % M] * M + lane % M).to(torch.int32)
    knots_ref.copy_envs_from(cand_knots, hand)
    torch.cuda.synchronize()
    assert torch.equal(hand, index)
    def same(x, y, key):
        if isinstance(x, dict):
            assert x.keys() == y.keys(), key
            for k in x:
                same(x[k], y[k], (key, k))
        else:
            assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y), key
    same(knots.checkpoint(), knots_ref.checkpoint(), "checkpoint")
    sel = kobs.view(K, nal, M, D).gather(1, choice.long().view(1, 1, M, 1).expand(K, 1, M, D))[:, 0]
    assert torch.equal(nom["obs"], sel) and torch.equal(knots.copy_envs_from(knots, want_obs=True).view(K, M, D), sel)
    # the gradients as written into ilqr_backward_into, against ilqr_backward fed permuted copies
    _, _, A, B = knots.linearize(nom["actions"].view(K * M, 2), want_next=False)
    outs = dict(gains_out=torch.zeros(K, 2, n, M, dtype=torch.float64, device=dev), ff_out=torch.zeros(K, 2, M, dtype=torch.float64, device=dev),
                dv_out=torch.zeros(K, 2, M, dtype=torch.float64, device=dev))
    knots.ilqr_backward_into(A.permute(1, 2, 0).contiguous(), B.permute(1, 2, 0).contiguous(), Q, R, knots=K, lx=nom["lx"], lu=nom["lu"],
                             mu=0.1, p_final=nom["p_final"], **outs)
    gains, ff, _, _, _, dv, _ = knots.ilqr_backward(A, B, Q, R, knots=K, lx=nom["lx"].permute(1, 0).contiguous(),
                                                    lu=nom["lu"].permute(1, 0).contiguous(), mu=0.1,
                                                    p_final=nom["p_final"].permute(1, 0).contiguous())
    viewed = knots.ilqr_backward(A, B, Q, R, knots=K, lx=nom["lx_view"], lu=nom["lu_view"], mu=0.1, p_final=nom["p_final_view"])
    torch.cuda.synchronize()
    assert torch.equal(outs["gains_out"].permute(0, 3, 1, 2), gains) and torch.equal(outs["ff_out"].permute(0, 2, 1), ff)
    assert torch.equal(outs["dv_out"].permute(0, 2, 1), dv) and bool((ff != 0).any())
    assert torch.equal(viewed[0], gains) and torch.equal(viewed[1], ff) and torch.equal(viewed[5], dv)
    for s in (cand, cand_knots, knots, knots_ref):
        s.close()


# ---------------------------------------------------------------------------------------
# 7. the example's device mode runs to its end
# ---------------------------------------------------------------------------------------
def test_example_with_the_device_line_search_never_raises_the_mean_cost(torch_mod):
    """A trajectory's cost changes only where a candidate lowered it, so the printed mean cannot rise; every iteration's line
    says how many trajectories took which step size, and they add up."""
    import os
    import re
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ilqr_balancing.py"), "--envs", "8", "--steps", "20", "--iters", "3",
                          "--line-search", "device"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    costs = [float(c) for c in re.findall(r"^iter +\d+ +cost +([-+0-9.eE]+)", out.stdout, re.M)]
    assert len(costs) == 4, out.stdout[-2000:]                      # the nominal and three iterations
    assert all(b <= a for a, b in zip(costs, costs[1:])), costs
    took = re.findall(r"step sizes (\d+) x 1\.0, (\d+) x 0\.5, (\d+) x 0\.25, (\d+) x 0\.125, none (\d+);", out.stdout)
    assert took and all(sum(int(v) for v in line) == 8 for line in took), out.stdout[-2000:]
