"""libos2r_box.so (include/os2r_box.h) on the MI355X: os2rb_ilqr_backward_box against the numpy restatement of
tests/test_ilqr_box_host.py on the inputs that file holds to reach every clamp byte, a refused knot and an invalid mu, bit for bit
(the sign of a zero aside: it is not part of the contract; integers exactly); against os2rt_ilqr_backward_mu on the device with
infinite bounds; aliased outputs, a call that asks for the clamp bytes and dv alone, and one closed loop on real handles."""
import ctypes

import numpy as np
import pytest

from helpers import make_config
from gym_os2r_amd import abi
from test_gpu_ilqr_line_search import MARK, PAD, _same_bits
from test_gpu_lqr_gains import R_COST
from test_ilqr_box_host import INF, ONE_SIDED, OUTPUTS, SHAPE, box_case, wanted

pytestmark = pytest.mark.gpu

UMARK = 0xA5
INPUTS = ("A", "B", "lx", "lu", "P_final", "p_final", "actions", "obs", "mu")
CASES = [(nq, dtype) for dtype in (abi.F64, abi.F32) for nq in (2, 5)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _np(dtype):
    return np.float64 if dtype == abi.F64 else np.float32


class BoxCall:
    """One os2rb_ilqr_backward_box call through ctypes: the inputs of `box_case` on the device, every output between guard bands
    of PAD sentinel elements.  The constructor uploads, run() launches."""

    def __init__(self, torch, c, nq, dtype):
        from gym_os2r_amd import box
        self.torch, self.lib, self.nq, self.dtype, self.c = torch, box.load(), nq, dtype, c
        dt = _np(dtype)
        n, K = 2 * nq, c["K"]
        M = c["A"].shape[2] // K
        D, nal = len(c["cols"]), len(c["alphas"])
        self.dims = (K, M)
        dev = torch.device("cuda:0")
        put = lambda x, t=dt: torch.as_tensor(np.ascontiguousarray(np.asarray(x).astype(t))).to(dev)
        self.ins = dict(A=put(c["A"]), B=put(c["B"]), mu=put(c["mu"]), **{k: put(v) for k, v in c["kw"].items()})
        self.ins_before = {k: v.clone() for k, v in self.ins.items()}
        shapes = dict(gains=(K, 2, n, M), ff=(K, 2, M), P=(n, n, M), p=(n, M), flags=(K, M), dv=(K, 2, M), weights=(K, 2, D + 1, nal * M),
                      clamped=(K, M))
        self.bufs, self.inner = {}, {}
        for name, shape in shapes.items():
            t, mark = (np.uint8, UMARK) if name in ("flags", "clamped") else (dt, MARK)
            self.bufs[name] = put(np.full(PAD + int(np.prod(shape)) + PAD, mark, t), t)
            self.inner[name] = self.bufs[name][PAD:-PAD].view(*shape)
        self.before = {k: v.clone() for k, v in self.bufs.items()}

    def run(self, lo=(-1.0, -1.0), hi=(1.0, 1.0), mu=None, only=OUTPUTS, alias=False, device=0):
        """mu None: the array of the case; a number: that scalar with a null mu_dev.  alias: P and p are written over P_final and
        p_final."""
        from gym_os2r_amd import control
        c, n = self.c, 2 * self.nq
        K, M = self.dims
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        out = lambda name: p(self.inner[name]) if name in only else None
        i = self.ins
        lay = control.layout(self.dtype, self.nq, device, c["cols"])
        q = (ctypes.c_double * (n * n))(*c["Q"].reshape(-1))
        r = (ctypes.c_double * 4)(*R_COST.reshape(-1))
        al = (ctypes.c_double * len(c["alphas"]))(*c["alphas"])
        V = lambda v: (ctypes.c_double * 2)(*v)
        pm, pv = (p(i["P_final"]), p(i["p_final"])) if alias else (out("P"), out("p"))
        st = ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        self.rc = self.lib.os2rb_ilqr_backward_box(ctypes.byref(lay), K, M, p(i["A"]), p(i["B"]), p(i["lx"]), p(i["lu"]), q, r,
                                                   0.0 if mu is None else mu, p(i["mu"]) if mu is None else None, V(lo), V(hi),
                                                   p(i["P_final"]), p(i["p_final"]), out("gains"), out("ff"), pm, pv, out("flags"), out("dv"),
                                                   out("clamped"), p(i["actions"]), p(i["obs"]), al, len(c["alphas"]), out("weights"), st)
        self.error = self.lib.os2rb_last_error()
        return self

    def check(self, want, what, only=OUTPUTS, alias=False):
        """Every output asked for against `want`, every other buffer and every guard band as it was, the inputs unread but for
        the aliased ones."""
        torch = self.torch
        assert self.rc == abi.OK, self.error
        torch.cuda.synchronize()
        for name, buf in self.bufs.items():
            mark = UMARK if buf.dtype == torch.uint8 else MARK
            assert bool((buf[:PAD] == mark).all()) and bool((buf[-PAD:] == mark).all()), (what, name)      # the guard bands
            if name not in only or (alias and name in ("P", "p")):
                assert torch.equal(buf, self.before[name]), (what, name)
                continue
            _same_bits(self.inner[name], want[name], f"{what}: {name}")
        for name, t in self.ins.items():
            if alias and name in ("P_final", "p_final"):
                _same_bits(t, want["P" if name == "P_final" else "p"], f"{what}: {name}, written over")
            else:
                assert torch.equal(t.view(torch.uint8), self.ins_before[name].view(torch.uint8)), (what, name)


@pytest.mark.parametrize("nq,dtype", CASES)
def test_every_output_equals_the_restatement_bit_for_bit(torch_mod, nq, dtype):
    """K = 5, M = 70 (three workgroups, the last with 6 lanes), one mu per trajectory, every output asked for: under the default
    box, where the inputs reach every clamp byte, a refused trajectory and an invalid mu (tests/test_ilqr_box_host.py asserts
    it), and with one side of each component open."""
    c = box_case(nq)
    assert (c["K"], c["A"].shape[2] // c["K"]) == SHAPE
    want = wanted(nq, _np(dtype))
    assert len(np.unique(want["clamped"])) == 9 and want["flags"].any()
    BoxCall(torch_mod, c, nq, dtype).run().check(want, f"box nq {nq} {dtype}")
    one = wanted(nq, _np(dtype), "one_sided")
    assert one["clamped"].any()
    BoxCall(torch_mod, c, nq, dtype).run(**ONE_SIDED).check(one, f"one side open, nq {nq} {dtype}")


@pytest.mark.parametrize("nq,dtype", CASES)
def test_a_scalar_mu_with_a_null_mu_dev(torch_mod, nq, dtype):
    c = box_case(nq, 2, 40)
    want = wanted(nq, _np(dtype), "scalar")
    assert want["clamped"].any() and (want["clamped"] == 0).any()
    BoxCall(torch_mod, c, nq, dtype).run(mu=0.5).check(want, f"scalar mu, nq {nq} {dtype}")


@pytest.mark.parametrize("nq,dtype", CASES)
def test_with_infinite_bounds_every_shared_output_has_the_bits_of_backward_mu(torch_mod, nq, dtype):
    """os2rt_ilqr_backward_mu on the same device arrays; clamped is all zero."""
    from gym_os2r_amd import control, steer
    torch = torch_mod
    c = box_case(nq)
    ours = BoxCall(torch, c, nq, dtype).run(lo=(-INF, -INF), hi=(INF, INF))
    theirs = BoxCall(torch, c, nq, dtype)
    n, (K, M) = 2 * nq, theirs.dims
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    i, o = theirs.ins, theirs.inner
    lay = control.layout(dtype, nq, 0, c["cols"])
    q, r = (ctypes.c_double * (n * n))(*c["Q"].reshape(-1)), (ctypes.c_double * 4)(*R_COST.reshape(-1))
    al = (ctypes.c_double * len(c["alphas"]))(*c["alphas"])
    lib = steer.load()
    rc = lib.os2rt_ilqr_backward_mu(ctypes.byref(lay), K, M, p(i["A"]), p(i["B"]), p(i["lx"]), p(i["lu"]), q, r, p(i["mu"]), p(i["P_final"]),
                                    p(i["p_final"]), p(o["gains"]), p(o["ff"]), p(o["P"]), p(o["p"]), p(o["flags"]), p(o["dv"]), p(i["actions"]),
                                    p(i["obs"]), al, len(c["alphas"]), p(o["weights"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == abi.OK and ours.rc == abi.OK, (lib.os2rt_last_error(), ours.error)
    torch.cuda.synchronize()
    for name in OUTPUTS[:-1]:
        assert torch.equal(ours.bufs[name].view(torch.uint8), theirs.bufs[name].view(torch.uint8)), name
    assert not bool(ours.inner["clamped"].any()) and bool((ours.bufs["clamped"][:PAD] == UMARK).all())
    assert bool(ours.inner["flags"].any()) and bool((ours.inner["ff"] != 0).any())


def test_outputs_may_alias_the_final_value_and_a_call_may_ask_for_little(torch_mod):
    """pmat_out and pvec_out over pmat_final and pvec_final; then clamp_dev and dv_dev alone: nothing else is written, not a
    guard word of any buffer, not an input."""
    nq, dtype = 5, abi.F64
    c = box_case(nq)
    want = wanted(nq, np.float64)
    BoxCall(torch_mod, c, nq, dtype).run(alias=True).check(want, "aliased", alias=True)
    BoxCall(torch_mod, c, nq, dtype).run(only=("clamped", "dv")).check(want, "clamped and dv alone", only=("clamped", "dv"))
    call = BoxCall(torch_mod, c, nq, dtype).run(only=("clamped", "flags"))
    assert call.rc == abi.ERR_INVALID and call.error.endswith(b"(gain, ff, pmat_out, pvec_out, dv, weights)")
    torch_mod.cuda.synchronize()
    assert all(torch_mod.equal(call.bufs[k], call.before[k]) for k in call.bufs)
    call = BoxCall(torch_mod, c, nq, dtype).run(device=1000)
    assert call.rc == abi.ERR_NO_DEVICE and call.error.startswith(b"os2rb_ilqr_backward_box: "), (call.rc, call.error)


def test_the_closed_loop_stays_inside_the_box_at_the_first_knot(torch_mod):
    """Monopod-nonorm-balance-v1, 8 trajectories x 5 knots: a recorded rollout of a nominal inside (-0.5, 0.5), linearize, the box
    pass with the table for alpha = (1, 1/2), rollout_schedule on the 16 forked lanes.  At knot 0 the state deviation is zero, so
    the applied action is the table's a0 + alpha k: exactly its bias entry where the component is clamped (that gain row is zero),
    and within the rounding of the D products of the row elsewhere.  It lies within [lo, hi] to 2 ulp of the bound -- (lo - a0) + a0
    rounds twice -- and strictly inside (-1, 1): the rollout's clip has not touched it."""
    torch = torch_mod
    from gym_os2r_amd.control import slot_columns
    from gym_os2r_amd.sim import HipSim
    K, M, alphas, lo, hi = 5, 8, (1.0, 0.5), -0.5, 0.5
    nal = len(alphas)
    N = nal * M

    def make(num):
        cfg = make_config("free_hip", "BalancingV1", False, num_envs=num, contact=True, seed=5, auto_reset=False, dtype=abi.F64)[0]
        return HipSim(cfg)
    nom_h, cand, knots = make(M), make(N), make(K * M)
    D, n, dev = nom_h.D, 2 * nom_h.nq, nom_h.device
    cols = slot_columns(nom_h.cfg.task, nom_h.nq)
    qdiag = np.array([0.0 if c not in cols else (1.0 if c < nom_h.nq else 0.01) for c in range(n)])
    Q, R = np.diag(qdiag), 1e-5 * np.eye(2)
    # the nominal: constant torques inside the box, close to its sides, recorded; the target: two radians off where it starts and R small, so the steps are long
    # (+-0.45 in the four sign patterns: whichever way a step points, some component has 0.05 of room)
    signs = np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, 1.0], [-1.0, -1.0]])[np.arange(M) % 4]
    table0 = torch.zeros(M, K, 2, D + 1, dtype=torch.float64, device=dev)
    table0[:, :, :, D] = torch.as_tensor(0.45 * np.repeat(signs[:, None, :], K, 1)).to(dev)
    _, _, (o_n, _, d_n, _, _), (a_n, _), kobs = nom_h.rollout_schedule(K, table0, want_outputs=True, want_actions=True, knots=knots,
                                                                       want_knot_obs=True)
    target = kobs[0] + 2.0
    _, _, _, nominal = nom_h.ilqr_line_search(kobs, o_n[K - 1], a_n, target, Q, R, done=d_n, want_cand_cost=False)
    a_k, obs_k = nominal["actions"].view(K * M, 2), nominal["obs"].view(K * M, D)
    _, _, A, B = knots.linearize(a_k, want_next=False)
    out = nom_h.ilqr_backward(A, B, Q, R, knots=K, lx=nominal["lx_view"], lu=nominal["lu_view"], mu=1e-6, p_final=nominal["p_final_view"],
                              actions=a_k, obs=obs_k, alphas=alphas, want_weights=True, box=(lo, hi))
    assert len(out) == 8
    gains, ff, _, _, flags, _, table, clamped = out
    first = torch.arange(M, dtype=torch.int32, device=dev).repeat(nal)
    cand.copy_envs_from(knots, first)
    _, _, _, (a_c, _), _ = cand.rollout_schedule(K, table, want_outputs=True, want_actions=True, want_knot_obs=True)
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu().numpy().copy()
    applied, ff0, a0, cl = cpu(a_c)[0].reshape(nal, M, 2), cpu(ff)[0], cpu(a_k)[:M], cpu(clamped)[0]
    tab, obs0 = cpu(table)[:, 0].reshape(nal, M, 2, D + 1), cpu(obs_k)[:M]
    print("first-knot steps", ff0.tolist(), "clamp bytes", cpu(clamped).tolist())
    assert not cpu(flags).any() and (np.abs(a0) == 0.45).all()
    assert cl.any(), cl                                                        # the limits hold at some first knots
    eps = np.finfo(np.float64).eps
    for i, alpha in enumerate(alphas):
        for j in range(2):
            held = (cl >> j & 1) != 0
            assert not tab[i, :, j, :D][held].any()
            assert np.array_equal(applied[i, :, j][held], tab[i, :, j, D][held])
            assert np.array_equal(tab[i, :, j, D][held], (a0[:, j] + alpha * ff0[:, j])[held])
            room = 8 * eps * (1.0 + np.abs(tab[i, :, j, :D] * obs0).sum(1) + np.abs(tab[i, :, j, D]))
            assert (np.abs(applied[i, :, j] - (a0[:, j] + alpha * ff0[:, j])) <= room).all(), (alpha, j)
        assert (applied[i] >= lo - 2 * np.spacing(abs(lo))).all() and (applied[i] <= hi + 2 * np.spacing(hi)).all(), alpha
        assert (np.abs(applied[i]) < 1.0).all()
    # alpha = 1 puts a clamped component on its bound
    on = np.where((cl[:, None] >> (2 + np.arange(2)) & 1) != 0, hi, lo)
    held = (cl[:, None] >> np.arange(2) & 1) != 0
    assert (np.abs(applied[0] - on)[held] <= 2 * np.spacing(hi)).all()
    for s in (nom_h, cand, knots):
        s.close()
