"""os2rc_ilqr_backward (include/os2r_control.h): the host side -- the header against the one table of gym_os2r_amd/control.py, the
exports of libos2r_control.so, every refusal through ctypes without a device, the resources of the eight kernels in the built
library, the numpy restatement the GPU tests compare with against the textbook recursion, against os2r_lqr_gains' restatement
and against an exact LQ problem, and the argument checks of HipSim.ilqr_backward that need no device.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from gym_os2r_amd import abi

sys.path.insert(0, os.path.join(ROOT, "tests"))
from header_check import _agrees, _is_pointer, _prototypes, checks_before_the_device, the_finite_and_symmetric_tests_make_no_hip_call  # noqa: E402

CASES = ((10, 4, 70), (4, 3, 3), (6, 2, 33), (8, 2, 33))



def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import control
    protos = _prototypes("os2r_control.h", "os2rc")
    assert [p[0] for p in protos] == list(control.ENTRY_POINTS) == ["os2rc_abi_version", "os2rc_last_error", "os2rc_ilqr_backward"]
    lib = control.load()
    for name, ret, args in protos:
        argtypes = control.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2rc_last_error" else C.c_int)
    args = protos[2][2]
    assert len(args) == 24 and args[9] == "double mu" and control.ENTRY_POINTS["os2rc_ilqr_backward"][9] is C.c_double
    with open(os.path.join(ROOT, "include", "os2r_control.h")) as f:
        header = f.read()
    assert re.search(r"#define OS2R_CONTROL_ABI_VERSION 1\b", header) and re.search(r"#define OS2RC_MAX_ALPHAS 16\b", header)
    assert lib.os2rc_abi_version() == control.ABI_VERSION == 1 and control.MAX_ALPHAS == 16
    # the struct of the header, field by field
    body = re.search(r"typedef struct Os2rControlLayout \{(.*?)\} Os2rControlLayout;", re.sub(r"/\*.*?\*/", " ", header, flags=re.S), re.S).group(1)
    fields = [re.sub(r"\[.*", "", d.split()[-1]) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in control.Os2rControlLayout._fields_]
    assert C.sizeof(control.Os2rControlLayout) == 4 * (4 + 12) and control.MAX_OBS == 12
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", control.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(control.ENTRY_POINTS)
    # and nothing was added to libos2r.so or its header for it
    with open(os.path.join(ROOT, "include", "os2r.h")) as f:
        assert "ilqr" not in f.read()


def test_slot_columns_reads_the_task():
    from gym_os2r_amd import control
    from helpers import make_config
    from test_gpu_lqr_gains import slot_columns
    for mode, normalized in (("free_hip", False), ("fixed_hip_torque", False), ("free_hip", True), ("simple", False)):
        cfg = make_config(mode, "StraightV1" if mode == "simple" else "BalancingV1", normalized, num_envs=8)[0]
        cols = control.slot_columns(cfg.task, cfg.model.nq)
        assert cols == slot_columns(cfg.task, cfg.model.nq) and len(cols) == cfg.task.obs_dim
        assert all(c == -1 for c in cols) == normalized
        lay = control.layout(abi.F32, cfg.model.nq, 3, cols)
        assert (lay.dtype, lay.nq, lay.device, lay.obs_dim) == (abi.F32, cfg.model.nq, 3, len(cols))
        assert list(lay.slot_col) == cols + [-1] * (12 - len(cols))


def test_refusals_come_through_ctypes_without_a_device():
    """Every cause of include/os2r_control.h has its own message; all of them are found before the first HIP call (the pointers
    handed over as device memory here are host memory, and nothing is written)."""
    from gym_os2r_amd import control
    lib = control.load()
    nq, n = 3, 6
    buf = (C.c_double * 4096)()
    d = C.cast(buf, C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def Lay(**kw):
        lay = control.layout(abi.F64, nq, 0, [0, 1, 3, -1])
        for k, v in kw.items():
            if k == "slot0":
                lay.slot_col[0] = v
            else:
                setattr(lay, k, v)
        return C.byref(lay)

    def Qm(i=None, j=None, v=0.0):
        m = np.eye(n)
        if i is not None:
            m[i, j] = v
        return (C.c_double * (n * n))(*m.reshape(-1))

    def Rm(*v):
        return (C.c_double * 4)(*(v or (0.1, 0.0, 0.0, 0.1)))

    def Al(*v):
        return (C.c_double * len(v))(*v)
    good = dict(lay=Lay(), K=1, M=4, a=d, b=d, lx=None, lu=None, q=Qm(), r=Rm(), mu=0.0, pf=None, vf=None, g=d, ff=None, po=None, vo=None,
                fl=None, dv=None, act=None, obs=None, al=None, nal=0, w=None)
    table = dict(w=d, act=d, obs=d, al=Al(1.0, 0.5), nal=2)

    def call(**kw):
        a = dict(good, **kw)
        return lib.os2rc_ilqr_backward(*[a[k] for k in good], None)
    # a null layout comes first: with nothing at all in the arguments it is what is named
    assert lib.os2rc_ilqr_backward(*[0.0 if t is C.c_double else None if _is_pointer(t) else 0
                                     for t in control.ENTRY_POINTS["os2rc_ilqr_backward"]]) == abi.ERR_INVALID
    assert lib.os2rc_last_error() == b"os2rc_ilqr_backward: null layout"
    seen = set()
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(dtype=-1)), b"dtype must be"),
                    (dict(lay=Lay(nq=1)), b"nq must be 2..5"), (dict(lay=Lay(nq=6)), b"nq must be 2..5"),
                    (dict(K=0), b"nknots must be >= 1"), (dict(M=0), b"ntraj must be >= 1"), (dict(K=-1), b"nknots must be >= 1"),
                    (dict(M=2 ** 40), b"ntraj exceeds"),
                    (dict(a=None), b"null a_dev"), (dict(b=None), b"null b_dev"), (dict(q=None), b"null q_host"), (dict(r=None), b"null r_host"),
                    (dict(q=Qm(1, 2, nan)), b"Q must be finite"), (dict(q=Qm(0, 0, -inf)), b"Q must be finite"),
                    (dict(q=Qm(1, 2, 0.5)), b"Q must be exactly symmetric"),
                    (dict(r=Rm(0.1, nan, nan, 0.1)), b"R must be finite"), (dict(r=Rm(inf, 0.0, 0.0, 0.1)), b"R must be finite"),
                    (dict(r=Rm(0.1, 0.01, 0.02, 0.1)), b"R must be exactly symmetric"),
                    (dict(mu=nan), b"mu must be finite"), (dict(mu=inf), b"mu must be finite"), (dict(mu=-inf), b"mu must be finite"),
                    (dict(mu=-1e-300), b"mu must be >= 0"),
                    (dict(g=None), b"all outputs are null"), (dict(g=None, fl=d), b"all outputs are null"),
                    (dict(table, act=None), b"weights need actions_dev, obs_dev and alpha_host"),
                    (dict(table, obs=None), b"weights need actions_dev, obs_dev and alpha_host"),
                    (dict(table, al=None), b"weights need actions_dev, obs_dev and alpha_host"),
                    (dict(table, nal=0), b"nalpha must be 1..16"), (dict(table, al=Al(*[1.0] * 17), nal=17), b"nalpha must be 1..16"),
                    (dict(table, al=Al(1.0, nan)), b"alpha must be finite"), (dict(table, al=Al(-inf, 1.0)), b"alpha must be finite"),
                    (dict(table, lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"), (dict(table, lay=Lay(obs_dim=13)), b"obs_dim must be 1..12"),
                    (dict(table, lay=Lay(slot0=n)), b"slot_col entries must be -1..n-1"),
                    (dict(table, lay=Lay(slot0=-2)), b"slot_col entries must be -1..n-1")]
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.os2rc_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(b"os2rc_ilqr_backward: "), (kw.keys(), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases}) == 22            # each cause has a text of its own
    assert not any(buf)                                             # a refused call wrote nothing
    texts = checks_before_the_device("os2r_control_capi.hip", "os2rc_ilqr_backward", ("layout_refusal", "slots_refusal"))
    assert len(texts) == 22
    the_finite_and_symmetric_tests_make_no_hip_call()


def test_kernel_resources():
    """All eight kernels ({float, double} x nq 2..5) are in the built library, none in libos2r.so, and none uses scratch:
    private_segment_fixed_size 0, no VGPR spill and no AGPRs in the code-object metadata.  Two workgroups of the widest one fit a
    CU's LDS.  These are the conditions os2r_lqr_gains' kernels are held to."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib, control
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(control.LIB_PATH)
    meta = kernel_meta.kernel_meta(control.LIB_PATH)
    assert len(meta) == 8 and not any("lqr_gains_kernel<" in k for k in meta), sorted(meta)
    for real in ("float", "double"):
        for nq in (2, 3, 4, 5):
            (name,) = [k for k in meta if f"ilqr_backward_kernel<{real}, {nq}>" in k]
            m = meta[name]
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
            assert m["agpr_count"] == 0 and m["vgpr_count"] <= 256, (name, m)
            assert 2 * m["group_segment_fixed_size"] <= 160 * 1024, (name, m)
    assert not any("ilqr_backward_kernel" in k for k in kernel_meta.kernel_meta(_lib.LIB_PATH))


def _textbook(A, B, Q, R, K, mu, lx, lu, p_final):
    """The regularised backward pass with linalg.solve in fp64 (kernel layouts in, kernel layouts out; P_final = Q)."""
    n, L = A.shape[0], A.shape[2]
    M = L // K
    P, p = np.repeat(Q[None], M, 0), p_final.T.copy()
    gains, ff, dv = np.zeros((K, 2, n, M)), np.zeros((K, 2, M)), np.zeros((K, 2, M))
    I2 = np.eye(2)
    for k in range(K - 1, -1, -1):
        s = slice(k * M, (k + 1) * M)
        a, b = A[:, :, s].transpose(2, 0, 1), B[:, :, s].transpose(2, 0, 1)
        at, bt = a.transpose(0, 2, 1), b.transpose(0, 2, 1)
        Qx, Qu = lx[:, s].T + (at @ p[:, :, None])[:, :, 0], lu[:, s].T + (bt @ p[:, :, None])[:, :, 0]
        Qxx, Quu, Qux = Q + at @ P @ a, R + bt @ P @ b, bt @ P @ a
        kf = -np.linalg.solve(Quu + mu * I2, Qu[:, :, None])[:, :, 0]
        Kf = -np.linalg.solve(Quu + mu * I2, Qux)
        Kt = Kf.transpose(0, 2, 1)
        p = Qx + (Kt @ Quu @ kf[:, :, None])[:, :, 0] + (Kt @ Qu[:, :, None])[:, :, 0] + (Qux.transpose(0, 2, 1) @ kf[:, :, None])[:, :, 0]
        P = Qxx + Kt @ Quu @ Kf + Kt @ Qux + Qux.transpose(0, 2, 1) @ Kf
        P = 0.5 * (P + P.transpose(0, 2, 1))
        gains[k], ff[k] = -Kf.transpose(1, 2, 0), kf.T
        dv[k, 0] = (kf * Qu).sum(1)
        dv[k, 1] = 0.5 * (kf[:, None, :] @ Quu @ kf[:, :, None])[:, 0, 0]
    return dict(gains=gains, ff=ff, P=P.transpose(1, 2, 0), p=p.T, dv=dv)


@pytest.mark.parametrize("mu", [0.0, 0.5])
def test_the_restatement_agrees_with_the_textbook_recursion(mu):
    """The numpy restatement of tests/test_gpu_ilqr_backward.py (the GPU tests' yardstick) against k = -(Quu + mu I)^-1 Qu,
    Kf = -(Quu + mu I)^-1 Qux, Vx = Qx + Kf'Quu k + Kf'Qu + Qux'k, Vxx = Qxx + Kf'Quu Kf + Kf'Qux + Qux'Kf, symmetrised, with
    linalg.solve in fp64: the same sums in another order, so the two differ by rounding only -- a knot forms each entry from
    about 2n products (n <= 10) and passes it through a 2 x 2 solve whose condition is below 100 here, and the recursion
    contracts: 1e3 eps relative to the largest entry bounds it with room (the tolerance and the reasoning of
    tests/test_lqr_gains_host.py; the worst seen is printed).  Nothing is refused and everything is finite."""
    from test_gpu_ilqr_backward import gradients, restate
    from test_gpu_lqr_gains import R_COST, synthetic
    # what is restated is the header's text: its steps are there, in the order the restatement follows
    with open(os.path.join(ROOT, "include", "os2r_control.h")) as f:
        header = " ".join(f.read().replace("\n *", " ").split())
    steps = ["1. PB, S00, S01, S11 as in os2r_lqr_gains step 1", "T00 = S00 + mu, T11 = S11 + mu, T01 = S01", "2. det = T00 T11 - T01 T01",
             "3. PA, G as in os2r_lqr_gains step 3", "4. K[0][j] = (T11 G[0][j] - T01 G[1][j]) / det",
             "5. Qx[j] = lx[j] + sum_l A[l][j] p[l]; Qu[c] = lu[c] + sum_l B[l][c] p[l]", "6. k0 = -((T11 Qu0 - T01 Qu1) / det)",
             "7. for i <= j: P'[i][j] = ((Q[i][j] + sum_l A[l][i] PA[l][j]) - (G[0][i] K[0][j] + G[1][i] K[1][j])) - mu (K[0][i] K[0][j] + K[1][i] K[1][j])",
             "8. p'[j] = (Qx[j] + (G[0][j] k0 + G[1][j] k1)) + mu (K[0][j] k0 + K[1][j] k1)",
             "9. dv[k][0] = k0 Qu0 + k1 Qu1; dv[k][1] = 0.5 (((S00 k0) k0 + (S11 k1) k1) + 2 ((S01 k0) k1))",
             "W[k][j][D][i M + m] = (a0_j + alpha_i k_j) - acc"]
    at = [header.find(t) for t in steps]
    assert all(a >= 0 for a in at) and at == sorted(at), at
    worst = {np.float32: 0.0, np.float64: 0.0}
    for n, K, M in CASES:
        A, B, Q = synthetic(n, K * M)
        lx, lu, pv = gradients(n, K * M, M)
        want = _textbook(A, B, Q, R_COST, K, mu, lx, lu, pv)
        for dtype in (np.float64, np.float32):
            got = restate(A, B, Q, R_COST, K, dtype, mu=mu, lx=lx, lu=lu, P_final=np.repeat(Q[:, :, None], M, 2), p_final=pv)
            assert got["weights"] is None and not got["flags"].any()
            assert np.array_equal(got["P"], got["P"].transpose(1, 0, 2))
            tol = 1e3 * np.finfo(dtype).eps
            for o, w in want.items():
                assert got[o].dtype == dtype and got[o].shape == w.shape and np.isfinite(got[o]).all(), (o, n, dtype)
                err = np.abs(got[o] - w).max() / np.abs(w).max()
                worst[dtype] = max(worst[dtype], err / np.finfo(dtype).eps)
                assert err <= tol, (o, n, K, M, dtype, err)
    print(f"mu = {mu}: worst error {worst[np.float32]:.1f} eps in fp32, {worst[np.float64]:.1f} eps in fp64")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_without_affine_terms_the_restatement_is_that_of_lqr_gains(dtype):
    from test_gpu_ilqr_backward import _same, gradients, restate
    from test_gpu_lqr_gains import R_COST, synthetic
    from test_gpu_lqr_gains import restate as restate_lqr
    for n, K, M in CASES:
        A, B, Q = synthetic(n, K * M)
        rng = np.random.default_rng(11)
        cols = [0, n - 1, -1, 1]
        kw = dict(actions=rng.uniform(-1.3, 1.3, (K * M, 2)), obs=rng.uniform(-2, 2, (K * M, 4)), cols=cols)
        g, P, f, W = restate_lqr(A, B, Q, R_COST, K, 1, dtype, **kw)
        got = restate(A, B, Q, R_COST, K, dtype, mu=0.0, alphas=(0.0, 1.0), **kw)
        _same(got["gains"], g, "gains")
        _same(got["P"], P, "P")
        _same(got["flags"], f, "flags")
        assert np.array_equal(got["weights"][..., :M], W) and np.array_equal(got["weights"][..., M:], W)     # k = 0: alpha does nothing
        for o in ("ff", "p", "dv"):                                  # by value: a zero's sign is not part of the contract
            assert got[o].dtype == dtype and not got[o].any(), o
        # gradients move ff, p and dv, and with mu = 0 neither the gains nor P
        lx, lu, pv = gradients(n, K * M, M)
        got = restate(A, B, Q, R_COST, K, dtype, mu=0.0, lx=lx, lu=lu, p_final=pv, alphas=(0.0, 1.0), **kw)
        _same(got["gains"], g, "gains")
        _same(got["P"], P, "P")
        assert np.array_equal(got["weights"][..., :M], W) and not np.array_equal(got["weights"][..., M:], W)
        assert all(np.abs(got[o]).max() > 1e-3 for o in ("ff", "p", "dv"))


@pytest.mark.parametrize("n,K,M", [(10, 6, 5), (4, 8, 3)])
def test_the_predicted_cost_change_of_an_exact_lq_problem_is_the_actual_one(n, K, M):
    """Time-varying linear dynamics, cost 1/2 x'Qx + 1/2 u'Ru per knot plus 1/2 x'Qx at the end, a random nominal: the model is
    exact, so the cost of the rollout under u = u_k + alpha k_k - K_k (x - x_k) changes by alpha sum dv0 + alpha^2 sum dv1, to
    rounding: 1e-12 of the largest nominal cost (measured 3.2e-16)."""
    from test_gpu_ilqr_backward import restate
    from test_gpu_lqr_gains import R_COST, synthetic
    A, B, Q = synthetic(n, K * M)
    rng = np.random.default_rng(3)
    x0, U = rng.standard_normal((M, n)), rng.standard_normal((K, M, 2))
    a = A.reshape(n, n, K, M).transpose(2, 3, 0, 1)                 # [K, M, n, n]
    b = B.reshape(n, 2, K, M).transpose(2, 3, 0, 1)

    def rollout(policy):
        x, xs, us, cost = x0, [], [], np.zeros(M)
        for k in range(K):
            u = policy(k, x)
            xs.append(x)
            us.append(u)
            cost = cost + 0.5 * np.einsum("mi,ij,mj->m", x, Q, x) + 0.5 * np.einsum("mi,ij,mj->m", u, R_COST, u)
            x = np.einsum("mij,mj->mi", a[k], x) + np.einsum("mij,mj->mi", b[k], u)
        return np.stack(xs), np.stack(us), x, cost + 0.5 * np.einsum("mi,ij,mj->m", x, Q, x)
    X, _, xK, J0 = rollout(lambda k, x: U[k])
    lx = (X @ Q).transpose(2, 0, 1).reshape(n, K * M)
    lu = (U @ R_COST).transpose(2, 0, 1).reshape(2, K * M)
    out = restate(A, B, Q, R_COST, K, np.float64, mu=0.0, lx=lx, lu=lu, p_final=(xK @ Q).T)
    assert not out["flags"].any()
    gains, ff, dv = out["gains"].transpose(0, 3, 1, 2), out["ff"].transpose(0, 2, 1), out["dv"]
    for alpha in (1.0, 0.5):
        _, _, _, J = rollout(lambda k, x: U[k] + alpha * ff[k] - np.einsum("mij,mj->mi", gains[k], x - X[k]))
        model = alpha * dv[:, 0].sum(0) + alpha ** 2 * dv[:, 1].sum(0)
        err = np.abs((J - J0) - model).max() / J0.max()
        print(f"n = {n}, K = {K}, alpha = {alpha}: |actual - predicted| / max nominal cost = {err:.2e}")
        assert (model < 0).all() and err <= 1e-12, (alpha, err)


def _bare(dtype, n=8, nq=3, D=4):
    """A HipSim that never met a device: enough of it for the checks that run before the library is called."""
    import torch
    from gym_os2r_amd.sim import HipSim
    s = HipSim.__new__(HipSim)
    s.N, s.nq, s.D, s.dtype, s.device = n, nq, D, dtype, torch.device("cpu")
    s._h = None
    s._lib = None      # (and it has no cfg: filling the layout would raise AttributeError, not ValueError)
    return s


def test_python_argument_errors_need_no_device():
    import torch
    from gym_os2r_amd.sim import HipSim
    assert callable(HipSim.ilqr_backward) and callable(HipSim.ilqr_backward_into)
    s = _bare(torch.float64)
    n, L, D, f64 = 6, 8, 4, torch.float64
    A, B = torch.zeros(L, n, n, dtype=f64), torch.zeros(L, n, 2, dtype=f64)
    Q, R = torch.eye(n, dtype=f64), 0.1 * torch.eye(2, dtype=f64)
    nan, inf = float("nan"), float("inf")
    act, obs = torch.zeros(L, 2, dtype=f64), torch.zeros(L, D, dtype=f64)
    a, b = torch.zeros(n, n, L, dtype=f64), torch.zeros(n, 2, L, dtype=f64)
    K, M = 2, 4
    g = torch.zeros(K, 2, n, M, dtype=f64)
    for bq in (Q.clone().index_put_((torch.tensor(1), torch.tensor(2)), torch.tensor(0.5, dtype=f64)), nan * Q, torch.eye(5, dtype=f64), "x", None):
        with pytest.raises(ValueError, match="^ilqr_backward: Q"):
            s.ilqr_backward(A, B, bq, R, knots=1)
        with pytest.raises(ValueError, match="^ilqr_backward: Q"):
            s.ilqr_backward_into(a, b, bq, R, knots=K, gains_out=g)
    for br in ([[0.1, nan], [nan, 0.1]], [[0.1, 0.01], [0.02, 0.1]], torch.eye(3), 0.1, None):
        with pytest.raises(ValueError, match="^ilqr_backward: R"):
            s.ilqr_backward(A, B, Q, br, knots=1)
        with pytest.raises(ValueError, match="^ilqr_backward: R"):
            s.ilqr_backward_into(a, b, Q, br, knots=K, gains_out=g)
    for mu in (nan, inf, -0.1, "x", None):
        with pytest.raises(ValueError, match="^ilqr_backward: mu"):
            s.ilqr_backward(A, B, Q, R, knots=1, mu=mu)
        with pytest.raises(ValueError, match="^ilqr_backward: mu"):
            s.ilqr_backward_into(a, b, Q, R, knots=K, mu=mu, gains_out=g)
    with pytest.raises(ValueError, match="^ilqr_backward: nothing asked for"):
        s.ilqr_backward(A, B, Q, R, knots=1, want_gains=False, want_ff=False, want_dv=False, want_flags=True)
    with pytest.raises(ValueError, match="^ilqr_backward: nothing asked for"):
        s.ilqr_backward_into(a, b, Q, R, knots=K, flags_out=torch.zeros(K, M, dtype=torch.uint8))
    for kw in (dict(), dict(actions=act), dict(actions=act, obs=obs), dict(obs=obs, alphas=(1.0,))):
        with pytest.raises(ValueError, match="^ilqr_backward: weights need actions, obs"):
            s.ilqr_backward(A, B, Q, R, knots=1, want_weights=True, **kw)
        with pytest.raises(ValueError, match="^ilqr_backward: weights need actions, obs"):
            s.ilqr_backward_into(a, b, Q, R, knots=K, weights_out=torch.zeros(K, 2, D + 1, M, dtype=f64), **kw)
    for al, msg in (((), "between 1 and 16 alphas"), ([1.0] * 17, "between 1 and 16 alphas"), ((1.0, nan), "every alpha must be finite"),
                    ((1.0, "x"), "alphas must be a sequence of numbers"), (0.5, "alphas must be a sequence of numbers")):
        with pytest.raises(ValueError, match="^ilqr_backward: " + msg):
            s.ilqr_backward(A, B, Q, R, knots=1, want_weights=True, actions=act, obs=obs, alphas=al)
    for kw in (dict(knots=0), dict(knots=-2)):
        with pytest.raises(ValueError, match="^ilqr_backward: knots must be >= 1"):
            s.ilqr_backward(A, B, Q, R, **kw)
    for kn in (3, 16):
        with pytest.raises(ValueError, match="^ilqr_backward: .*no multiple of knots"):
            s.ilqr_backward(A, B, Q, R, knots=kn)
    for x, y in ((A.float(), B), (A, B.float()), (A[:, :5], B), (A, B[:, :, :1]), (A.permute(1, 2, 0), B), (A, B[:4]), (A.numpy(), B), (A, None)):
        with pytest.raises(ValueError, match="^ilqr_backward: "):
            s.ilqr_backward(x, y, Q, R, knots=1)
    for kw in (dict(lx=torch.zeros(L, n + 1, dtype=f64)), dict(lu=torch.zeros(L, 3, dtype=f64)), dict(P_final=torch.zeros(L, n, n, dtype=f64)),
               dict(p_final=torch.zeros(L, n, dtype=f64)),
               dict(want_weights=True, actions=act, obs=torch.zeros(L, D + 1, dtype=f64), alphas=(1.0,))):
        with pytest.raises(ValueError, match="^ilqr_backward: .*expected shape"):
            s.ilqr_backward(A, B, Q, R, knots=2, **kw)                                         # M = 4 here
    # the kernel-layout variant: every tensor is what the kernel assumes, or the call is refused before the library is reached
    w2 = torch.zeros(K, 2, D + 1, 2 * M, dtype=f64)
    for kw in (dict(A=A, gains_out=g),                                                    # the public layout is not the kernel's
               dict(A=a.float(), gains_out=g), dict(B=b[:, :1], gains_out=g), dict(B=None, gains_out=g),
               dict(A=torch.zeros(n, L, n, dtype=f64).permute(0, 2, 1), gains_out=g),           # not contiguous
               dict(gains_out=torch.zeros(K, M, 2, n, dtype=f64)), dict(gains_out=g.float()),
               dict(ff_out=torch.zeros(K, M, 2, dtype=f64)), dict(dv_out=torch.zeros(K, 2, M + 1, dtype=f64)),
               dict(P_out=torch.zeros(M, n, n, dtype=f64)), dict(p_out=torch.zeros(M, n, dtype=f64)),
               dict(gains_out=g, P_final=torch.zeros(n, n, L, dtype=f64)), dict(gains_out=g, p_final=torch.zeros(n, L, dtype=f64)),
               dict(gains_out=g, lx=torch.zeros(L, n, dtype=f64)), dict(gains_out=g, lu=torch.zeros(2, L, dtype=torch.float32)),
               dict(gains_out=g, flags_out=torch.zeros(K, M, dtype=torch.int32)), dict(gains_out=g, flags_out=torch.zeros(M, K, dtype=torch.uint8)),
               dict(weights_out=torch.zeros(K, 2, D + 1, M, dtype=f64), actions=act, obs=obs, alphas=(1.0, 0.5)),       # one alpha's worth
               dict(weights_out=w2, actions=act[:4], obs=obs, alphas=(1.0, 0.5)),
               dict(weights_out=w2, actions=act, obs=obs.float(), alphas=(1.0, 0.5)),
               dict(gains_out=[0.0] * 8)):
        args = dict(dict(A=a, B=b), **kw)
        with pytest.raises(ValueError, match="^ilqr_backward"):
            s.ilqr_backward_into(args.pop("A"), args.pop("B"), Q, R, knots=K, **args)
    # what linearize() returns is taken without a copy
    view = torch.zeros(n, n, L, dtype=f64).permute(2, 0, 1)
    assert view.permute(1, 2, 0).contiguous().data_ptr() == view.data_ptr()
