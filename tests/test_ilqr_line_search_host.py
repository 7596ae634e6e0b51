"""os2rs_ilqr_line_search (include/os2r_search.h): the host side -- the header against the one table of gym_os2r_amd/search.py, the
exports of libos2r_search.so, the other libraries as they were, every refusal through ctypes without a device, the resources of
the eight kernels in the built library, the numpy restatement the GPU tests compare with against a direct formula, its selection
logic on crafted inputs, its agreement with the torch statement of examples/ilqr_balancing.py, and the argument checks of
HipSim.ilqr_line_search that need no device.  No GPU needed."""
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
from header_check import _agrees, _header, _is_pointer, _prototypes, checks_before_the_device, the_finite_and_symmetric_tests_make_no_hip_call  # noqa: E402

NAMES = ["os2rs_abi_version", "os2rs_last_error", "os2rs_ilqr_line_search"]
CONTROL_KERNELS = 8



def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import control, search
    protos = _prototypes("os2r_search.h", "os2rs")
    assert [p[0] for p in protos] == list(search.ENTRY_POINTS) == NAMES
    lib = search.load()
    for name, ret, args in protos:
        argtypes = search.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2rs_last_error" else C.c_int)
    args = protos[2][2]
    assert len(args) == 24 and args[:5] == ["const Os2rControlLayout* layout", "int32_t nknots", "int64_t ntraj", "int32_t nalpha", "uint32_t flags"]
    assert args[-1] == "void* stream" and search.ENTRY_POINTS["os2rs_ilqr_line_search"][4] is C.c_uint32
    header = _header("os2r_search.h")
    assert re.search(r"#define OS2R_SEARCH_ABI_VERSION 1\b", header) and re.search(r"#define OS2RS_ACCEPT_ALWAYS 1u\b", header)
    assert '#include "os2r_control.h"' in header and "typedef struct" not in header      # the layout is os2r_control.h's
    assert lib.os2rs_abi_version() == search.ABI_VERSION == 1 and search.ACCEPT_ALWAYS == 1
    assert search.Os2rControlLayout is control.Os2rControlLayout and search.layout is control.layout
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", search.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(search.ENTRY_POINTS)


def test_the_other_libraries_are_as_they_were():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib, control
    for name in ("os2r.h", "os2r_control.h", "os2r_record.h"):
        assert "line_search" not in _header(name), name
    assert list(control.ENTRY_POINTS) == ["os2rc_abi_version", "os2rc_last_error", "os2rc_ilqr_backward"]
    meta = kernel_meta.kernel_meta(control.LIB_PATH)
    assert len(meta) == CONTROL_KERNELS and all("ilqr_backward_kernel<" in k for k in meta), sorted(meta)
    assert not any("line_search" in k for k in kernel_meta.kernel_meta(_lib.LIB_PATH))
    for path in (_lib.LIB_PATH, control.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert "os2rs_" not in out, path


def test_refusals_come_through_ctypes_without_a_device():
    """Every cause of include/os2r_search.h has its own message; all of them are found before the first HIP call (the pointers
    handed over as device memory here are host memory, and nothing is written)."""
    from gym_os2r_amd import control, search
    lib = search.load()
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
    good = dict(lay=Lay(), K=2, M=4, nal=2, flags=0, kobs=d, eobs=d, act=d, done=None, tgt=d, q=Qm(), r=Rm(), qf=None, cost=d, an=None,
                on=None, en=None, lx=None, lu=None, pf=None, choice=d, index=None, cc=None)
    assert len(good) + 1 == len(search.ENTRY_POINTS["os2rs_ilqr_line_search"])

    def call(**kw):
        a = dict(good, **kw)
        return lib.os2rs_ilqr_line_search(*[a[k] for k in good], None)
    # a null layout comes first: with nothing at all in the arguments it is what is named
    assert lib.os2rs_ilqr_line_search(*[None if _is_pointer(t) else 0 for t in search.ENTRY_POINTS["os2rs_ilqr_line_search"]]) == abi.ERR_INVALID
    assert lib.os2rs_last_error() == b"os2rs_ilqr_line_search: null layout"
    seen = set()
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(dtype=-1)), b"dtype must be"),
             (dict(lay=Lay(nq=1)), b"nq must be 2..5"), (dict(lay=Lay(nq=6)), b"nq must be 2..5"),
             (dict(lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"), (dict(lay=Lay(obs_dim=13)), b"obs_dim must be 1..12"),
             (dict(lay=Lay(slot0=n)), b"slot_col entries must be -1..n-1"), (dict(lay=Lay(slot0=-2)), b"slot_col entries must be -1..n-1"),
             (dict(K=0), b"nknots must be >= 1"), (dict(K=-1), b"nknots must be >= 1"), (dict(M=0), b"ntraj must be >= 1"),
             (dict(M=-5), b"ntraj must be >= 1"), (dict(nal=0), b"nalpha must be 1..16"), (dict(nal=17), b"nalpha must be 1..16"),
             (dict(K=1024, M=2 ** 17, nal=16), b"exceeds 2^31 - 1"), (dict(K=1, M=2 ** 31, nal=1), b"exceeds 2^31 - 1"),
             (dict(M=2 ** 62), b"exceeds 2^31 - 1"),
             (dict(flags=2), b"unknown flag bits"), (dict(flags=0x80000001), b"unknown flag bits"),
             (dict(kobs=None), b"null knot_obs_dev"), (dict(eobs=None), b"null end_obs_dev"), (dict(act=None), b"null act_dev"),
             (dict(tgt=None), b"null target_dev"), (dict(q=None), b"null q_host"), (dict(r=None), b"null r_host"),
             (dict(cost=None), b"null cost_dev"), (dict(choice=None), b"null choice_dev"),
             (dict(q=Qm(1, 2, nan)), b"Q must be finite"), (dict(q=Qm(0, 0, -inf)), b"Q must be finite"),
             (dict(r=Rm(0.1, nan, nan, 0.1)), b"R must be finite"), (dict(r=Rm(inf, 0.0, 0.0, 0.1)), b"R must be finite"),
             (dict(qf=Qm(3, 3, nan)), b"Qf must be finite"), (dict(qf=Qm(1, 0, inf)), b"Qf must be finite"),
             (dict(q=Qm(1, 2, 0.5)), b"Q must be exactly symmetric"), (dict(r=Rm(0.1, 0.01, 0.02, 0.1)), b"R must be exactly symmetric"),
             (dict(qf=Qm(4, 0, 1e-300)), b"Qf must be exactly symmetric")]
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.os2rs_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(b"os2rs_ilqr_line_search: "), (kw.keys(), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases}) == 24            # each cause has a text of its own
    assert not any(buf)                                             # a refused call wrote nothing
    # 2^31 - 1 lanes themselves are taken by the checks (the next refusal is about something else)
    assert call(K=1, M=2 ** 31 - 1, nal=1, q=None) == abi.ERR_INVALID and lib.os2rs_last_error().endswith(b"null q_host")
    texts = checks_before_the_device("os2r_search_capi.hip", "os2rs_ilqr_line_search", ("layout_refusal", "slots_refusal"))
    assert len(texts) == 24
    the_finite_and_symmetric_tests_make_no_hip_call()


def test_kernel_resources():
    """All eight kernels ({float, double} x nq 2..5) are in the built library and none uses scratch: private_segment_fixed_size
    0, no VGPR spill and no AGPRs in the code-object metadata.  Two workgroups of the widest one fit a CU's LDS."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import search
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(search.LIB_PATH)
    meta = kernel_meta.kernel_meta(search.LIB_PATH)
    assert len(meta) == 8, sorted(meta)
    for real in ("float", "double"):
        for nq in (2, 3, 4, 5):
            (name,) = [k for k in meta if f"ilqr_line_search_kernel<{real}, {nq}>" in k]
            m = meta[name]
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
            assert m["agpr_count"] == 0 and m["vgpr_count"] <= 128, (name, m)          # 16 waves of a workgroup on four SIMDs
            assert 2 * m["group_segment_fixed_size"] <= 160 * 1024, (name, m)


STEPS = ["1. at knot k, o is row j of knot_obs[k] and a_c = clamp(act[k][j][c], -1, 1)",
         "2. e[c], c < n, is o[d] - target[m][d] for the lowest raw slot d with slot_col[d] == c, and 0 if no slot shows column c",
         "3. gx[r] = sum_c Q[r][c] e[c] over all c < n; sx = 0.5 sum_r e[r] gx[r]",
         "4. gu[c] = R[c][0] a_0 + R[c][1] a_1; su = 0.5 (a_0 gu[0] + a_1 gu[1])",
         "5. J = (J + sx) + su, starting from J = 0, with k ascending",
         "6. behind the last knot e is formed from end_obs[j]: gf[r] = sum_c Qf[r][c] e[c]; J = J + 0.5 sum_r e[r] gf[r]",
         "7. candidate i is acceptable when J is finite (tested on the bit pattern), no done entry of lane j is nonzero, and either OS2RS_ACCEPT_ALWAYS is set or J < cost[m]",
         "ties to the lowest i, and -1 if none is acceptable",
         "8. where choice[m] = i >= 0, with j = i M + m: cost[m] = J; act_nom[k][m][c] = a_c (clamped); obs_nom[k][m][:] = o (all D slots)",
         "lx[r][k M + m] = gx[r]; lu[c][k M + m] = gu[c]; pvec_final[r][m] = gf[r]"]


def test_the_restatement_follows_the_header_and_agrees_with_the_direct_formula():
    """What is restated is the header's text: its steps are there, in the order the restatement's comments follow.  Then the
    restatement's costs against 1/2 e'Qe + 1/2 a'Ra per knot plus 1/2 e'Qf e in one fp64 einsum each, on the same rounded inputs
    and the same e: the two are the same sums in another order, so a cost differs by at most (operations a term passes through)
    x eps x (the sum of the absolute values of its products) -- the recursive-summation bound, Higham (2002), eq. 4.4, taken
    with the count of one whole cost, K (n (n - 1) + (n - 1) + 5) + n (n - 1) + n additions.  The worst ratio to that bound is
    printed."""
    import inspect
    import test_gpu_ilqr_line_search as t
    header = " ".join(_header("os2r_search.h").replace("\n *", " ").split())
    at = [header.find(s) for s in STEPS]
    assert all(a >= 0 for a in at) and at == sorted(at), at
    src = inspect.getsource(t.restate)
    marks = [src.index(f"# {i}.") for i in range(1, 9)]
    assert marks[2:] == sorted(marks[2:]) and marks[1] < marks[2] and marks[0] < marks[3]      # (step 2 and 3 are helpers, defined first)
    worst = {}
    for nq, D, K, M, nalpha, _ in t.SHAPES:
        c = t.crafted(nq, D, K, M, nalpha)
        n, N = 2 * nq, nalpha * M
        for dtype in (np.float64, np.float32):
            got = t.restate_crafted(c, dtype, always=True)["cand_cost"].reshape(N)
            eps = np.finfo(dtype).eps
            r = lambda x: np.asarray(x).astype(dtype).astype(np.float64)
            Q, R, Qf = r(c["Q"]), r(c["R"]), r(c["Qf"])
            tgt = np.tile(c["target"].astype(dtype), (nalpha, 1))

            def err(o):
                e = np.zeros(o.shape[:-1] + (n,), dtype)
                for col in range(n):
                    shows = [d for d in range(D) if c["cols"][d] == col]
                    if shows:
                        e[..., col] = o[..., shows[0]] - tgt[:, shows[0]]
                return e.astype(np.float64)
            e, ef = err(c["knot_obs"].astype(dtype)), err(c["end_obs"].astype(dtype))
            a = np.clip(c["act"].astype(dtype), -1, 1).astype(np.float64)
            with np.errstate(all="ignore"):
                want = 0.5 * np.einsum("kji,il,kjl->j", e, Q, e) + 0.5 * np.einsum("kji,il,kjl->j", a, R, a) + 0.5 * np.einsum("ji,il,jl->j", ef, Qf, ef)
                size = 0.5 * np.einsum("kji,il,kjl->j", np.abs(e), np.abs(Q), np.abs(e)) + 0.5 * np.einsum("kji,il,kjl->j", np.abs(a), np.abs(R), np.abs(a)) \
                    + 0.5 * np.einsum("ji,il,jl->j", np.abs(ef), np.abs(Qf), np.abs(ef))
            finite = np.isfinite(want)
            assert np.array_equal(finite, np.isfinite(got)) and finite.sum() >= N - M
            ops = K * (n * (n - 1) + (n - 1) + 5) + n * (n - 1) + n
            ratio = (np.abs(got[finite].astype(np.float64) - want[finite]) / (ops * eps * size[finite] + np.finfo(np.float64).tiny)).max()
            worst[dtype.__name__] = max(worst.get(dtype.__name__, 0.0), ratio)
            assert ratio <= 1.0, (nq, D, K, M, nalpha, dtype, ratio)
    print("worst |restated - direct| over the recursive-summation bound:", {k: f"{v:.3f}" for k, v in worst.items()})


def test_selection_logic_of_the_restatement():
    import test_gpu_ilqr_line_search as t
    for nq, D, K, M, nalpha, _ in t.SHAPES[:1] + t.SHAPES[2:]:
        c = t.crafted(nq, D, K, M, nalpha)
        N = nalpha * M
        for dtype in (np.float64, np.float32):
            out = t.restate_crafted(c, dtype)
            choice, J, nom = out["choice"], out["cand_cost"], out["nominal"]
            was = {k: np.asarray(v).astype(dtype) for k, v in c["nominal"].items()}
            ms = np.arange(M)
            assert (choice[ms % 3 == 0] == -1).all()                                   # a nominal cost below every candidate
            tie = ms[(ms % 5 == 1) & (ms % 3 != 0) & (ms % 7 != 3) & (ms % 7 != 5)]
            assert len(tie) and (choice[tie] == 0).all() and all((t._bits(J[:, m]) == t._bits(J[0, m])).all() for m in tie)
            pair = ms[(ms % 5 == 2) & (ms % 3 != 0) & (ms % 7 != 5)]
            assert len(pair) and (choice[pair] == 1).all() and (J[1, pair] == J[2, pair]).all()
            nan = ms[ms % 7 == 3]
            assert len(nan) and np.isnan(J[0, nan]).all() and (choice[nan] != 0).all()
            unread = ms[(ms % 7 == 4) & (ms % 5 != 1)]
            assert len(unread) and np.isfinite(J[0, unread]).all()                     # the higher slot of a column shown twice is not read
            took = unread[choice[unread] == 0]
            assert all(np.isnan(nom["obs_nom"][K // 2, m, D - 1]) for m in took)       # ... but the row is copied whole
            ended = ms[(ms % 7 == 5) & (ms % 3 != 0)]
            assert len(ended) and (J[nalpha - 1, ended] == 0).all() and (choice[ended] != nalpha - 1).all() and (choice[ended] >= 0).all()
            # a trajectory that accepted nothing keeps every nominal byte, and its index entries are -1
            refused = choice < 0
            lanes = np.tile(refused, K)
            for name, rows in (("cost", refused), ("end_nom", refused)):
                assert (t._bits(nom[name][rows]) == t._bits(was[name][rows])).all(), name
            for name in ("act_nom", "obs_nom"):
                assert (t._bits(nom[name][:, refused]) == t._bits(was[name][:, refused])).all(), name
            for name, cols_ in (("lx", lanes), ("lu", lanes), ("p_final", refused)):
                assert (t._bits(nom[name][:, cols_]) == t._bits(was[name][:, cols_])).all(), name
            assert (out["index"][lanes] == -1).all()
            # an accepted one: the index of its candidate's knots, the candidate's cost and rows
            for m in ms[~refused][:8]:
                j = choice[m] * M + m
                assert [out["index"][k * M + m] for k in range(K)] == [k * N + j for k in range(K)]
                assert nom["cost"][m] == J[choice[m], m] < was["cost"][m]
                assert np.array_equal(nom["act_nom"][:, m], np.clip(c["act"][:, j].astype(dtype), -1, 1))
                assert (t._bits(nom["obs_nom"][:, m]) == t._bits(c["knot_obs"][:, j].astype(dtype))).all()
                assert np.array_equal(nom["end_nom"][m], c["end_obs"][j].astype(dtype))
            # ACCEPT_ALWAYS ignores cost: the best acceptable candidate of every trajectory
            free = t.restate_crafted(c, dtype, always=True)
            assert (free["choice"] >= 0).all() and np.array_equal(free["choice"][~refused], choice[~refused])
            with np.errstate(invalid="ignore"):
                okJ = np.where(np.isfinite(J) & ~(c["done"] != 0).any(0).reshape(nalpha, M), J, np.inf)
            assert np.array_equal(free["choice"], okJ.argmin(0))
    # a column shown twice reads its lowest slot: moving the higher one changes nothing, moving the lower one does
    nq, D, K, M, nalpha, _ = t.SHAPES[3]
    c = t.crafted(nq, D, K, M, nalpha)
    assert c["cols"][D - 1] == c["cols"][0] and c["cols"][1] == -1
    base = t.restate_crafted(c, np.float64, always=True)["cand_cost"]
    for slot, moves in ((D - 1, False), (1, False), (0, True)):
        k2 = c["knot_obs"].copy()
        k2[:, :, slot] += 1.0
        moved = t.restate_crafted(dict(c, knot_obs=k2), np.float64, always=True)["cand_cost"]
        fin = np.isfinite(base)
        assert (not np.array_equal(moved[fin], base[fin])) == moves, slot


def test_agrees_with_the_torch_statement_of_the_example():
    """Steps 3, 6 and 7 of examples/ilqr_balancing.py in torch, fp64, diagonal Q, the argmin taken per trajectory: the same
    choice; costs, lx, lu and p_final within the recursive-summation bound of test_the_restatement_..., (the additions of the
    restated sum) x eps x (the sum of the absolute values of its products), element by element."""
    import torch
    import test_gpu_ilqr_line_search as t
    nq, D, K, M, nal = 5, 10, 6, 37, 4
    rng = np.random.default_rng(5)
    n, N = 2 * nq, nal * M
    cols = [0, 1, 2, 3, 4, 5, 6, 7, -1, 9]
    slots = [d for d in range(D) if cols[d] >= 0]
    shown = [cols[d] for d in slots]
    target = rng.standard_normal((M, D))
    obs_k = target + 0.5 * rng.standard_normal((K, M, D))                 # the nominal
    end_obs = target + 0.5 * rng.standard_normal((M, D))
    U = rng.uniform(-1.2, 1.2, (K, M, 2))
    scale = rng.uniform(0.8, 1.3, (nal, M, 1))                            # the candidates: the nominal's error, scaled
    kobs_c = np.stack([(target + scale[i] * (obs_k - target)) for i in range(nal)], 1).reshape(K, N, D)
    kobs_c += 0.05 * rng.standard_normal(kobs_c.shape)
    eobs_c = (target + scale * (end_obs - target)).reshape(N, D)
    act_c = np.tile(U, (1, nal, 1)) * rng.uniform(0.5, 1.1, (K, N, 1))
    qdiag = np.array([0.0 if c not in shown else (1.0 if c < nq else 0.01) for c in range(n)])
    Q, R = np.diag(qdiag), 0.1 * np.eye(2)
    tt = torch.as_tensor
    tgt, qs, Rt = tt(target)[:, slots], tt(qdiag[shown]), tt(R)

    def cost(obs_seq, act):                                                # examples/ilqr_balancing.py, cost()
        err = obs_seq[:, :, slots] - tgt.repeat(obs_seq.shape[1] // M, 1)
        a = act.clamp(-1.0, 1.0)
        return 0.5 * (err * err * qs).sum(dim=(0, 2)) + 0.5 * torch.einsum("kbi,ij,kbj->b", a, Rt, a)
    J = cost(torch.cat([tt(obs_k), tt(end_obs)[None]]), tt(U))
    J_c = cost(torch.cat([tt(kobs_c), tt(eobs_c)[None]]), tt(act_c)).view(nal, M)
    best = J_c.argmin(0)                                                   # step 7, per trajectory
    accept = J_c.gather(0, best[None])[0] < J
    choice_t = torch.where(accept, best, -1).numpy()
    out = t.restate(kobs_c, eobs_c, act_c, target, Q, R, cols, np.float64, nominal=dict(
        cost=J.numpy(), lx=np.zeros((n, K * M)), lu=np.zeros((2, K * M)), p_final=np.zeros((n, M))))
    assert np.array_equal(out["choice"], choice_t) and (choice_t >= 0).any() and (choice_t < 0).any() and len(set(choice_t.tolist())) >= 3
    eps = np.finfo(np.float64).eps
    ops = K * (n * (n - 1) + (n - 1) + 5) + n * (n - 1) + n
    err = np.abs(out["cand_cost"] - J_c.numpy()) / (ops * eps * np.abs(J_c.numpy()))      # (every product of these costs is >= 0)
    print(f"costs: worst |restated - torch| over the bound {err.max():.3f}")
    assert err.max() <= 1.0
    # step 3 of the example for the accepted candidates: lx = Q (x_k - x*), lu = R a_k, p_final = Q (x_K - x*)
    acc = np.nonzero(choice_t >= 0)[0]
    j = choice_t[acc] * M + acc
    lx = torch.zeros(K, len(acc), n, dtype=torch.float64)
    lx[:, :, shown] = qs * (tt(kobs_c)[:, j][:, :, slots] - tgt[acc])
    lu = tt(act_c)[:, j].clamp(-1.0, 1.0) @ Rt
    pf = torch.zeros(len(acc), n, dtype=torch.float64)
    pf[:, shown] = qs * (tt(eobs_c)[j][:, slots] - tgt[acc])
    got_lx = out["nominal"]["lx"].reshape(n, K, M)[:, :, acc].transpose(1, 2, 0)
    got_lu = out["nominal"]["lu"].reshape(2, K, M)[:, :, acc].transpose(1, 2, 0)
    got_pf = out["nominal"]["p_final"][:, acc].T
    # the sums of absolute products, element by element: sum_c |Q[r][c] e[c]| and |R[c][0] a_0| + |R[c][1] a_1|
    e_k = np.zeros((K, len(acc), n))
    e_k[:, :, shown] = kobs_c[:, j][:, :, slots] - target[acc][:, slots]
    e_f = np.zeros((len(acc), n))
    e_f[:, shown] = eobs_c[j][:, slots] - target[acc][:, slots]
    a_k = np.clip(act_c[:, j], -1.0, 1.0)
    for name, got, want, adds, size in (("lx", got_lx, lx.numpy(), n - 1, np.abs(e_k) @ np.abs(Q)), ("lu", got_lu, lu.numpy(), 1, np.abs(a_k) @ np.abs(R)),
                                        ("p_final", got_pf, pf.numpy(), n - 1, np.abs(e_f) @ np.abs(Q))):
        assert got.shape == want.shape == size.shape, name
        over = np.abs(got - want) - adds * eps * size
        print(f"{name}: worst difference {np.abs(got - want).max():.2e}, worst difference minus its bound {over.max():.2e}")
        assert (over <= 0).all(), name


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
    assert callable(HipSim.ilqr_line_search) and callable(HipSim.ilqr_line_search_into)
    s = _bare(torch.float64)
    n, D, K, M, nal, f64 = 6, 4, 3, 4, 2, torch.float64
    N, L = nal * M, K * M
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    kobs, eobs, act, tgt = z(K, N, D), z(N, D), z(K, N, 2), z(M, D)
    Q, R = torch.eye(n, dtype=f64), 0.1 * torch.eye(2, dtype=f64)
    cost, choice = z(M), z(M, dtype=torch.int32)
    nan = float("nan")
    ok = dict(cost=cost, choice=choice)

    def both(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            s.ilqr_line_search_into(*args, **dict(ok, **kw))
        hi = {k: v for k, v in kw.items() if k in ("done", "Q_final")}
        if len(hi) == len(kw):
            with pytest.raises(ValueError, match=match):
                s.ilqr_line_search(*args, **hi)
    for bq in (Q.clone().index_put_((torch.tensor(1), torch.tensor(2)), torch.tensor(0.5, dtype=f64)), nan * Q, torch.eye(5, dtype=f64), "x", None):
        both("^ilqr_line_search: Q", kobs, eobs, act, tgt, bq, R)
    for br in ([[0.1, nan], [nan, 0.1]], [[0.1, 0.01], [0.02, 0.1]], torch.eye(3), 0.1, None):
        both("^ilqr_line_search: R", kobs, eobs, act, tgt, Q, br)
    for bf in (nan * Q, torch.eye(5, dtype=f64), Q.clone().index_put_((torch.tensor(0), torch.tensor(3)), torch.tensor(0.5, dtype=f64)), "x"):
        both("^ilqr_line_search: Q_final", kobs, eobs, act, tgt, Q, R, Q_final=bf)
    # N no multiple of M, no trajectories, too many candidates
    both("^ilqr_line_search: .*no multiple", z(K, N + 1, D), z(N + 1, D), z(K, N + 1, 2), tgt, Q, R)
    both("^ilqr_line_search: .*no multiple", z(K, 2, D), z(2, D), z(K, 2, 2), tgt, Q, R)
    both("^ilqr_line_search: .*no multiple", kobs, eobs, act, z(0, D), Q, R)
    both("^ilqr_line_search: between 1 and 16 candidates", z(K, 17, D), z(17, D), z(K, 17, 2), z(1, D), Q, R)
    # wrong shapes, dtypes, layouts, types
    for args in ((kobs.float(), eobs, act, tgt), (kobs, eobs.float(), act, tgt), (kobs, eobs, act.float(), tgt), (kobs, eobs, act, tgt.float()),
                 (z(K, N, D + 1), eobs, act, tgt), (kobs, z(N, D + 1), act, tgt), (kobs, z(N + M, D), act, tgt), (kobs, eobs, z(K, N, 3), tgt),
                 (kobs, eobs, z(K + 1, N, 2), tgt), (kobs, eobs, act, z(M, D + 1)), (z(N, K, D).permute(1, 0, 2), eobs, act, tgt),
                 (kobs, z(D, N).permute(1, 0), act, tgt), (kobs.numpy(), eobs, act, tgt), (kobs, None, act, tgt), (kobs, eobs, None, tgt),
                 (kobs, eobs, act, None), (z(K * N, D), eobs, act, tgt), (kobs, eobs, act, z(M))):
        both("^ilqr_line_search: ", *args, Q, R)
    both("^ilqr_line_search: done", kobs, eobs, act, tgt, Q, R, done=z(K, N))
    both("^ilqr_line_search: done", kobs, eobs, act, tgt, Q, R, done=z(N, K, dtype=torch.uint8))
    for kw in (dict(cost=None), dict(choice=None), dict(cost=z(M + 1)), dict(cost=cost.float()), dict(choice=z(M)), dict(choice=z(M, dtype=torch.int64)),
               dict(act_nom=z(K, 2, M)), dict(obs_nom=z(K, M, D + 1)), dict(obs_nom=z(K, M, D).float()), dict(end_nom=z(M, D + 1)),
               dict(lx=z(L, n)), dict(lx=z(L, n).permute(1, 0)), dict(lu=z(L, 2)), dict(p_final=z(M, n)), dict(p_final=z(n, L)),
               dict(index=z(L)), dict(index=z(M, dtype=torch.int32)), dict(cand_cost=z(M, nal)), dict(cand_cost=z(nal, M).float()),
               dict(act_nom=[0.0] * 8)):
        with pytest.raises(ValueError, match="^ilqr_line_search: "):
            s.ilqr_line_search_into(kobs, eobs, act, tgt, Q, R, **dict(ok, **kw))
    for bad in ({}, dict(cost=cost), [1, 2], "x"):
        with pytest.raises(ValueError, match="^ilqr_line_search: nominal"):
            s.ilqr_line_search(kobs, eobs, act, tgt, Q, R, nominal=bad)
