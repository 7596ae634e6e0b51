"""libos2r_steer.so (include/os2r_steer.h): the host side -- the header against the one table of gym_os2r_amd/steer.py, the exports
of the library, Os2rSteerRule as gcc lays it out, the other four libraries as they were, every refusal of both entry points
through ctypes without a device, the resources of the sixteen kernels in the built library, the numpy restatement of the steer
rule the GPU tests compare with (`restate_steer`) on crafted inputs that reach every branch of it (`crafted_steer`), and the
argument checks of HipSim.ilqr_steer and of ilqr_backward(mu_dev=...) that need no device.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from gym_os2r_amd import abi

sys.path.insert(0, os.path.join(ROOT, "tests"))
from header_check import _agrees, _header, _is_pointer, _prototypes, checks_before_the_device, the_finite_and_symmetric_tests_make_no_hip_call  # noqa: E402

NAMES = ["os2rt_abi_version", "os2rt_last_error", "os2rt_ilqr_backward_mu", "os2rt_ilqr_steer"]
RULE = ("armijo", "shrink", "grow", "mu_floor", "mu_start", "mu_max", "tol")
DEFAULTS = dict(armijo=0.0, shrink=0.5, grow=10.0, mu_floor=1e-3, mu_start=0.1, mu_max=1e6, tol=0.0)
BRANCH_RULE = dict(DEFAULTS, armijo=1e-4, tol=1e-3)        # the rule of the branch-covering inputs
BRANCH_SHAPE = (5, 10, 7, 70, 3)                           # nq, D, K, M, nalpha: two workgroups with a tail, K no multiple of nalpha
ALPHAS = (1.0, 0.5, 0.25, 0.125) * 4


# ---------------------------------------------------------------------------------------
# the restatement of include/os2r_steer.h, os2rt_ilqr_steer (needs no device)
# ---------------------------------------------------------------------------------------
def restate_steer(c, dtype, rule):
    """c: the dict of `crafted_steer` -> what test_gpu_ilqr_line_search.restate returns, the nominal also holding mu, status and
    iters after the call."""
    import test_gpu_ilqr_line_search as t
    K, N, _ = c["knot_obs"].shape
    M = c["target"].shape[0]
    nalpha = N // M
    r = {k: np.float64(rule[k]).astype(dtype) for k in RULE}                     # rounded once
    al = np.asarray(c["alphas"][:nalpha], np.float64).astype(dtype)
    dv, cost = c["dv"].astype(dtype), c["nominal"]["cost"].astype(dtype)
    mu, status, iters = c["mu"].astype(dtype), c["status"].astype(np.int32), c["iters"].astype(np.int32)
    with np.errstate(all="ignore"):
        # 1. the cost of every candidate
        J = t.restate_crafted(c, dtype, always=True)["cand_cost"]
        # 2.
        d1, d2 = dv[0, 0], dv[0, 1]
        for k in range(1, K):
            d1, d2 = d1 + dv[k, 0], d2 + dv[k, 1]
        # 3.
        ok = np.isfinite(J) & ~(c["done"] != 0).any(0).reshape(nalpha, M) & (J < cost[None]) & (status == 0)[None]
        if r["armijo"] != 0:
            for i in range(nalpha):
                e = (al[i] * d1) + ((al[i] * al[i]) * d2)
                ok[i] &= np.isfinite(e) & (cost - J[i] >= r["armijo"] * (-e))
        # 4. and the nominal of step 5: the line search's own selection and write-back among the acceptable candidates (a done
        # flag on every other one; ACCEPT_ALWAYS, since step 3 has compared the costs already)
        out = t.restate_crafted(dict(c, done=np.tile((~ok).reshape(1, N), (K, 1)).astype(np.uint8)), dtype, always=True)
        choice, nom = out["choice"], out["nominal"]
        assert np.array_equal(out["cand_cost"].view(np.uint8), J.view(np.uint8))
        taken = choice >= 0
        Jb = J[np.maximum(choice, 0), np.arange(M)]
        # 5.
        mu_new = np.where(taken, np.where(mu > r["mu_floor"], r["shrink"] * mu, dtype(0)), mu)
        iters = iters + taken.astype(np.int32)
        converged = taken & (cost - Jb <= r["tol"] * np.abs(cost))
        # 6.
        rejected = ~taken & (status == 0)
        to = np.maximum(r["grow"] * mu, r["mu_start"])                           # (a NaN is caught by `invalid`)
        invalid = ~np.isfinite(mu) | (mu < 0)
        stalled = rejected & (invalid | (to > r["mu_max"]))
        mu_new = np.where(rejected & ~stalled, to, mu_new)
        status = np.where(converged, 1, np.where(stalled, 2, status)).astype(np.int32)
    nom.update(mu=mu_new.astype(dtype), status=status, iters=iters)
    out["branches"] = dict(taken=taken, converged=converged, rejected=rejected, stalled=stalled, invalid=invalid, ok=ok, J=J, d1=d1, d2=d2)
    return out


def crafted_steer(nq, D, K, M, nalpha, dtype, rule=BRANCH_RULE, seed=0):
    """test_gpu_ilqr_line_search.crafted (a nominal cost of 0 where m % 3 == 0, a tie where m % 5 == 1, a done flag in the best
    candidate where m % 7 == 5, ...) with a dv whose predicted change every lower cost passes, mu cycling through 0.4, 5e-4, 0
    and 3, every status 0, and by trajectory (where M reaches it)
      m = 4    a nominal cost just above the best candidate's: accepted and converged
      m = 7    a predicted change of -1e12 per knot: every candidate lowers the cost, Armijo refuses them all
      m = 8    a NaN in dv, m = 10 an infinity: e is not finite
      m = 9    rejected with mu = mu_max: stalled
      m = 12, 15, 18   rejected with mu = -1, NaN, inf: invalid, stalled, mu left as it is
      m = 11, 13       accepted with mu = NaN, -2: mu becomes 0
      m = 16, 17, 21   status 1, 2, 1 on entry: frozen
    The cost of m = 4 is made from the candidates' costs in `dtype`, so the inputs are made per dtype."""
    import test_gpu_ilqr_line_search as t
    c = t.crafted(nq, D, K, M, nalpha, seed)
    rng = np.random.default_rng(seed + 100)
    dv = np.stack([-rng.uniform(0.1, 1.0, (K, M)), rng.uniform(0.0, 0.05, (K, M))], 1)      # [K, 2, M]
    mu = np.array([0.4, 5e-4, 0.0, 3.0])[np.arange(M) % 4]
    status, iters = np.zeros(M, np.int32), (np.arange(M) % 3).astype(np.int32)
    cost = c["nominal"]["cost"].copy()

    def at(m):
        return m < M
    if at(4):
        J = t.restate_crafted(c, dtype, always=True)["cand_cost"].astype(np.float64)[:, 4]
        usable = np.isfinite(J) & ~(c["done"] != 0).any(0).reshape(nalpha, M)[:, 4]
        cost[4] = J[usable].min() * (1.0 + 1e-5)
        dv[:, 0, 4], dv[:, 1, 4] = -1e-6, 0.0
    if at(7):
        dv[:, 0, 7], dv[:, 1, 7] = -1e12, 0.0
    if at(8):
        dv[K // 2, 1, 8] = np.nan
    if at(10):
        dv[0, 0, 10] = -np.inf
    for m, v in ((9, rule["mu_max"]), (12, -1.0), (15, np.nan), (18, np.inf), (11, np.nan), (13, -2.0)):
        if at(m):
            mu[m] = v
    for m, v in ((16, 1), (17, 2), (21, 1)):
        if at(m):
            status[m] = v
    c["nominal"] = dict(c["nominal"], cost=cost)
    return dict(c, dv=dv, mu=mu, status=status, iters=iters, alphas=ALPHAS[:nalpha])


def test_the_restated_rule_on_crafted_inputs_that_reach_every_branch():
    from gym_os2r_amd import steer
    # the restatement's rule members, defaults and status codes are the library's
    assert RULE == tuple(f[0] for f in steer.Os2rSteerRule._fields_) and DEFAULTS == steer.RULE_DEFAULTS
    assert (steer.ACTIVE, steer.CONVERGED, steer.STALLED) == (0, 1, 2)
    nq, D, K, M, nalpha = BRANCH_SHAPE
    for dtype in (np.float64, np.float32):
        c = crafted_steer(nq, D, K, M, nalpha, dtype)
        out = restate_steer(c, dtype, BRANCH_RULE)
        b, nom, choice = out["branches"], out["nominal"], out["choice"]
        mu0, st0, it0 = c["mu"].astype(dtype), c["status"], c["iters"]
        rule = {k: np.float64(v).astype(dtype) for k, v in BRANCH_RULE.items()}
        cost0 = c["nominal"]["cost"].astype(dtype)
        taken = b["taken"]
        # accepted, mu shrunk to a nonzero value / set to 0
        shrunk = taken & (nom["mu"] != 0)
        assert shrunk.any() and np.array_equal(nom["mu"][shrunk], rule["shrink"] * mu0[shrunk]) and (mu0[shrunk] > rule["mu_floor"]).all()
        zeroed = taken & (nom["mu"] == 0) & (mu0 > 0)
        assert zeroed.any() and (mu0[zeroed] <= rule["mu_floor"]).all()
        assert taken[[11, 13]].all() and (nom["mu"][[11, 13]] == 0).all()                       # an invalid mu that accepted
        assert np.array_equal(nom["iters"], it0 + taken) and (nom["cost"][taken] < cost0[taken]).all()
        # converged: m = 4 and nobody else
        assert np.array_equal(np.nonzero(b["converged"])[0], [4]) and nom["status"][4] == 1 and taken[4]
        # lower cost, refused by Armijo; a non-finite e
        with np.errstate(invalid="ignore"):
            lower = (b["J"] < cost0[None]) & np.isfinite(b["J"])
        assert lower[:, 7].any() and not b["ok"][:, 7].any() and np.isfinite(b["d1"][7]) and choice[7] == -1
        for m in (8, 10):
            assert lower[:, m].any() and not b["ok"][:, m].any() and not (np.isfinite(b["d1"][m]) and np.isfinite(b["d2"][m])) and choice[m] == -1
        # ... all three are rejected and raised
        for m in (7, 8, 10):
            assert nom["status"][m] == 0 and nom["mu"][m] == max(rule["grow"] * mu0[m], rule["mu_start"]) > mu0[m]
        raised = b["rejected"] & ~b["stalled"]
        assert (nom["mu"][raised] == np.maximum(rule["grow"] * mu0[raised], rule["mu_start"])).all() and (nom["status"][raised] == 0).all()
        assert (raised & (mu0 == 0)).any() and (raised & (mu0 == 3)).any()                      # from mu_start, and grown
        # stalled: at mu_max, and the invalid ones; mu as it was, bit for bit
        assert b["stalled"][[9, 12, 15, 18]].all() and b["stalled"].sum() == 4 and not b["invalid"][9] and b["invalid"][[12, 15, 18]].all()
        assert (nom["status"][b["stalled"]] == 2).all()
        assert np.array_equal(nom["mu"][b["stalled"]].view(np.uint8), mu0[b["stalled"]].view(np.uint8))
        # frozen on entry: nothing of the trajectory moves (16 would have accepted)
        frozen = st0 != 0
        assert frozen.sum() == 3 and (choice[frozen] == -1).all() and lower[:, 16].any()
        for name in ("mu", "status", "iters", "cost"):
            was = dict(mu=mu0, status=st0, iters=it0, cost=cost0)[name]
            assert np.array_equal(nom[name][frozen].view(np.uint8), was[frozen].view(np.uint8)), name
        assert (out["index"][np.tile(frozen, K)] == -1).all() and np.isfinite(out["cand_cost"][:, 16]).all()
        # a done flag in the best candidate (it sits on the target: J = 0), and a tie
        ended = np.arange(M)[(np.arange(M) % 7 == 5) & taken]
        assert len(ended) and (b["J"][nalpha - 1, ended] == 0).all() and (choice[ended] != nalpha - 1).all()
        tie = np.arange(M)[(np.arange(M) % 5 == 1) & (np.arange(M) % 7 != 3) & (np.arange(M) % 7 != 5) & taken]
        assert len(tie) and (choice[tie] == 0).all() and all((b["J"][:, m] == b["J"][0, m]).all() for m in tie)
        # with armijo = 0 and every status 0 the selection is the line search's own
        import test_gpu_ilqr_line_search as t
        free = dict(c, status=np.zeros(M, np.int32))
        got, want = restate_steer(free, dtype, dict(BRANCH_RULE, armijo=0.0)), t.restate_crafted(free, dtype)
        assert np.array_equal(got["choice"], want["choice"]) and np.array_equal(got["index"], want["index"])
        for name in want["nominal"]:
            assert np.array_equal(got["nominal"][name].view(np.uint8), want["nominal"][name].view(np.uint8)), name
        assert (got["choice"][[7, 8, 10, 16]] >= 0).all()


# ---------------------------------------------------------------------------------------
# header, table, exports, struct
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import control, steer
    protos = _prototypes("os2r_steer.h", "os2rt")
    assert [p[0] for p in protos] == list(steer.ENTRY_POINTS) == NAMES
    lib = steer.load()
    for name, ret, args in protos:
        argtypes = steer.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2rt_last_error" else C.c_int)
    # os2rt_ilqr_backward_mu is os2rc_ilqr_backward with `double mu` replaced by `const void* mu_dev`
    (_, _, theirs), = [p for p in _prototypes("os2r_control.h", "os2rc") if p[0] == "os2rc_ilqr_backward"]
    assert [a if a != "double mu" else "const void* mu_dev" for a in theirs] == protos[2][2] and "double mu" in theirs
    # os2rt_ilqr_steer: the arguments of os2rs_ilqr_line_search without flags, and the new ones
    (_, _, theirs), = [p for p in _prototypes("os2r_search.h", "os2rs") if p[0] == "os2rs_ilqr_line_search"]
    added = ["const void* dv_dev", "const double* alpha_host", "const Os2rSteerRule* rule_host", "void* mu_dev", "int32_t* status_dev",
             "int32_t* iters_dev"]
    assert sorted(protos[3][2]) == sorted([a for a in theirs if a != "uint32_t flags"] + added) and protos[3][2][-1] == "void* stream"
    assert steer.ENTRY_POINTS["os2rt_ilqr_steer"][14] is C.POINTER(steer.Os2rSteerRule) and protos[3][2][14] == added[2]
    header = _header("os2r_steer.h")
    assert re.search(r"#define OS2R_STEER_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert lib.os2rt_abi_version() == steer.ABI_VERSION == 1
    assert steer.Os2rControlLayout is control.Os2rControlLayout and steer.layout is control.layout
    assert (steer.ACTIVE, steer.CONVERGED, steer.STALLED) == tuple(int(re.search(rf"#define OS2RT_{k} (\d)", header).group(1))
                                                                   for k in ("ACTIVE", "CONVERGED", "STALLED")) == (0, 1, 2)
    assert steer.RULE_DEFAULTS == DEFAULTS
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", steer.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(steer.ENTRY_POINTS)


def test_the_rule_struct_is_laid_out_as_gcc_lays_it_out():
    from gym_os2r_amd import steer
    assert tuple(f[0] for f in steer.Os2rSteerRule._fields_) == RULE and all(f[1] is C.c_double for f in steer.Os2rSteerRule._fields_)
    assert shutil.which("gcc")
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "os2r_steer.h"\nint main(void) {\n  printf("%zu", sizeof(Os2rSteerRule));\n' + \
        "".join(f'  printf(" %zu", offsetof(Os2rSteerRule, {f}));\n' for f in RULE) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "rule.c"), os.path.join(tmp, "rule")
        with open(src, "w") as f:
            f.write(prog)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(steer.Os2rSteerRule)] + [getattr(steer.Os2rSteerRule, f).offset for f in RULE] == [56] + [8 * i for i in range(7)]


def test_the_other_libraries_are_as_they_were():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib, control, search, steer
    assert not set(steer.ENTRY_POINTS) & (set(_lib.ENTRY_POINTS) | set(_lib.RECORD_ENTRY_POINTS) | set(control.ENTRY_POINTS) | set(search.ENTRY_POINTS))
    for name in ("os2r.h", "os2r_control.h", "os2r_record.h", "os2r_search.h"):
        assert "os2rt_" not in _header(name) and "steer" not in _header(name), name
    assert list(control.ENTRY_POINTS) == ["os2rc_abi_version", "os2rc_last_error", "os2rc_ilqr_backward"]
    assert list(search.ENTRY_POINTS) == ["os2rs_abi_version", "os2rs_last_error", "os2rs_ilqr_line_search"]
    exports = {_lib.LIB_PATH: set(_lib.ENTRY_POINTS), _lib.RECORD_LIB_PATH: set(_lib.RECORD_ENTRY_POINTS),
               control.LIB_PATH: set(control.ENTRY_POINTS), search.LIB_PATH: set(search.ENTRY_POINTS)}
    for path, table in exports.items():
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == table, path
        kernels = kernel_meta.kernel_meta(path)
        assert kernels and not any("_mu_kernel" in k or "steer" in k for k in kernels), path
    assert len(kernel_meta.kernel_meta(control.LIB_PATH)) == 8 and len(kernel_meta.kernel_meta(search.LIB_PATH)) == 8


def test_kernel_resources():
    """All sixteen kernels ({backward_mu, steer} x {float, double} x nq 2..5) are in the built library and none uses scratch:
    private_segment_fixed_size 0, no VGPR spill and no AGPRs in the code-object metadata.  The steer kernels stay within the 128
    registers at which the 16 waves of their widest workgroup fit four SIMDs; two workgroups of the widest kernel fit a CU's LDS."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import steer
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(steer.LIB_PATH)
    meta = kernel_meta.kernel_meta(steer.LIB_PATH)
    assert len(meta) == 16, sorted(meta)
    widest = 0
    for real in ("float", "double"):
        for nq in (2, 3, 4, 5):
            for family in ("ilqr_backward_mu_kernel", "ilqr_steer_kernel"):
                (name,) = [k for k in meta if f"{family}<{real}, {nq}>" in k]
                m = meta[name]
                assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
                if family == "ilqr_steer_kernel":
                    assert m["vgpr_count"] <= 128, (name, m)
                widest = max(widest, m["group_segment_fixed_size"])
    assert 0 < 2 * widest <= 160 * 1024, widest


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def _matrices(n):
    def Qm(i=None, j=None, v=0.0):
        m = np.eye(n)
        if i is not None:
            m[i, j] = v
        return (C.c_double * (n * n))(*m.reshape(-1))

    def Rm(*v):
        return (C.c_double * 4)(*(v or (0.1, 0.0, 0.0, 0.1)))
    return Qm, Rm


def _lay(chain, **kw):
    from gym_os2r_amd import control
    lay = control.layout(abi.F64, chain, 0, [0, 1, 3, -1])
    for k, v in kw.items():
        if k == "slot0":
            lay.slot_col[0] = v
        else:
            setattr(lay, k, v)
    return C.byref(lay)


def _refused(lib, call, cases, prefix, count):
    seen = set()
    for kw, msg in cases:
        rc = call(**kw)
        err = lib.os2rt_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(prefix), (kw.keys(), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases}) == count, (len(seen), len({m for _, m in cases}))      # each cause has a text of its own


def test_refusals_of_backward_mu_come_through_ctypes_without_a_device():
    from gym_os2r_amd import steer
    lib = steer.load()
    nq, n = 3, 6
    buf = (C.c_double * 4096)()
    d = C.cast(buf, C.c_void_p)
    nan, inf = float("nan"), float("inf")
    Qm, Rm = _matrices(n)
    Lay = lambda **kw: _lay(nq, **kw)
    Al = lambda *v: (C.c_double * len(v))(*v)
    good = dict(lay=Lay(), K=2, M=4, a=d, b=d, lx=None, lu=None, q=Qm(), r=Rm(), mu=d, pf=None, vf=None, gain=d, ff=None, po=None, vo=None,
                flag=None, dv=None, act=None, obs=None, al=None, nal=0, w=None)
    name = "os2rt_ilqr_backward_mu"
    assert len(good) + 1 == len(steer.ENTRY_POINTS[name])

    def call(**kw):
        a = dict(good, **kw)
        return getattr(lib, name)(*[a[k] for k in good], None)
    assert getattr(lib, name)(*[None if _is_pointer(t) else 0 for t in steer.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rt_last_error() == b"os2rt_ilqr_backward_mu: null layout"
    wts = dict(w=d, act=d, obs=d, al=Al(1.0, 0.5), nal=2)
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(nq=1)), b"nq must be 2..5"),
             (dict(lay=Lay(nq=6)), b"nq must be 2..5"), (dict(K=0), b"nknots must be >= 1"), (dict(M=0), b"ntraj must be >= 1"),
             (dict(M=2 ** 62), b"ntraj exceeds what one launch covers"), (dict(a=None), b"null a_dev"), (dict(b=None), b"null b_dev"),
             (dict(q=None), b"null q_host"), (dict(r=None), b"null r_host"), (dict(mu=None), b"null mu_dev"),
             (dict(q=Qm(1, 2, nan)), b"Q must be finite"), (dict(r=Rm(inf, 0.0, 0.0, 0.1)), b"R must be finite"),
             (dict(q=Qm(1, 2, 0.5)), b"Q must be exactly symmetric"), (dict(r=Rm(0.1, 0.01, 0.02, 0.1)), b"R must be exactly symmetric"),
             (dict(gain=None), b"all outputs are null"), (dict(wts, act=None), b"weights need"),
             (dict(wts, obs=None), b"weights need"), (dict(wts, al=None), b"weights need"),
             (dict(wts, nal=0), b"nalpha must be 1..16"), (dict(wts, nal=17), b"nalpha must be 1..16"),
             (dict(wts, al=Al(1.0, nan)), b"alpha must be finite"), (dict(wts, lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"),
             (dict(wts, lay=Lay(obs_dim=13)), b"obs_dim must be 1..12"), (dict(wts, lay=Lay(slot0=n)), b"slot_col entries must be -1..n-1")]
    _refused(lib, call, cases, b"os2rt_ilqr_backward_mu: ", 21)
    assert not any(buf)                                             # a refused call wrote nothing
    # those of os2rc_ilqr_backward without the two about mu, and "null mu_dev"
    texts = checks_before_the_device("os2r_steer_capi.hip", name, ("layout_refusal", "slots_refusal"))
    theirs = checks_before_the_device("os2r_control_capi.hip", "os2rc_ilqr_backward", ("layout_refusal", "slots_refusal"))
    assert sorted(texts) == sorted([x for x in theirs if not x.startswith("mu must")] + ["null mu_dev"]) and len(texts) + 1 == len(theirs) == 22
    the_finite_and_symmetric_tests_make_no_hip_call()


def test_refusals_of_steer_come_through_ctypes_without_a_device():
    from gym_os2r_amd import steer
    lib = steer.load()
    nq, n = 3, 6
    buf = (C.c_double * 4096)()
    d = C.cast(buf, C.c_void_p)
    nan, inf = float("nan"), float("inf")
    Qm, Rm = _matrices(n)
    Lay = lambda **kw: _lay(nq, **kw)
    Al = lambda *v: (C.c_double * len(v))(*v)
    Rule = lambda **kw: C.byref(steer.Os2rSteerRule(**dict(DEFAULTS, **kw)))
    good = dict(lay=Lay(), K=2, M=4, nal=2, kobs=d, eobs=d, act=d, done=None, tgt=d, q=Qm(), r=Rm(), qf=None, dv=d, al=Al(1.0, 0.5),
                rule=Rule(), cost=d, an=None, on=None, en=None, lx=None, lu=None, pf=None, mu=d, status=d, iters=None, choice=d, index=None,
                cc=None)
    name = "os2rt_ilqr_steer"
    assert len(good) + 1 == len(steer.ENTRY_POINTS[name])

    def call(**kw):
        a = dict(good, **kw)
        return getattr(lib, name)(*[a[k] for k in good], None)
    assert getattr(lib, name)(*[None if _is_pointer(t) else 0 for t in steer.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2rt_last_error() == b"os2rt_ilqr_steer: null layout"
    cases = [(dict(lay=None), b"null layout"), (dict(lay=Lay(dtype=2)), b"dtype must be"), (dict(lay=Lay(nq=1)), b"nq must be 2..5"),
             (dict(lay=Lay(obs_dim=0)), b"obs_dim must be 1..12"), (dict(lay=Lay(slot0=-2)), b"slot_col entries must be -1..n-1"),
             (dict(K=0), b"nknots must be >= 1"), (dict(M=0), b"ntraj must be >= 1"), (dict(nal=0), b"nalpha must be 1..16"),
             (dict(nal=17), b"nalpha must be 1..16"), (dict(K=1024, M=2 ** 17, nal=16, al=Al(*[1.0] * 16)), b"exceeds 2^31 - 1"),
             (dict(M=2 ** 62), b"exceeds 2^31 - 1"),
             (dict(kobs=None), b"null knot_obs_dev"), (dict(eobs=None), b"null end_obs_dev"), (dict(act=None), b"null act_dev"),
             (dict(tgt=None), b"null target_dev"), (dict(q=None), b"null q_host"), (dict(r=None), b"null r_host"),
             (dict(dv=None), b"null dv_dev"), (dict(al=None), b"null alpha_host"), (dict(rule=None), b"null rule_host"),
             (dict(cost=None), b"null cost_dev"), (dict(mu=None), b"null mu_dev"), (dict(status=None), b"null status_dev"),
             (dict(choice=None), b"null choice_dev"),
             (dict(q=Qm(1, 2, nan)), b"Q must be finite"), (dict(r=Rm(0.1, nan, nan, 0.1)), b"R must be finite"),
             (dict(qf=Qm(3, 3, nan)), b"Qf must be finite"), (dict(q=Qm(1, 2, 0.5)), b"Q must be exactly symmetric"),
             (dict(r=Rm(0.1, 0.01, 0.02, 0.1)), b"R must be exactly symmetric"), (dict(qf=Qm(4, 0, 1e-300)), b"Qf must be exactly symmetric"),
             (dict(al=Al(1.0, inf)), b"alpha must be finite"), (dict(al=Al(nan, 0.5)), b"alpha must be finite"),
             (dict(rule=Rule(tol=nan)), b"every member of the rule"), (dict(rule=Rule(armijo=inf)), b"every member of the rule"),
             (dict(rule=Rule(mu_max=inf)), b"every member of the rule"),
             (dict(rule=Rule(armijo=-1e-9)), b"rule armijo must be >= 0"), (dict(rule=Rule(shrink=-0.1)), b"rule shrink must be 0..1"),
             (dict(rule=Rule(shrink=1.5)), b"rule shrink must be 0..1"), (dict(rule=Rule(grow=0.99)), b"rule grow must be >= 1"),
             (dict(rule=Rule(mu_floor=-1.0)), b"rule mu_floor must be >= 0"), (dict(rule=Rule(mu_start=0.0)), b"rule mu_start must be > 0"),
             (dict(rule=Rule(mu_start=-0.1)), b"rule mu_start must be > 0"), (dict(rule=Rule(mu_max=0.05)), b"rule mu_max must be >= mu_start"),
             (dict(rule=Rule(tol=-1.0)), b"rule tol must be >= 0")]
    _refused(lib, call, cases, b"os2rt_ilqr_steer: ", 37)
    assert not any(buf)                                             # a refused call wrote nothing
    # the edges of the rule are taken: the next refusal is about something else
    edge = Rule(armijo=0.0, shrink=0.0, grow=1.0, mu_floor=0.0, mu_start=1e-300, mu_max=1e-300, tol=0.0)
    assert call(rule=edge, choice=None) == abi.ERR_INVALID and lib.os2rt_last_error().endswith(b"null choice_dev")
    assert call(rule=Rule(shrink=1.0), choice=None) == abi.ERR_INVALID and lib.os2rt_last_error().endswith(b"null choice_dev")
    # those of os2rs_ilqr_line_search without the one about flags, and the new ones
    texts = checks_before_the_device("os2r_steer_capi.hip", name, ("layout_refusal", "slots_refusal"))
    theirs = checks_before_the_device("os2r_search_capi.hip", "os2rs_ilqr_line_search", ("layout_refusal", "slots_refusal"))
    assert set(theirs) - set(texts) == {"unknown flag bits"} and len(texts) == 37 and len(set(texts) - set(theirs)) == 14
    # the error text belongs to the entry point that failed last
    assert lib.os2rt_ilqr_backward_mu(*[None if _is_pointer(t) else 0 for t in steer.ENTRY_POINTS["os2rt_ilqr_backward_mu"]]) == abi.ERR_INVALID
    assert lib.os2rt_last_error() == b"os2rt_ilqr_backward_mu: null layout"


# ---------------------------------------------------------------------------------------
# the Python layer, without a device
# ---------------------------------------------------------------------------------------
def _bare(dtype, n=8, nq=3, D=4):
    """A HipSim that never met a device: enough of it for the checks that run before the library is called."""
    import torch
    from gym_os2r_amd.sim import HipSim
    s = HipSim.__new__(HipSim)
    s.N, s.nq, s.D, s.dtype, s.device = n, nq, D, dtype, torch.device("cpu")
    s._h = None
    s._lib = None      # (and it has no cfg: filling the layout would raise AttributeError, not ValueError)
    return s


def test_the_rule_of_the_python_layer():
    from gym_os2r_amd import steer
    r = steer.rule()
    assert {k: getattr(r, k) for k in RULE} == DEFAULTS
    r = steer.rule(dict(armijo=1e-4, tol=0.5), tol=1e-3)
    assert (r.armijo, r.tol, r.shrink) == (1e-4, 1e-3, 0.5)
    nan = float("nan")
    for bad in (dict(armijo=-1.0), dict(shrink=1.1), dict(shrink=-0.1), dict(grow=0.5), dict(mu_floor=-1.0), dict(mu_start=0.0),
                dict(mu_max=0.01), dict(tol=-1.0), dict(tol=nan), dict(mu_max=float("inf")), dict(nothing=1.0), dict(armijo="x")):
        with pytest.raises(ValueError, match="^ilqr_steer: "):
            steer.rule(bad)
        with pytest.raises(ValueError, match="^ilqr_steer: "):
            steer.rule(**bad)


def test_python_argument_errors_need_no_device():
    import torch
    from gym_os2r_amd.sim import HipSim
    assert callable(HipSim.ilqr_steer) and callable(HipSim.ilqr_steer_into)
    s = _bare(torch.float64)
    n, D, K, M, nal, f64 = 6, 4, 3, 4, 2, torch.float64
    N, L = nal * M, K * M
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    kobs, eobs, act, tgt, dv, al = z(K, N, D), z(N, D), z(K, N, 2), z(M, D), z(K, 2, M), (1.0, 0.5)
    Q, R = torch.eye(n, dtype=f64), 0.1 * torch.eye(2, dtype=f64)
    ok = dict(cost=z(M), mu=z(M), status=i32(M), choice=i32(M))
    nan = float("nan")

    def into(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            s.ilqr_steer_into(*args, **dict(ok, **kw))
    bad_q = Q.clone().index_put_((torch.tensor(1), torch.tensor(2)), torch.tensor(0.5, dtype=f64))
    for bq in (bad_q, nan * Q, torch.eye(5, dtype=f64), "x", None):
        into("^ilqr_steer: Q", kobs, eobs, act, tgt, bq, R, dv, al)
    for br in ([[0.1, nan], [nan, 0.1]], [[0.1, 0.01], [0.02, 0.1]], torch.eye(3), None):
        into("^ilqr_steer: R", kobs, eobs, act, tgt, Q, br, dv, al)
    into("^ilqr_steer: Q_final", kobs, eobs, act, tgt, Q, R, dv, al, Q_final=bad_q)
    into("^ilqr_steer: .*no multiple", z(K, N + 1, D), z(N + 1, D), z(K, N + 1, 2), tgt, Q, R, dv, al)
    into("^ilqr_steer: between 1 and 16 candidates", z(K, 17, D), z(17, D), z(K, 17, 2), z(1, D), Q, R, z(K, 2, 1), (1.0,) * 17)
    for bad_al in ((1.0,), (1.0, 0.5, 0.25), (1.0, nan), "xy", None, 1.0):
        into("^ilqr_steer: ", kobs, eobs, act, tgt, Q, R, dv, bad_al)
    for args in ((kobs.float(), eobs, act, tgt, Q, R, dv), (kobs, z(N, D + 1), act, tgt, Q, R, dv), (kobs, eobs, z(K, N, 3), tgt, Q, R, dv),
                 (kobs, eobs, act, z(M, D + 1), Q, R, dv), (kobs, None, act, tgt, Q, R, dv), (kobs, eobs, None, tgt, Q, R, dv),
                 (kobs, eobs, act, tgt, Q, R, None), (kobs, eobs, act, tgt, Q, R, z(K, M, 2)), (kobs, eobs, act, tgt, Q, R, dv.float()),
                 (kobs, eobs, act, tgt, Q, R, z(M, 2, K).permute(2, 1, 0)), (kobs.numpy(), eobs, act, tgt, Q, R, dv)):
        into("^ilqr_steer: ", *args, al)
    for kw in (dict(cost=None), dict(mu=None), dict(status=None), dict(choice=None), dict(mu=z(M + 1)), dict(mu=z(M).float()),
               dict(status=z(M)), dict(status=torch.zeros(M, dtype=torch.int64)), dict(iters=z(M)), dict(iters=i32(M + 1)), dict(choice=z(M)),
               dict(done=z(K, N)), dict(lx=z(L, n)), dict(index=z(L)), dict(cand_cost=z(M, nal)), dict(act_nom=z(K, 2, M)),
               dict(rule=dict(grow=0.5)), dict(armijo=-1.0), dict(tol=nan), dict(rule=dict(unknown=1.0))):
        into("^ilqr_steer: ", kobs, eobs, act, tgt, Q, R, dv, al, **kw)
    with pytest.raises(ValueError, match="^ilqr_steer: unknown rule members"):
        s.ilqr_steer_into(kobs, eobs, act, tgt, Q, R, dv, al, **dict(ok, always=True))        # there is no ACCEPT_ALWAYS here
    # ilqr_steer: the nominal, and dv in the shape ilqr_backward returns it
    nominal = dict(cost=z(M), actions=z(K, M, 2), obs=z(K, M, D), end_obs=z(M, D), lx=z(n, L), lu=z(2, L), p_final=z(n, M))
    for bad in (None, {}, dict(cost=z(M)), [1, 2]):
        with pytest.raises(ValueError, match="^ilqr_steer: nominal"):
            s.ilqr_steer(kobs, eobs, act, tgt, Q, R, z(K, M, 2), al, nominal=bad)
    for bad_dv in (dv, z(K, M, 2).float(), None, z(K, M + 1, 2)):
        with pytest.raises(ValueError, match="^ilqr_steer: dv"):
            s.ilqr_steer(kobs, eobs, act, tgt, Q, R, bad_dv, al, nominal=dict(nominal))
    with pytest.raises(ValueError, match="^ilqr_steer: .*rule"):
        s.ilqr_steer(kobs, eobs, act, tgt, Q, R, z(K, M, 2), al, nominal=dict(nominal), shrink=2.0)
    with pytest.raises(ValueError, match="^ilqr_steer: mu"):
        s.ilqr_steer(kobs, eobs, act, tgt, Q, R, z(K, M, 2), al, nominal=dict(nominal, mu=z(M).float()))
    # ilqr_backward: mu_dev together with a nonzero mu, and a mu_dev that is not what the kernel assumes
    A, B = z(L, n, n), z(L, n, 2)
    a, b = A.permute(1, 2, 0).contiguous(), B.permute(1, 2, 0).contiguous()
    with pytest.raises(ValueError, match="^ilqr_backward: mu_dev and a nonzero mu"):
        s.ilqr_backward(A, B, Q, R, knots=K, mu=0.5, mu_dev=z(M))
    with pytest.raises(ValueError, match="^ilqr_backward: mu_dev and a nonzero mu"):
        s.ilqr_backward_into(a, b, Q, R, knots=K, mu=0.5, mu_dev=z(M), gains_out=z(K, 2, n, M))
    for bad in (z(M + 1), z(M).float(), z(2 * M)[::2], [0.0] * M, z(M, 1)):
        with pytest.raises(ValueError, match="^ilqr_backward: mu_dev"):
            s.ilqr_backward(A, B, Q, R, knots=K, mu_dev=bad)
        with pytest.raises(ValueError, match="^ilqr_backward: mu_dev"):
            s.ilqr_backward_into(a, b, Q, R, knots=K, mu_dev=bad, gains_out=z(K, 2, n, M))
