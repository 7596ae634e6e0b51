"""libos2r_sysid.so (include/os2r_sysid.h) without a device: the header against the table of gym_os2r_amd.sysid and the library's
exports; the kernels' resources; every refusal of os2ri_perturb and os2ri_update through ctypes, each with a text of its own and
nothing written; the numpy restatement of tests/sysid_ref.py against an independent statement (np.einsum, np.linalg.solve); the
whole identification loop, with the CPU oracle as the simulator and the restatement as the update, on two problems; crafted single
calls that reach every branch of the update; and the argument checks of the HipSim methods."""
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sysid_ref as R  # noqa: E402
from header_check import HIP_CALL, _agrees, _csrc, _function, _header, _is_pointer, _prototypes  # noqa: E402

NAMES = ["os2ri_abi_version", "os2ri_last_error", "os2ri_perturb", "os2ri_update"]
KERNELS = ("sysid_perturb_kernel", "sysid_segment_kernel", "sysid_sum_kernel", "sysid_sum_few_kernel", "sysid_step_kernel")
# The restatement against the plain statement, max |difference| / max |entry| over the shapes of PLAIN_SHAPES, as measured: in
# float64 against np.einsum / np.linalg.solve (the order of the sums differs, nothing else), and the float32 restatement against
# the float64 one fed the same float32 inputs.  The bound is eight times the measured value, the project's custom.
MEASURED = {np.float64: dict(cost=2.956e-15, hess=6.403e-16, grad=1.022e-15, delta=1.177e-15),
            np.float32: dict(cost=5.717e-08, hess=6.719e-06, grad=9.388e-07, delta=1.041e-06)}
MARGIN = 8
PLAIN_SHAPES = ((1, 200, 5, 5, 10), (1, 64, 3, 21, 10), (3, 70, 4, 3, 8))          # T, Q, K, P, D


def _far(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


# ---------------------------------------------------------------------------------------
# header, table, exports, resources
# ---------------------------------------------------------------------------------------
def test_the_table_is_the_header_and_the_library_exports_it():
    from gym_os2r_amd import _lib, control, sysid
    protos = _prototypes("os2r_sysid.h", "os2ri")
    assert [p[0] for p in protos] == list(sysid.ENTRY_POINTS) == NAMES
    lib = sysid.load()
    for name, ret, args in protos:
        argtypes = sysid.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2ri_last_error" else C.c_int)
    perturb, update = protos[2][2], protos[3][2]
    assert perturb[:8] == ["const Os2rControlLayout* layout", "int32_t nparams", "int64_t nsets", "int64_t nsegments", "const int32_t* sel_host",
                           "const double* h_host", "const double* lo_host", "const double* hi_host"]
    assert len(perturb) == 12 and perturb[-1] == "void* stream" and perturb[-2] == "void* params_dev"
    assert update[:9] == ["const Os2rControlLayout* layout", "int32_t nparams", "int64_t nsets", "int64_t nsegments", "int32_t nsteps",
                          "const double* h_host", "const double* lo_host", "const double* hi_host", "const Os2riConstants* constants"]
    assert len(update) == 37 and update[-1] == "void* stream" and update[-3:-1] == ["void* sums_dev", "int32_t* counts_dev"]
    assert sysid.ENTRY_POINTS["os2ri_update"][8] is C.POINTER(sysid.Os2riConstants)
    header = _header("os2r_sysid.h")
    assert re.search(r"#define OS2R_SYSID_ABI_VERSION 1\b", header) and '#include "os2r_control.h"' in header
    assert len(re.findall(r"#include", header)) == 1
    assert lib.os2ri_abi_version() == sysid.ABI_VERSION == 1
    assert sysid.MAX_PARAMS == int(re.search(r"#define OS2RI_MAX_PARAMS (\d+)", header).group(1)) == 4 * 5 + 1
    assert sysid.CHUNKS == int(re.search(r"#define OS2RI_CHUNKS (\d+)", header).group(1)) == R.CHUNKS == 64
    assert sysid.MAX_SETS == int(re.search(r"#define OS2RI_MAX_SETS (\d+)", header).group(1)) == 2 ** 26 - 1     # 64 threads a set, a grid below 2^32
    # the Makefile: the library is in the default target once, under a name of its own, and `clean` removes it
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "Makefile")) as f:
        make = f.read()
    assert "\nSYSID := ../libos2r_sysid.so\n" in make and "\nCMA := ../libos2r_cma.so\n" in make
    (default,) = re.findall(r"^all: (.*)$", make, re.M)
    assert default.split().count("$(SYSID)") == 1 and "libos2r_sysid" not in default
    (clean,) = re.findall(r"^clean:\n\t(rm -rf .*)$", make, re.M)
    assert clean.split().count("../libos2r_sysid.so") == 1 and clean.split().count("../libos2r_cma.so") == 1
    body = re.sub(r"/\*.*?\*/", " ", re.search(r"typedef struct Os2riConstants \{(.*?)\} Os2riConstants;", header, re.S).group(1), flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("double", "").split(",")]
    assert fields == list(sysid.CONSTANT_NAMES) == list(R.CONSTANT_NAMES) == [n for n, _ in sysid.Os2riConstants._fields_]
    assert C.sizeof(sysid.Os2riConstants) == 8 * 7 and sysid.STATE == R.STATE
    k = sysid.constants()
    assert (k.shrink, k.grow, k.lam_min, k.lam_max) == (0.5, 10.0, 1e-9, 1e6) and k.diag_floor > 0 and k.tol == 0 and k.cost_floor == 0
    assert {n: getattr(k, n) for n in sysid.CONSTANT_NAMES} == R.DEFAULTS
    assert sysid.Os2rControlLayout is control.Os2rControlLayout and sysid.layout is control.layout
    assert not set(sysid.ENTRY_POINTS) & (set(_lib.ENTRY_POINTS) | set(_lib.RECORD_ENTRY_POINTS)) and len(_lib.ENTRY_POINTS) == 35
    assert shutil.which("nm")
    out = subprocess.run(["nm", "-D", "--defined-only", sysid.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == set(NAMES)
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "libos2r_sysid.map")) as f:
        assert re.search(r"global:\s*os2ri_\*;\s*local:\s*\*;", f.read())
    flat = " ".join(header.replace("\n *", " ").split())
    assert "adjacent-pair tree" in flat and "in ascending order onto 0" in flat and "NOT contracted" in flat
    assert "A rejected iteration has therefore spent its 2 P perturbed lanes" in flat
    for line in ("the periodic wrap of an angle residual", "bounds, steps or constants per set", "forward (one-sided) differences with P + 1 lanes",
                 "parameters outside the five fields", "a covariance / Cramer-Rao output", "robust losses",
                 "an active-set treatment of the bounds instead of the clamp", "segments of unequal length", "analytic parameter derivatives",
                 "identifying across a reset"):
        assert line in flat, line
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "os2r_sysid.h":
            assert "os2ri_" not in _header(name).lower() and "os2r_sysid" not in _header(name).lower(), name
    # the sums over the segments of a set are the included body of os2r_pg.hpp, not a copy
    src = _csrc("os2r_sysid.hpp")
    assert '#include "os2r_pg.hpp"' in src and "pg_wave_sum<T>(" in src and "pg_few_sum<T>(" in src and "__shfl_xor" not in src
    # the packed layout: the rows of a field are what set_params takes
    packed = np.arange(21 * 6, dtype=np.float64).reshape(21, 6)
    fields = {f: sysid.field_view(packed, 5, f) for f in sysid.FIELDS}
    assert [v.shape for v in fields.values()] == [(5, 6)] * 4 + [(1, 6)] and all(np.shares_memory(v, packed) and v.flags.c_contiguous for v in fields.values())
    assert np.array_equal(sysid.pack(fields, 5), packed) and sysid.rows(5) == 21 and sysid.row(5, abi.PARAM_GRAVITY) == 20
    assert sysid.row(3, abi.PARAM_MU, 2) == 11
    with pytest.raises(ValueError):
        sysid.row(3, abi.PARAM_GRAVITY, 1)


def test_kernel_resources():
    """Exactly ten kernels, the five of os2r_sysid.hpp in float and double, are in the built library and none uses scratch:
    private_segment_fixed_size 0, no VGPR or SGPR spill and no AGPRs in the code-object metadata.  The register counts are printed
    (and recorded in DESIGN.md section 4).  The segment kernel is a workgroup of up to eleven waves, three a SIMD, which 168 VGPRs
    allow; its LDS is the tile of differences (21 x 3 x 64), two rows of twelve slots and one of flags."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import sysid
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(sysid.LIB_PATH)
    meta = kernel_meta.kernel_meta(sysid.LIB_PATH)
    assert len(meta) == 10, sorted(meta)
    for kernel in KERNELS:
        for real, size in (("float", 4), ("double", 8)):
            (name,) = [k for k in meta if f"{kernel}<{real}>" in k]
            m = meta[name]
            print(f"{kernel}<{real}>: {m['vgpr_count']} VGPRs, {m['sgpr_count']} SGPRs, {m['group_segment_fixed_size']} bytes of LDS")
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["agpr_count"] == 0, (name, m)
            assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 168, (name, m)
            lds = {"sysid_segment_kernel": (21 * 3 * 64 + 2 * 12 * 64) * size + 4 * (12 * 64 + 64),
                   "sysid_step_kernel": (253 + 441 + 21) * size}.get(kernel, 0)
            assert lds <= m["group_segment_fixed_size"] <= lds + 64, (name, m, lds)


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def _lay(dtype=abi.F64, **kw):
    from gym_os2r_amd import control
    lay = control.layout(dtype, 3, 0, [0, 1, 3, -1])
    for k, v in kw.items():
        setattr(lay, k, v)
    return C.byref(lay)


def _dbl(*v):
    return (C.c_double * len(v))(*v)


def _refused(lib, fn, prefix, good, cases, buf):
    seen = set()
    for kw, msg in cases:
        a = dict(good, **kw)
        rc = fn(*[a[k] for k in good], None)
        err = lib.os2ri_last_error()
        assert rc == abi.ERR_INVALID and msg in err and err.startswith(prefix), (list(kw), msg, rc, err)
        seen.add(err)
    assert len(seen) == len({m for _, m in cases})                        # each cause has a text of its own
    assert not any(buf)                                                   # a refused call wrote nothing
    return seen


def _source_checks(unit_function, helpers):
    """The source: no HIP call and every refusal of an argument before check_device."""
    body = _function(_csrc("os2r_sysid_capi.hip"), "int " + unit_function)
    first_hip = body.index("check_device(")
    assert not re.search(HIP_CALL, body[:first_hip]) and body.index("DeviceGuard") > first_hip and body.index("auto launch") > first_hip
    fails = [m.start() for m in re.finditer(r"fail\(OS2R_ERR_INVALID", body)]
    assert fails and all(i < first_hip for i in fails)
    for helper in helpers:
        text = _function(_csrc("os2r_sysid_capi.hip"), helper if helper.startswith("const") else r"[a-z_:* ()]+ " + helper)
        assert not re.search(HIP_CALL + r"|check_device|DeviceGuard|launch", text), helper


SHARED_CASES = [
    (dict(lay=None), b"null layout"), (dict(lay="dtype"), b"dtype must be"), (dict(lay="nq"), b"nq must be 2..5"),
    (dict(P=0), b"nparams must be 1..21"), (dict(P=22), b"nparams must be 1..21"), (dict(T=0), b"nsets must be >= 1"),
    (dict(T=2 ** 26, M=2 ** 26), b"nsets must be < 2^26"), (dict(T=2 ** 40, M=2 ** 40), b"nsets must be < 2^26"),
    (dict(M=0), b"nsegments must be >= 1"), (dict(M=-4), b"nsegments must be >= 1"), (dict(M=5), b"nsegments must be a multiple of nsets"),
    (dict(M=2 ** 31, T=1), b"(2 nparams + 1) * nsegments exceeds 2^31 - 1"), (dict(M=2 ** 62, T=2), b"(2 nparams + 1) * nsegments exceeds 2^31 - 1"),
    (dict(h=None), b"null h_host"), (dict(lo=None), b"null lo_host"), (dict(hi=None), b"null hi_host"),
    (dict(h=_dbl(0.1, 0.0, 0.1)), b"h_host entries must be finite and > 0"), (dict(h=_dbl(0.1, -1.0, 0.1)), b"h_host entries must be finite and > 0"),
    (dict(h=_dbl(float("nan"), 1, 1)), b"h_host entries must be finite and > 0"), (dict(h=_dbl(1, 1, float("inf"))), b"h_host entries must be finite and > 0"),
    (dict(lo=_dbl(0, float("nan"), 0)), b"must not be NaN"), (dict(hi=_dbl(float("nan"), 1, 1)), b"must not be NaN"),
    (dict(lo=_dbl(0, 2, 0)), b"lo_host must be <= hi_host"), (dict(hi=_dbl(1, 1, float("-inf"))), b"lo_host must be <= hi_host"),
]


def _shared(cases):
    out = []
    for kw, msg in cases:
        if kw.get("lay") == "dtype":
            kw = dict(lay=_lay(dtype=2))
        elif kw.get("lay") == "nq":
            kw = dict(lay=_lay(nq=6))
        out.append((kw, msg))
    return out


def test_perturb_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import sysid
    lib = sysid.load()
    P, T, M, F = 3, 2, 4, 13
    N = (2 * P + 1) * M
    buf = (C.c_double * 4096)()
    base = C.addressof(buf)
    at = lambda i: C.c_void_p(base + 8 * i)
    where = dict(theta=0, base=64, params=256)
    sel = (C.c_int32 * 6)(1, 1, 1, 2, 4, 0)
    good = dict(lay=_lay(), P=P, T=T, M=M, sel=sel, h=_dbl(0.1, 0.1, 0.1), lo=_dbl(0, 0, -11), hi=_dbl(1, 1, float("inf")),
                **{k: at(v) for k, v in where.items()})
    name = "os2ri_perturb"
    assert len(good) + 1 == len(sysid.ENTRY_POINTS[name])
    assert lib.os2ri_perturb(*[None if _is_pointer(t) else 0 for t in sysid.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2ri_last_error() == b"os2ri_perturb: null layout"
    pairs = lambda *v: (C.c_int32 * 6)(*v)
    cases = _shared(SHARED_CASES) + [
        (dict(lay=_lay(abi.F32), h=_dbl(0.1, 1e-60, 0.1)), b"h_host entries must be finite and > 0"),
        (dict(sel=None), b"null sel_host"), (dict(sel=pairs(5, 0, 1, 2, 4, 0)), b"sel_host fields must be 0..4"),
        (dict(sel=pairs(-1, 0, 1, 2, 4, 0)), b"sel_host fields must be 0..4"), (dict(sel=pairs(1, 3, 1, 2, 4, 0)), b"sel_host entries must be 0..nq-1"),
        (dict(sel=pairs(1, 1, 1, 2, 4, 1)), b"sel_host entries must be 0..nq-1"), (dict(sel=pairs(1, 1, 4, 0, 1, 1)), b"sel_host names a parameter twice"),
        (dict(theta=None), b"null theta_dev"), (dict(base=None), b"null base_dev"), (dict(params=None), b"null params_dev"),
        (dict(M=(2 ** 32 - 1) // (F * 7) + 2), b"(4 nq + 1) * (2 nparams + 1) * nsegments exceeds 2^32 - 1"),
        (dict(M=2 ** 31 // 7 - 1 - (2 ** 31 // 7 - 1) % 2), b"(4 nq + 1) * (2 nparams + 1) * nsegments exceeds 2^32 - 1"),
        (dict(params=at(where["theta"] + T * P - 1)), b"params_dev overlaps theta_dev"), (dict(params=at(where["base"] + F * M - 1)), b"params_dev overlaps base_dev")]
    seen = _refused(lib, lib.os2ri_perturb, b"os2ri_perturb: ", good, cases, buf)
    assert len(seen) == 25
    edges = [dict(P=1, sel=(C.c_int32 * 2)(4, 0)), dict(lo=_dbl(float("-inf"), 0, 0), hi=_dbl(float("inf"), 0, 0)), dict(h=_dbl(5e-324, 1e300, 1)),
             dict(M=(2 ** 32 - 1) // (F * 7), params=C.c_void_p(2 ** 44), base=C.c_void_p(2 ** 45)), dict(params=at(where["base"] + F * M)),
             dict(P=1, sel=(C.c_int32 * 2)(4, 0), h=_dbl(0.1), lo=_dbl(0.0), hi=_dbl(1.0), T=2 ** 26 - 1, M=2 ** 26 - 1, theta=C.c_void_p(2 ** 46),
                  params=C.c_void_p(2 ** 44), base=C.c_void_p(2 ** 45))]
    assert ((2 ** 32 - 1) // (F * 7)) % T == 0 and ((2 ** 32 - 1) // (F * 7) + 2) % T == 0
    for kw in edges:                                  # (device 1000 is never there, with a GPU or without)
        a = dict(good, **dict(kw, lay=_lay(device=1000)))
        assert lib.os2ri_perturb(*[a[k] for k in good], None) == abi.ERR_NO_DEVICE and lib.os2ri_last_error().startswith(b"os2ri_perturb: "), kw
    assert not any(buf)
    _source_checks(name, ("overlap_refusal", "null_refusal", r"const char\* shape_refusal", r"const char\* rows_refusal", "is_step", "is_nan"))


def test_update_refusals_come_through_ctypes_without_a_device():
    from gym_os2r_amd import sysid
    lib = sysid.load()
    P, T, M, K, D = 3, 2, 4, 2, 4
    N, E = (2 * P + 1) * M, R.nsums(P)
    buf = (C.c_double * 8192)()
    base = C.addressof(buf)
    at = lambda i: C.c_void_p(base + 8 * i)
    size = dict(obs=K * N * D, meas=K * M * D, done=K * N, prec=D, theta=T * P, theta_best=T * P, cost_best=T, hess=T * P * P, grad=T * P, lam=T,
                status=T, iters=T, theta_best_out=T * P, cost_best_out=T, hess_out=T * P * P, grad_out=T * P, lam_out=T, status_out=T, iters_out=T,
                theta_next=T * P, cost=T, valid=T, accepted=T, failed=T, delta=T * P, sums=E * (M + T), counts=M + T)
    where, nxt = {}, 0
    for n, v in size.items():
        where[n] = nxt
        nxt += v + 1
    assert nxt < 8192
    nan, inf = float("nan"), float("inf")

    def Kc(**kw):
        k = sysid.constants()
        for n, v in kw.items():
            setattr(k, n, v)
        return C.byref(k)
    order = list(size)
    good = dict(lay=_lay(), P=P, T=T, M=M, K=K, h=_dbl(0.1, 0.1, 0.1), lo=_dbl(0, 0, -11), hi=_dbl(1, 1, inf), consts=Kc(),
                **{k: at(where[k]) for k in order})
    name = "os2ri_update"
    assert len(good) + 1 == len(sysid.ENTRY_POINTS[name])
    assert lib.os2ri_update(*[None if _is_pointer(t) else 0 for t in sysid.ENTRY_POINTS[name]]) == abi.ERR_INVALID
    assert lib.os2ri_last_error() == b"os2ri_update: null layout"
    optional = ("done", "cost", "valid", "accepted", "failed", "delta")
    required = [n for n in order if n not in optional]
    end = lambda n: where[n] + size[n] - 1
    cases = _shared(SHARED_CASES) + [
        (dict(lay=_lay(obs_dim=0)), b"obs_dim must be 1..12"), (dict(lay=_lay(obs_dim=13)), b"obs_dim must be 1..12"), (dict(K=0), b"nsteps must be >= 1"),
        (dict(consts=None), b"null constants"), (dict(consts=Kc(lam_min=-1e-9)), b"constants->lam_min must be >= 0"),
        (dict(consts=Kc(diag_floor=0.0)), b"constants->diag_floor must be > 0"), (dict(consts=Kc(diag_floor=-1.0)), b"constants->diag_floor must be > 0")]
    cases += [(dict(consts=Kc(**{n: bad})), b"constants->" + n.encode() + b" must be finite") for n in sysid.CONSTANT_NAMES for bad in (nan, inf, -inf)]
    cases += [(dict(**{n: None}), b"null " + n.encode() + b"_dev") for n in required]
    cases += [(dict(theta_best_out=at(where["theta_best"])), b"theta_best_out_dev overlaps theta_best_dev"),
              (dict(cost_best_out=at(end("obs"))), b"cost_best_out_dev overlaps obs_dev"), (dict(hess_out=at(end("hess"))), b"hess_out_dev overlaps hess_dev"),
              (dict(grad_out=at(where["meas"])), b"grad_out_dev overlaps meas_dev"), (dict(lam_out=at(where["lam"])), b"lam_out_dev overlaps lam_dev"),
              (dict(status_out=at(where["status"])), b"status_out_dev overlaps status_dev"), (dict(iters_out=at(where["prec"])), b"iters_out_dev overlaps prec_dev"),
              (dict(theta_next=at(where["theta"])), b"theta_next_dev overlaps theta_dev"), (dict(theta_next=at(end("theta_best_out"))), b"theta_next_dev overlaps theta_best_out_dev"),
              (dict(cost=at(where["cost_best"])), b"cost_dev overlaps cost_best_dev"), (dict(valid=at(where["done"])), b"valid_dev overlaps done_dev"),
              (dict(accepted=at(where["iters_out"])), b"accepted_dev overlaps iters_out_dev"), (dict(failed=at(where["grad"])), b"failed_dev overlaps grad_dev"),
              (dict(delta=at(where["theta_next"])), b"delta_dev overlaps theta_next_dev"), (dict(sums=at(end("obs"))), b"sums_dev overlaps obs_dev"),
              (dict(sums=at(where["delta"])), b"sums_dev overlaps delta_dev"), (dict(counts=at(end("sums"))), b"counts_dev overlaps sums_dev"),
              (dict(counts=at(where["iters"])), b"counts_dev overlaps iters_dev")]
    seen = _refused(lib, lib.os2ri_update, b"os2ri_update: ", good, cases, buf)
    assert len(required) == 21 and len(seen) == 14 + 6 + 7 + len(required) + 18
    edges = [dict(K=1), dict(done=None, cost=None, valid=None, accepted=None, failed=None, delta=None), dict(consts=Kc(lam_min=0.0, tol=-1.0, cost_floor=-1.0, lam_max=-5.0)),
             dict(counts=at(where["sums"] + size["sums"])), dict(K=2 ** 31 - 1, obs=C.c_void_p(2 ** 50), meas=C.c_void_p(2 ** 44), done=None)]
    for kw in edges:
        a = dict(good, **dict(kw, lay=_lay(device=1000)))
        assert lib.os2ri_update(*[a[k] for k in good], None) == abi.ERR_NO_DEVICE and lib.os2ri_last_error().startswith(b"os2ri_update: "), kw
    assert not any(buf)
    _source_checks(name, ("overlap_refusal", "null_refusal", "constants_refusal", r"const char\* shape_refusal"))


# ---------------------------------------------------------------------------------------
# the restatement against an independent statement
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_restatement_against_a_plain_statement(dtype):
    """float64: cost, H, g and the damped step of the restatement against np.einsum / np.linalg.solve on random problems, every
    segment valid.  float32: the restatement in float32 against itself in float64 on the same float32 inputs."""
    from gym_os2r_amd import sysid
    assert sysid.CHUNKS == R.CHUNKS and {n: getattr(sysid.constants(), n) for n in sysid.CONSTANT_NAMES} == R.DEFAULTS
    worst = dict.fromkeys(MEASURED[dtype], 0.0)
    for T, Q, K, P, D in PLAIN_SHAPES:
        c = R.random_problem(T, Q, K, P, D, np.float64, seed=7)
        M = c["M"]
        if dtype is np.float32:
            for k in ("obs", "meas", "prec", "theta"):
                c[k] = c[k].astype(np.float32)
            c["h"] = c["h"].astype(np.float32).astype(np.float64)
            wide = dict(c, **{k: c[k].astype(np.float64) for k in ("obs", "meas", "prec", "theta")})
            c["state"] = R.fresh_state(c["theta"], 1e-3, np.float32)
            wide["state"] = R.fresh_state(wide["theta"], np.float32(1e-3), np.float64)
            got, want = R.restate(c, np.float32), R.restate(wide, np.float64)
            assert got["accepted"].all() and want["accepted"].all() and not got["failed"].any()
            for n in worst:
                worst[n] = max(worst[n], _far(got[n], want[n]))
            continue
        got = R.restate(c, np.float64)
        assert got["accepted"].all() and (got["valid"] == Q).all() and not got["failed"].any()
        lanes = c["obs"].reshape(K, 2 * P + 1, M, D)
        for t in range(T):
            cost, H, g, delta = R.plain_step(lanes[:, :, t::T].reshape(K, -1, D), c["meas"][:, t::T], c["prec"], c["theta"][t], c["h"], c["lo"], c["hi"],
                                             got["lam"][t], sysid.constants().diag_floor)
            for n, have, want in (("cost", got["cost"][t], cost), ("hess", got["hess"][t], H), ("grad", got["grad"][t], g), ("delta", got["delta"][t], delta)):
                worst[n] = max(worst[n], _far(have, want))
    print({n: f"{v:.3e}" for n, v in worst.items()})
    for n, v in worst.items():
        assert v <= MARGIN * MEASURED[dtype][n], (n, v)


# ---------------------------------------------------------------------------------------
# the whole loop on the CPU oracle
# ---------------------------------------------------------------------------------------
def loop_on_the_oracle(name, oracle):
    from gym_os2r_amd import sysid
    c = R.loop_case(name, oracle)
    assert [sysid.row(c["nq"], f, i) for f, i in c["sel"]] == c["rows"] and sysid.rows(c["nq"]) == c["base"].shape[0]
    S = 2 * len(c["sel"]) + 1
    sim = oracle.OracleSim(c["config"](S * c["M"])[0])
    q0, qd0, actions = np.tile(c["q0"], (1, S)), np.tile(c["qd0"], (1, S)), np.tile(c["actions"], (1, S, 1))       # once, before the loop
    prec = np.ones(c["D"])
    history = R.run_loop(c, lambda params: R.oracle_rollout(sim, c["nq"], params, q0, qd0, actions),
                         lambda obs, done, theta, state: R.restate_update(obs, c["meas"], done, prec, theta, c["h"], c["lo"], c["hi"], state,
                                                                          sysid.constants(), np.float64))     # (lam0 and the defaults)
    sim.close()
    return c, history


@pytest.mark.parametrize("name", ["A", "B"])
def test_the_loop_identifies_the_parameters_on_the_oracle(oracle, name):
    """perturb -> set_params x 5 -> set_state -> K steps -> update, six times, with OracleSim as the simulator and the restatement
    as the update (numpy seed 0, lam0 = 1e-3).  A: fixed_hip, no contact, 8 segments of 5 steps, the damping of hip and knee and
    gravity.  B: free_hip on the ground, 16 segments of 10 steps, mu, friction and mass scale of the knee's body.  cost_best never
    rises and every parameter ends within 1e-4 relative of the truth.  Measured with this restatement at seed 0: 4.9e-11 (A) and
    1.1e-8 (B) -- 2e6 and 9e3 times below the bound --, all segments valid in every iteration, every point accepted."""
    c, history = loop_on_the_oracle(name, oracle)
    truth = np.array(c["truth"])
    best = [h["cost_best"][0] for h in history]
    err = np.abs(history[-1]["theta_best"][0] - truth) / np.abs(truth)
    print(name, "cost_best", best, "relative error", err, "valid", [int(h["valid"][0]) for h in history], "accepted", [int(h["accepted"][0]) for h in history])
    assert len(history) == R.LOOP_ITERS == 6 and all(b <= a for a, b in zip(best, best[1:]))
    assert all(int(h["valid"][0]) == c["M"] for h in history)
    assert (err <= R.LOOP_BOUND).all(), err


# ---------------------------------------------------------------------------------------
# crafted single calls
# ---------------------------------------------------------------------------------------
def check_roles(c, out, dtype):
    """What every role of crafted_roles must come to, whoever computed `out`."""
    role, st, k = c["role"], c["state"], c["consts"]
    P = c["P"]
    same = lambda t: all(np.atleast_1d(out[n][t]).tobytes() == np.atleast_1d(st[n][t]).tobytes() for n in R.STATE)
    t = role["fresh"]
    assert out["accepted"][t] == 1 and out["status"][t] == 0 and out["valid"][t] == 2 and out["iters"][t] == 1 and out["failed"][t] == 0
    assert out["cost_best"][t] == out["cost"][t] and np.array_equal(out["theta_best"][t], c["theta"][t]) and out["lam"][t] == dtype(dtype(1e-3) * dtype(0.5))
    assert np.array_equal(out["theta_next"][t], np.minimum(np.maximum(out["theta_best"][t] + out["delta"][t], c["lo"].astype(dtype)), c["hi"].astype(dtype)))
    assert out["theta_next"][t][1] <= dtype(c["hi"][1]) and np.array_equal(out["hess"][t], out["hess"][t].T) and out["delta"][t].any()
    t = role["reject"]
    assert out["accepted"][t] == 0 and out["status"][t] == 0 and out["lam"][t] == dtype(dtype(1e-3) * dtype(10)) and out["iters"][t] == 1
    for n in ("theta_best", "cost_best", "hess", "grad"):
        assert np.array_equal(out[n][t], st[n][t]), n
    assert out["cost"][t] > st["cost_best"][t] and out["delta"][t].any()          # the step is that of the stored system under the new lam
    t = role["lam_max"]
    assert out["accepted"][t] == 0 and out["status"][t] == 2 and out["lam"][t] == dtype(10) > dtype(k["lam_max"])
    t = role["tol"]
    assert out["accepted"][t] == 1 and out["status"][t] == 1 and out["cost_best"][t] < st["cost_best"][t]
    t = role["cost_floor"]
    assert out["accepted"][t] == 1 and out["status"][t] == 1 and out["cost"][t] <= dtype(k["cost_floor"])
    t = role["no_valid"]
    assert out["valid"][t] == 0 and out["accepted"][t] == 0 and same(t) and np.array_equal(out["theta_next"][t], c["theta"][t]) and not out["delta"][t].any()
    for name in ("done_minus", "nan_plus", "nan_nominal"):
        assert out["valid"][role[name]] == 1 and out["accepted"][role[name]] == 1, name
    t = role["nan_reading"]
    assert out["valid"][t] == 2 and out["accepted"][t] == 1 and np.isfinite(out["cost"][t])
    t = role["frozen"]
    assert same(t) and np.array_equal(out["theta_next"][t], st["theta_best"][t]) and out["status"][t] == 2 and out["iters"][t] == 17
    assert np.isfinite(out["cost"]).sum() == len(R.ROLES) - 1 and not out["failed"].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_crafted_sets_reach_every_branch(dtype):
    from gym_os2r_amd import sysid
    assert sysid.STATE == R.STATE and sysid.CONSTANT_NAMES == R.CONSTANT_NAMES and sysid.MAX_PARAMS == 21
    c = R.crafted_roles(dtype)
    out = R.restate(c, dtype)
    check_roles(c, out, dtype)
    P, t = c["P"], c["role"]["fresh"]
    # the one-sided quotient: parameter 1 sits half a step below its bound, so Delta_1 = 1.5 h, not 2 h
    plus, minus = R.points(c["theta"], c["h"], c["lo"], c["hi"], dtype)
    assert plus[t, 1] == dtype(c["hi"][1]) and abs((plus - minus)[t, 1] / dtype(c["h"][1]) - 1.5) < 1e-5
    assert out["grad"][t, 1] == dtype(out["totals"][1 + 1, t] / (plus - minus)[t, 1])
    # a dropped slot and a skipped reading change nothing but through what is left: garbage there is not read
    d = dict(c, obs=c["obs"].copy(), meas=c["meas"].copy())
    d["obs"][:, :, 1] = 1e30
    d["meas"][:, :, 3] = np.nan
    lanes = d["obs"].reshape(c["K"], 2 * P + 1, c["M"], c["D"])
    lanes[1, :, c["role"]["nan_reading"], 0] = -7e20
    again = R.restate(d, dtype)
    for n in R.STATE + ("theta_next", "cost", "valid"):
        assert np.array_equal(again[n], out[n], equal_nan=True), n
    # a held parameter: unit diagonal, zero row, column and gradient, no step, the others as without it
    h = R.crafted_held(dtype)
    held = R.restate(h, dtype)
    assert held["accepted"].all() and not held["failed"].any() and not held["delta"][:, 2].any() and held["delta"][:, :2].all()
    assert (held["hess"][:, 2, 2] == 1).all() and not held["hess"][:, 2, :2].any() and not held["hess"][:, :2, 2].any() and not held["grad"][:, 2].any()
    assert np.array_equal(held["theta_next"][:, 2], h["theta"][:, 2])
    # a failing pivot
    p = R.crafted_pivot(dtype)
    bad = R.restate(p, dtype)
    assert bad["accepted"][0] == 1 and bad["failed"][0] == 1 and not bad["delta"].any() and np.array_equal(bad["theta_next"], p["theta"])
    assert bad["hess"][0, 0, 0] == 0 and bad["lam"][0] == 0
    # the perturbation: every lane, the unidentified rows, the bounds
    rows = [4, 1, 12]
    basep = np.arange(13 * c["M"], dtype=dtype).reshape(13, c["M"])
    params = R.restate_perturb(c["theta"], basep, rows, c["h"], c["lo"], c["hi"], dtype).reshape(13, 2 * P + 1, c["M"])
    sets = np.arange(c["M"]) % c["T"]
    for r in range(13):
        if r not in rows:
            assert (params[r] == basep[r][None]).all()
    for i, r in enumerate(rows):
        for s in range(2 * P + 1):
            want = plus[sets, i] if s == 1 + i else (minus[sets, i] if s == 1 + P + i else c["theta"][sets, i])
            assert np.array_equal(params[r, s], want), (r, s)


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


def test_python_argument_errors_need_no_device(monkeypatch):
    import torch
    from gym_os2r_amd import sysid
    from gym_os2r_amd.sim import HipSim
    for method in ("sysid_init", "sysid_perturb", "sysid_perturb_into", "sysid_update", "sysid_update_into"):
        assert callable(getattr(HipSim, method))

    def no_load():
        raise AssertionError("a refused call reached sysid.load")
    monkeypatch.setattr(sysid, "load", no_load)
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    s = _bare(f64)
    P, T, M, K, D, F = 3, 2, 4, 2, 4, 13
    N, E = (2 * P + 1) * M, R.nsums(P)
    z = lambda *shape, dtype=f64: torch.zeros(*shape, dtype=dtype)
    for bad in (z(T), z(T, 22), z(0, P), None):
        with pytest.raises(ValueError, match="^sysid_init: "):
            s.sysid_init(bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, None):
        with pytest.raises(ValueError, match="^sysid_init: "):
            s.sysid_init(z(T, P), bad)
    state = s.sysid_init(torch.ones(T, P, dtype=f64))
    assert [tuple(t.shape) for t in state] == [(T, P), (T,), (T, P, P), (T, P), (T,), (T,), (T,)]
    assert (state[0] == 1).all() and torch.isinf(state[1]).all() and not state[2].any() and not state[3].any() and (state[4] == 1e-3).all()
    assert state[5].dtype == i32 and state[6].dtype == i32 and not state[5].any() and not state[6].any()
    sel, h, lo, hi = [(1, 1), (1, 2), (4, 0)], [0.1, 0.1, 0.1], [0, 0, -11], [1, 1, float("inf")]
    ok = dict(sel=sel, h=h, lo=lo, hi=hi)
    theta, base, params = z(T, P), z(F, M), z(F, N)

    def perturb(*args, **kw):
        with pytest.raises(ValueError, match="^sysid_perturb: "):
            s.sysid_perturb_into(*args, **dict(ok, **kw))
    steps = (dict(h=[0.1, 0.0, 0.1]), dict(h=[0.1, float("nan"), 0.1]), dict(h=[0.1, 0.1]), dict(h="x"), dict(h=[]), dict(lo=[0, 2, 0]),
             dict(lo=[0, float("nan"), 0]), dict(hi=[1, 1]), dict(h=[0.1] * 22, lo=[0] * 22, hi=[1] * 22))
    for kw in steps + (dict(sel=None), dict(sel=[(1, 1), (1, 2)]), dict(sel=[(1, 1), (1, 1), (4, 0)]), dict(sel=[(5, 0), (1, 2), (4, 0)]),
                       dict(sel=[(1, 3), (1, 2), (4, 0)]), dict(sel=[(1, 1), (1, 2), (4, 1)]), dict(sel=[(1.0, 1), (1, 2), (4, 0)]), dict(sel=7)):
        perturb(theta, base, params, **kw)
    for args in ((None, base, params), (z(T, P + 1), base, params), (theta.float(), base, params), (theta, None, params), (theta, z(F, 5), params),
                 (theta, z(F + 1, M), params), (theta, base, None), (theta, base, z(F, N + 1)), (theta, base, z(N, F).t()), (theta, base, params.to("meta")),
                 (theta, base, base)):
        perturb(*args)
    with pytest.raises(ValueError, match="^sysid_perturb: "):
        s.sysid_perturb(theta, z(F), **ok)
    perturb(theta, base, params, h=np.array([True, True, True]))
    # a step is judged as the library judges it: rounded once to the handle's dtype
    single = _bare(torch.float32)
    assert single._sysid_steps("x", None, [1e-45], [0], [1])[0] == 1 and s._sysid_steps("x", None, [5e-324, 1e300], [0, 0], [1, 1])[0] == 2
    for bad in ([1e-46], [1e39], [0.0], [-0.0]):
        with pytest.raises(ValueError, match="^x: h"):
            single._sysid_steps("x", None, bad, [0], [1])
    assert not hasattr(HipSim, "sysid_lanes")
    obs, meas, prec, done = z(K, N, D), z(K, M, D), z(D), z(K, N, dtype=u8)
    new = tuple(torch.zeros_like(t) for t in state)
    nxt, sums, counts = z(T, P), z(E * (M + T)), z(M + T, dtype=i32)
    full = (obs, meas, prec, theta, state, new, nxt, sums, counts)
    uok = dict(h=h, lo=lo, hi=hi, constants=sysid.constants())
    swap = lambda seq, i, t: tuple(t if j == i else a for j, a in enumerate(seq))

    def update(*args, **kw):
        with pytest.raises(ValueError, match="^sysid_update: "):
            s.sysid_update_into(*args, **dict(uok, **kw))
    for kw in steps:
        update(*full, **kw)
    broken = sysid.constants()
    broken.tol = float("nan")
    for bad in (None, dict(), broken, sysid.constants(lam_min=-1.0), sysid.constants(diag_floor=0.0)):
        update(*full, constants=bad)
    for args in (swap(full, 0, None), swap(full, 0, z(K, N + 1, D)), swap(full, 0, obs.float()), swap(full, 1, z(K, 5, D)), swap(full, 1, z(K + 1, M, D)),
                 swap(full, 2, None), swap(full, 2, z(D + 1)), swap(full, 3, z(T + 1, P)), swap(full, 4, None), swap(full, 4, state[:6]),
                 swap(full, 4, swap(state, 5, z(T))), swap(full, 4, swap(state, 2, z(T, P, P + 1))), swap(full, 5, state), swap(full, 5, swap(new, 0, nxt)),
                 swap(full, 6, None), swap(full, 6, theta), swap(full, 7, None), swap(full, 7, z(E, M + T)), swap(full, 8, z(M + T)), swap(full, 8, None),
                 swap(full, 7, sums.to("meta"))):
        update(*args)
    for kw in (dict(done=z(K, N)), dict(done=z(K, N + 1, dtype=u8)), dict(cost=z(T + 1)), dict(cost=new[1]), dict(valid=z(T)), dict(accepted=z(T, dtype=i32)),
               dict(failed=counts[:T]), dict(delta=z(T, P + 1)), dict(delta=nxt)):
        update(*full, **kw)
    with pytest.raises(ValueError, match="^sysid_update: "):
        s.sysid_update(obs, z(K, D), prec, theta, state, h=h, lo=lo, hi=hi)
    # what passes every check reaches the loader, and only then (the bare handle has no cfg to fill a layout from)
    with pytest.raises(AttributeError):
        s.sysid_perturb_into(theta, base, params, **ok)
    with pytest.raises(AttributeError):
        s.sysid_update_into(*full, done=done, cost=z(T), valid=z(T, dtype=i32), accepted=z(T, dtype=u8), failed=z(T, dtype=i32), delta=z(T, P), **uok)
