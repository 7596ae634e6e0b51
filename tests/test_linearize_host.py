"""os2r_linearize (include/os2r.h): the host side -- declaration, export, bindings, the unchanged ABI numbers, the null-handle
refusal, the resources of the linearise kernels in the built library and the argument checks of HipSim.linearize that need
no device.  No GPU needed."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT
from gym_os2r_amd import abi


def test_linearize_is_declared_exported_and_bound():
    from gym_os2r_amd import _lib
    with open(os.path.join(ROOT, "include", "os2r.h")) as f:
        header = f.read()
    assert re.search(r"OS2R_API int os2r_linearize\s*\(Os2rSim\* sim, const void\* actions_dev, const double eps\[3\]", header)
    assert "os2r_linearize" in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "os2r_linearize")
    assert hasattr(importlib.import_module("gym_os2r_amd._os2r_py"), "linearize")
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert "os2r_linearize" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    from gym_os2r_amd.sim import HipSim, _PybindLib
    assert callable(HipSim.linearize) and callable(HipSim.linearize_into) and callable(_PybindLib.os2r_linearize)


def test_abi_numbers_stay():
    """The entry point came without a new ABI minor: a binding looks the symbol up."""
    from gym_os2r_amd import _lib
    lib = _lib.load()
    assert lib.os2r_abi_version() == 6 and lib.os2r_abi_minor() == 1
    assert importlib.import_module("gym_os2r_amd._os2r_py").abi_minor() == 1
    with open(os.path.join(ROOT, "include", "os2r.h")) as f:
        header = f.read()
    assert re.search(r"#define OS2R_ABI_MINOR 1\b", header)


def test_null_handle_is_rejected_without_a_device():
    from gym_os2r_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    eps = (ctypes.c_double * 3)(1e-6, 1e-6, 1e-6)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.os2r_linearize(None, p, eps, p, p, p, None) == abi.ERR_INVALID
    assert b"os2r_linearize" in lib.os2r_last_error(None) and b"null handle" in lib.os2r_last_error(None)
    m = importlib.import_module("gym_os2r_amd._os2r_py")
    a = ctypes.addressof(buf)
    assert m.linearize(0, a, 1e-6, 1e-6, 1e-6, a, a, a, 0) == abi.ERR_INVALID
    assert "null handle" in m.last_error(0)


def test_refusals_come_before_the_handle_is_looked_into():
    """Every cause of include/os2r.h has its own message in the entry point, and the eps values are tested on their bit pattern
    (the library is built without NaN semantics) before any comparison."""
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "os2r_capi.hip")) as f:
        src = f.read()
    body = re.search(r"int os2r_linearize\(.*?\n}\n", src, re.S).group(0)
    for msg in ("null handle", "null actions", "null eps", "all three outputs are null", "eps must be finite", "eps must be positive",
                "must be < 1"):
        assert msg in body, msg
    assert body.index("is_finite(&eps[k])") < body.index("eps[k] > 0.0") < body.index("DeviceGuard")


def test_linearize_kernel_resources():
    """The budget of the step kernels (test_code_objects_of_the_built_library_have_no_scratch_and_no_runtime_tables), applied to
    the linearise kernels: no scratch traffic (a few bytes of SGPR-spill bookkeeping excepted: then no vector spill and no
    scratch instruction), fp32 variants within 256 unified registers, no robot table as a data symbol; variants for both
    dtypes, the compiled-in robots and the run-time models."""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    import isa_histogram
    from gym_os2r_amd import _lib
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) and os.path.exists(_lib.LIB_PATH)
    meta = kernel_meta.kernel_meta(_lib.LIB_PATH)
    lin = {k: v for k, v in meta.items() if "linearize_kernel<" in k}
    for real in ("float", "double"):
        st = [k for k in lin if f"linearize_kernel<{real}, os2r::StModel<" in k]
        rt = [k for k in lin if f"linearize_kernel<{real}, os2r::RtModel<" in k]
        # contact {on, off} x per-env parameters {on, off}: the four robots (the 2-dof one has no contact variant) and the
        # chains of 2..5 dofs; fp64 once per solver, the compiled-in robots also with the default sweep counts folded in
        assert len(st) == (42 if real == "double" else 28), (real, len(st))
        assert len(rt) == (32 if real == "double" else 16), (real, len(rt))
        for nq in (2, 3, 4, 5):
            assert any(f"RtModel<{real}, {nq}>" in k for k in rt), (real, nq)
        for mid in range(4):
            assert any(f"StModel<{real}, {mid}>" in k for k in st), (real, mid)
    for name, m in lin.items():
        if m["private_segment_fixed_size"] != 0:
            needle = name[name.index("linearize_kernel<"):name.index(">(os2r::LinArgs") + 2]
            _, _, insts = isa_histogram.disassemble(_lib.LIB_PATH, needle)
            assert m["vgpr_spill_count"] == 0 and not [i for i in insts if i[1].startswith("scratch_")], (name, m)
            assert m["private_segment_fixed_size"] <= 68, (name, m)
        assert m["vgpr_spill_count"] <= 8, (name, m)                # AGPR spill slots of the register allocator, a handful at most
        if "linearize_kernel<float" in name:
            assert m["vgpr_count"] <= 256, (name, m["vgpr_count"])
    tables = []
    for co in kernel_meta.code_objects(_lib.LIB_PATH):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            out = subprocess.run([os.path.join(kernel_meta.LLVM, "llvm-readelf"), "--symbols", f.name], capture_output=True, text=True).stdout
        tables += [ln.split()[-1] for ln in out.splitlines() if ("Tables" in ln or "CandMeta" in ln) and "OBJECT" in ln]
    assert not tables, sorted(set(tables))[:5]


def _bare(dtype, n=8, nq=3):
    """A HipSim that never met a device: enough of it for the checks that run before the library is called."""
    import torch
    from gym_os2r_amd.sim import HipSim
    s = HipSim.__new__(HipSim)
    s.N, s.nq, s.D, s.dtype, s.device = n, nq, 4, dtype, torch.device("cpu")
    s._h = None
    s._lib = None      # reaching the library would raise AttributeError, not ValueError
    return s


def test_python_argument_errors_need_no_device():
    import torch
    s = _bare(torch.float64)
    assert s._linearize_eps(None) == (torch.finfo(torch.float64).eps ** (1 / 3),) * 3
    assert _bare(torch.float32)._linearize_eps(None) == (torch.finfo(torch.float32).eps ** (1 / 3),) * 3
    assert s._linearize_eps(1e-5) == (1e-5, 1e-5, 1e-5) and s._linearize_eps([1e-5, 2e-5, 3e-5]) == (1e-5, 2e-5, 3e-5)
    for bad in (0.0, -1e-6, float("nan"), float("inf"), (1e-6, 1e-6), (1e-6, 1e-6, 1.0), (1e-6, 0.0, 1e-6), (1e-6, 1e-6, float("nan")),
                True, "x", (1e-6, 1e-6, 1e-6, 1e-6), 1.0):
        with pytest.raises(ValueError, match="linearize"):
            s._linearize_eps(bad)
    act = torch.zeros(8, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="nothing asked for"):
        s.linearize(act, want_next=False, want_A=False, want_B=False)
    with pytest.raises(ValueError, match="expected shape"):
        s.linearize(torch.zeros(7, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="nothing asked for"):
        s.linearize_into(act)
    with pytest.raises(ValueError, match="actions are required"):
        s.linearize_into(None, A_out=torch.zeros(6, 6, 8, dtype=torch.float64))
    good_a = torch.zeros(6, 6, 8, dtype=torch.float64)
    for kw in (dict(actions=act.float(), A_out=good_a),                                  # dtype of the actions
               dict(actions=act[:, :1], A_out=good_a),                                   # shape of the actions
               dict(actions=act, A_out=torch.zeros(8, 6, 6, dtype=torch.float64)),       # the public layout is not the kernel's
               dict(actions=act, A_out=good_a.float()),
               dict(actions=act, A_out=torch.zeros(6, 8, 6, dtype=torch.float64).permute(0, 2, 1)),   # not contiguous
               dict(actions=act, B_out=torch.zeros(6, 3, 8, dtype=torch.float64)),
               dict(actions=act, next_out=torch.zeros(3, 8, dtype=torch.float64)),
               dict(actions=act, next_out=[0.0] * 48)):
        with pytest.raises(ValueError, match="linearize"):
            s.linearize_into(eps=1e-6, **kw)
