"""os2r_copy_envs (include/os2r.h): the host side -- declaration, export, bindings, the unchanged ABI numbers, flag values, the
null-handle refusals and the resources of the copy kernel in the built library.  No GPU needed."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from gym_os2r_amd import abi


def test_copy_envs_is_declared_exported_and_bound():
    from gym_os2r_amd import _lib
    with open(os.path.join(ROOT, "include", "os2r.h")) as f:
        header = f.read()
    assert re.search(r"OS2R_API int os2r_copy_envs\s*\(", header)
    assert "os2r_copy_envs" in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "os2r_copy_envs")
    assert hasattr(importlib.import_module("gym_os2r_amd._os2r_py"), "copy_envs")
    import shutil
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert "os2r_copy_envs" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    from gym_os2r_amd.sim import HipSim, _PybindLib
    assert callable(HipSim.copy_envs_from) and callable(_PybindLib.os2r_copy_envs)


def test_abi_numbers_stay_and_the_flags_as_compiled(tmp_path):
    """The entry point came without a new ABI minor (a binding looks the symbol up); the two selection bits of the header, as
    gcc compiles them, are abi.py's."""
    from gym_os2r_amd import _lib
    lib = _lib.load()
    assert lib.os2r_abi_version() == 6 and lib.os2r_abi_minor() == 1
    src = tmp_path / "flags.c"
    src.write_text("\n".join([
        "#include <stdio.h>", f'#include "{os.path.join(ROOT, "include", "os2r.h")}"', "int main(void) {",
        '  printf("%d %d %d %d\\n", OS2R_COPY_STATE, OS2R_COPY_PARAMS, OS2R_ABI_VERSION, OS2R_ABI_MINOR);', "  return 0;", "}"]))
    exe = tmp_path / "flags"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    vals = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert vals == [abi.COPY_STATE, abi.COPY_PARAMS, 6, 1]
    assert abi.COPY_STATE != abi.COPY_PARAMS and abi.COPY_STATE & abi.COPY_PARAMS == 0


def test_null_handles_are_rejected_without_a_device():
    """A null destination or a null source is OS2R_ERR_INVALID through both bindings, with a message; a fake non-null handle
    next to the null one is never looked into."""
    from gym_os2r_amd import _lib
    lib = _lib.load()
    both = abi.COPY_STATE | abi.COPY_PARAMS
    assert lib.os2r_copy_envs(None, None, None, both, None, None) == abi.ERR_INVALID
    assert b"os2r_copy_envs" in lib.os2r_last_error(None) and b"null" in lib.os2r_last_error(None)
    buf = (ctypes.c_double * 64)()
    assert lib.os2r_copy_envs(None, ctypes.cast(buf, ctypes.c_void_p), None, both, None, None) == abi.ERR_INVALID
    m = importlib.import_module("gym_os2r_amd._os2r_py")
    assert m.copy_envs(0, 0, 0, both, 0, 0) == abi.ERR_INVALID
    assert m.copy_envs(0, ctypes.addressof(buf), 0, both, 0, 0) == abi.ERR_INVALID
    assert "null" in m.last_error(0)


def test_null_source_is_refused_before_anything_else():
    """The null-source check needs a destination handle to be reached, so without a device the source is read: in the entry
    point both null checks come first, each with its message, before `what` or the handles' fields are looked at."""
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "os2r_capi.hip")) as f:
        src = f.read()
    body = re.search(r"int os2r_copy_envs\(.*?\n}\n", src, re.S).group(0)
    lines = [ln.strip() for ln in body.splitlines()[1:]]
    assert lines[0].startswith("if (!dst)") and "null destination" in lines[0] and "OS2R_ERR_INVALID" in lines[0]
    assert lines[1].startswith("if (!src)") and "null source" in lines[1] and "OS2R_ERR_INVALID" in lines[1]
    assert "OS2R_COPY_STATE | OS2R_COPY_PARAMS" in body and "same_model" in body


def test_copy_kernel_resources():
    """The copy kernel is pure memory movement at full occupancy: no scratch (private segment 0, no scratch instruction in the
    disassembly), no LDS, no register spill, and few enough registers for at least four waves per SIMD (512 / 128).  The
    observation kernel behind obs_dev carries observe() and the LDS tile of the coalesced [N][D] store; it has no scratch
    either."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    import isa_histogram
    from gym_os2r_amd import _lib
    if not os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs ROCm's llvm-readelf and the built libos2r.so")
    meta = kernel_meta.kernel_meta(_lib.LIB_PATH)
    copy = {k: m for k, m in meta.items() if "copy_envs_kernel<" in k}
    assert len(copy) == 2 and any("<float>" in k for k in copy) and any("<double>" in k for k in copy), sorted(copy)
    for name, m in copy.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] + (m["agpr_count"] or 0) <= 128, (name, "vgpr_count", m["vgpr_count"], "agpr_count", m["agpr_count"])
        _, _, insts = isa_histogram.disassemble(_lib.LIB_PATH, name[name.index("copy_envs_kernel<"):name.index(">(") + 2])
        assert insts and not [i for i in insts if i[1].startswith("scratch_")], name
        # a group's loads are issued before its stores: somewhere kCopyGroup = 8 loads of the handle's dtype follow each other
        # with no store between them
        width = "global_load_dwordx2" if "<double>" in name else "global_load_dword"
        run = best = 0
        for _, mn, _ in insts:
            run = run + 1 if mn == width else 0 if mn.startswith("global_store") else run
            best = max(best, run)
        assert best >= 8, (name, best)
    obs = {k: m for k, m in meta.items() if "copy_envs_obs_kernel<" in k}
    assert len(obs) == 8, sorted(obs)
    for name, m in obs.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] + (m["agpr_count"] or 0) <= 128, (name, m["vgpr_count"])
