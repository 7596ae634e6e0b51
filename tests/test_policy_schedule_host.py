"""os2r_rollout_policy_scheduled (include/os2r.h): the host side -- declaration, export, bindings, flag values, the null-handle
check, the unchanged ABI minor and the scratch-free policy kernels of the built library.  No GPU needed."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from gym_os2r_amd import abi

NAME = "os2r_rollout_policy_scheduled"


def test_scheduled_rollout_is_declared_exported_and_bound():
    from gym_os2r_amd import _lib
    with open(os.path.join(ROOT, "include", "os2r.h")) as f:
        header = f.read()
    assert re.search(r"OS2R_API int %s\s*\(" % NAME, header)
    assert NAME in _lib.SYMBOLS
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT %s$" % NAME, exported, re.M)
    assert hasattr(_lib.load(), NAME)
    m = importlib.import_module("gym_os2r_amd._os2r_py")
    assert hasattr(m, "rollout_policy_scheduled")


def test_schedule_flags_match_the_header_as_compiled(tmp_path):
    src = tmp_path / "flags.c"
    src.write_text("\n".join([
        "#include <stdio.h>", f'#include "{os.path.join(ROOT, "include", "os2r.h")}"', "int main(void) {",
        '  printf("%d %d %d %d %d %d\\n", OS2R_POLICY_CLOCK_EPISODE, OS2R_POLICY_SCHEDULE_WRAP, OS2R_POLICY_PER_ENV, OS2R_POLICY_TANH,',
        "         OS2R_POLICY_FIRST_EPISODE, OS2R_POLICY_SIGMA_PER_ENV);",
        "  return 0;", "}"]))
    exe = tmp_path / "flags"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    vals = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert vals[:2] == [abi.POLICY_CLOCK_EPISODE, abi.POLICY_SCHEDULE_WRAP] == [16, 32]
    assert vals[2:] == [abi.POLICY_PER_ENV, abi.POLICY_TANH, abi.POLICY_FIRST_EPISODE, abi.POLICY_SIGMA_PER_ENV]
    assert len(set(vals)) == 6                        # distinct from the four old bits and from each other
    for v in vals:
        assert v & (v - 1) == 0                       # single bits


def test_null_handle_is_rejected_without_a_device():
    from gym_os2r_amd import _lib
    lib = _lib.load()
    w = (ctypes.c_double * 64)()
    wp = ctypes.cast(w, ctypes.c_void_p)
    for n in (1, 0):
        assert lib.os2r_rollout_policy_scheduled(None, n, wp, 1, 0, 0, None, 0, None, None, None, None, None, None, None, None,
                                                 None, None) == abi.ERR_INVALID
    m = importlib.import_module("gym_os2r_amd._os2r_py")
    assert m.rollout_policy_scheduled(0, 4, ctypes.addressof(w), 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == abi.ERR_INVALID


def test_abi_minor_is_unchanged():
    """The entry point came without a new minor: a binding looks the symbol up."""
    from gym_os2r_amd import _lib
    lib = _lib.load()
    assert lib.os2r_abi_minor() == abi.ABI_MINOR == 1
    assert lib.os2r_abi_version() == abi.ABI_VERSION == 6


def test_policy_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib
    if not os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs ROCm's llvm-readelf and the built libos2r.so")
    meta = kernel_meta.kernel_meta(_lib.LIB_PATH)
    seen = 0
    for name, m in meta.items():
        if "policy_rollout_kernel<" in name or "policy_kernel<" in name:
            seen += 1
            assert m["private_segment_fixed_size"] == 0, (name, m)
    assert seen >= 28, seen        # twenty fused variants and the eight kernels of the launch loop, at the least
