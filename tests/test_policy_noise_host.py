"""os2r_rollout_policy_noisy (include/os2r.h): the host side -- declaration, export, bindings, the ABI minor, flag values,
argument checks and the resources of the policy kernels in the built library.  No GPU needed."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from gym_os2r_amd import abi


def test_noisy_rollout_is_declared_exported_and_bound():
    from gym_os2r_amd import _lib
    with open(os.path.join(ROOT, "include", "os2r.h")) as f:
        header = f.read()
    for sym in ("os2r_rollout_policy_noisy", "os2r_abi_minor"):
        assert re.search(r"OS2R_API int %s\s*\(" % sym, header), sym
        assert sym in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
        assert hasattr(importlib.import_module("gym_os2r_amd._os2r_py"), sym[len("os2r_"):])
    import shutil
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert {"os2r_rollout_policy_noisy", "os2r_abi_minor"} <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_abi_minor_and_the_new_flag_as_compiled(tmp_path):
    from gym_os2r_amd import _lib
    lib = _lib.load()
    assert lib.os2r_abi_minor() == abi.ABI_MINOR == 1
    assert importlib.import_module("gym_os2r_amd._os2r_py").abi_minor() == 1
    assert lib.os2r_abi_version() == abi.ABI_VERSION == 6
    src = tmp_path / "flags.c"
    src.write_text("\n".join([
        "#include <stdio.h>", f'#include "{os.path.join(ROOT, "include", "os2r.h")}"', "int main(void) {",
        '  printf("%d %d %d %d %d %d\\n", OS2R_POLICY_SIGMA_PER_ENV, OS2R_POLICY_PER_ENV, OS2R_POLICY_TANH,',
        "         OS2R_POLICY_FIRST_EPISODE, OS2R_ABI_VERSION, OS2R_ABI_MINOR);", "  return 0;", "}"]))
    exe = tmp_path / "flags"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    vals = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert vals == [abi.POLICY_SIGMA_PER_ENV, abi.POLICY_PER_ENV, abi.POLICY_TANH, abi.POLICY_FIRST_EPISODE, 6, 1]
    assert len({abi.POLICY_SIGMA_PER_ENV, abi.POLICY_PER_ENV, abi.POLICY_TANH, abi.POLICY_FIRST_EPISODE}) == 4


def test_null_handle_is_rejected_without_a_device():
    """Without a handle every call is OS2R_ERR_INVALID, whatever else is wrong with it (nsteps < 1, null weights, null sigma);
    the argument checks behind a valid handle are in tests/test_gpu_policy_noise.py."""
    from gym_os2r_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for n, w, sg in ((1, p, p), (0, p, p), (-3, p, p), (1, None, p), (1, p, None)):
        assert lib.os2r_rollout_policy_noisy(None, n, w, 0, sg, 7, None, None, None, None, None, None, None, None, None,
                                             None) == abi.ERR_INVALID
    m = importlib.import_module("gym_os2r_amd._os2r_py")
    a = ctypes.addressof(buf)
    assert m.rollout_policy_noisy(0, 4, a, 0, a, 7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == abi.ERR_INVALID
    assert m.rollout_policy_noisy(0, 4, a, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == abi.ERR_INVALID


def test_the_deterministic_entry_point_does_not_know_the_new_flag():
    """os2r_rollout_policy's check of its flag bits (csrc/os2r_capi.hip) sits behind the null-handle check, so without a device
    the source is read: its mask names the three old bits and not OS2R_POLICY_SIGMA_PER_ENV; the noisy entry point's names all
    four.  (The refusal itself, with a handle, is in tests/test_gpu_policy_noise.py.)"""
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "os2r_capi.hip")) as f:
        src = f.read()
    old = re.search(r"int os2r_rollout_policy\(.*?\n}\n", src, re.S).group(0)
    new = re.search(r"int os2r_rollout_policy_noisy\(.*?\n}\n", src, re.S).group(0)
    mask_old = re.search(r"flags & ~\(([^)]*)\)", old).group(1)
    mask_new = re.search(r"flags & ~\(([^)]*)\)", new).group(1)
    names = lambda s: {x.strip() for x in s.split("|")}
    assert names(mask_old) == {"OS2R_POLICY_PER_ENV", "OS2R_POLICY_TANH", "OS2R_POLICY_FIRST_EPISODE"}
    assert names(mask_new) == names(mask_old) | {"OS2R_POLICY_SIGMA_PER_ENV"}
    assert "sigma" not in old and "null sigma" in new


def test_policy_kernels_have_no_scratch():
    """Every kernel that evaluates the policy -- the fused policy_rollout_kernel variants and the launch loop's policy_kernel --
    has a private segment of 0 bytes with the noise branch in it (the register bounds are those of
    tests/test_policy_rollout_host.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib
    if not os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs ROCm's llvm-readelf and the built libos2r.so")
    meta = kernel_meta.kernel_meta(_lib.LIB_PATH)
    pol = {k: m for k, m in meta.items() if "policy_rollout_kernel<" in k or re.search(r"policy_kernel<(float|double), [2-5]>", k)}
    assert len(pol) >= 20 + 8, len(pol)
    for name, m in pol.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
