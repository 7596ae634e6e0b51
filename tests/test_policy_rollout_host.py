"""os2r_rollout_policy (include/os2r.h): the host side -- declaration, export, bindings, flag values, argument checks and the
resources of its kernels in the built library.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from gym_os2r_amd import abi


def test_rollout_policy_is_declared_exported_and_bound():
    import importlib
    from gym_os2r_amd import _lib
    with open(os.path.join(ROOT, "include", "os2r.h")) as f:
        header = f.read()
    assert re.search(r"OS2R_API int os2r_rollout_policy\s*\(", header)
    assert "os2r_rollout_policy" in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "os2r_rollout_policy")
    assert _lib.load().os2r_abi_version() == abi.ABI_VERSION == 6
    m = importlib.import_module("gym_os2r_amd._os2r_py")
    assert hasattr(m, "rollout_policy")


def test_policy_flags_match_the_header_as_compiled(tmp_path):
    src = tmp_path / "flags.c"
    src.write_text("\n".join([
        "#include <stdio.h>", f'#include "{os.path.join(ROOT, "include", "os2r.h")}"', "int main(void) {",
        '  printf("%d %d %d %d\\n", OS2R_POLICY_PER_ENV, OS2R_POLICY_TANH, OS2R_POLICY_FIRST_EPISODE, OS2R_ABI_VERSION);',
        "  return 0;", "}"]))
    exe = tmp_path / "flags"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(src)])
    vals = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert vals == [abi.POLICY_PER_ENV, abi.POLICY_TANH, abi.POLICY_FIRST_EPISODE, abi.ABI_VERSION]
    assert len({abi.POLICY_PER_ENV, abi.POLICY_TANH, abi.POLICY_FIRST_EPISODE}) == 3


def test_null_handle_is_rejected_without_a_device():
    import importlib
    from gym_os2r_amd import _lib
    lib = _lib.load()
    w = (ctypes.c_double * 64)()
    for n in (1, 0):
        assert lib.os2r_rollout_policy(None, n, ctypes.cast(w, ctypes.c_void_p), 0, None, None, None, None, None, None, None,
                                       None) == abi.ERR_INVALID
    m = importlib.import_module("gym_os2r_amd._os2r_py")
    assert m.rollout_policy(0, 4, ctypes.addressof(w), 0, 0, 0, 0, 0, 0, 0, 0, 0) == abi.ERR_INVALID


def _meta():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib
    if not os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs ROCm's llvm-readelf and the built libos2r.so")
    return kernel_meta.kernel_meta(_lib.LIB_PATH)


def _fused_rollout_key(name):
    """(dtype, model, layout, DR) of a fused rollout variant of step_kernel / of a policy_rollout_kernel."""
    m = re.search(r"<(float|double), os2r::StModel<\1, (\d)>, true, (true|false), .*?(os2r::StLayout<\d+ull, \d+ull, \d+>)", name)
    return m and (m.group(1), m.group(2), m.group(4), m.group(3))


def test_policy_kernels_exist_wherever_a_fused_rollout_does_and_fit_the_registers():
    meta = _meta()
    rollouts, policies = set(), {}
    for name, m in meta.items():
        if "step_kernel<" in name and re.search(r", true>\(os2r::StepArgs<", name) and re.search(r", (true|false), \d, true>\(", name):
            rollouts.add(_fused_rollout_key(name))
        if "policy_rollout_kernel<" in name:
            policies[_fused_rollout_key(name)] = (name, m)
    assert len(rollouts) >= 20 and None not in rollouts, len(rollouts)
    assert set(policies) == rollouts, sorted(set(policies) ^ rollouts)[:4]
    for key, (name, m) in policies.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)     # no scratch
        assert m["vgpr_spill_count"] <= 8, (name, m)
        if key[0] == "float":
            assert m["vgpr_count"] <= 256, (name, m["vgpr_count"])  # two waves per SIMD
    # the launch loop's policy kernels: one per chain length of the run-time-model units, per dtype
    loops = [k for k in meta if re.search(r"policy_kernel<(float|double), [2-5]>", k)]
    assert len(loops) == 8, loops
    assert sum("policy_accumulate_kernel<" in k for k in meta) == 2


def test_configs_stamped_with_the_previous_abi_are_still_accepted():
    """ABI 6 added an entry point, not a field: os2r_create takes configs stamped 5 or 6 and refuses any other stamp (checked
    before any device is looked for)."""
    from helpers import make_config
    from gym_os2r_amd import _lib
    lib = _lib.load()
    cfg, _, _ = make_config("free_hip", num_envs=8, contact=True)
    for stamp, accepted in ((4, False), (5, True), (6, True), (7, False)):
        cfg.abi_version = stamp
        out = ctypes.c_void_p()
        rc = lib.os2r_create(ctypes.byref(cfg), ctypes.byref(out))
        msg = lib.os2r_last_error(None).decode()
        if rc == abi.OK:
            lib.os2r_destroy(out)
        assert (rc == abi.ERR_INVALID and "abi_version mismatch" in msg) == (not accepted), (stamp, rc, msg)
