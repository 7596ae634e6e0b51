"""os2rr_rollout_policy_recorded (include/os2r_record.h, libos2r_record.so): the host side.  The entry point cannot be one of
libos2r.so's: tests/test_bindings_host.py and tests/test_host_api.py hold that library's header, its table of entry points and its
dynamic symbol table to the same 35 names, so it lives in a companion library linked from the same objects, as os2rc_ilqr_backward
does.  Here: declaration, export, both bindings, libos2r.so's symbol table and ABI minor unchanged, the
refusals that need no device, the layout of the kernel argument, the resources of the policy kernels in the built library and the
unchanged shape of what rollout_schedule / rollout_policy return without the recording keywords.  No GPU needed."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from gym_os2r_amd import abi

NAME = "os2rr_rollout_policy_recorded"


def test_recorded_rollout_is_declared_exported_and_bound():
    from gym_os2r_amd import _lib
    assert NAME in _lib.RECORD_ENTRY_POINTS and NAME not in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "os2r_record.h")) as f:
        header = f.read()
    assert re.search(r"OS2R_API int %s\s*\(" % NAME, header)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.RECORD_LIB_PATH], text=True)
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert names == set(_lib.RECORD_ENTRY_POINTS) == set(re.findall(r"\b(os2rr_[a-z_0-9]+)\s*\(", header)), names
    # libos2r.so's symbol table is what it was: the entry points of os2r.h
    main = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert {ln.split()[-1] for ln in main.splitlines() if ln.strip()} == set(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 35
    lib = _lib.load_record()
    assert hasattr(lib, NAME) and lib.os2rr_abi_version() == _lib.RECORD_ABI_VERSION == 1
    m = importlib.import_module("gym_os2r_amd._os2r_py")
    assert hasattr(m, "rollout_policy_recorded") and callable(_lib._PybindLib.os2rr_rollout_policy_recorded)
    # everything from nsteps on is the scheduled entry point, argument for argument
    assert _lib.RECORD_ENTRY_POINTS[NAME][5:] == _lib.ENTRY_POINTS["os2r_rollout_policy_scheduled"][1:]
    assert len(_lib.RECORD_ENTRY_POINTS[NAME]) == 22


def test_abi_minor_is_unchanged():
    from gym_os2r_amd import _lib
    lib = _lib.load()
    assert lib.os2r_abi_minor() == abi.ABI_MINOR == 1
    assert lib.os2r_abi_version() == abi.ABI_VERSION == 6


def test_null_handle_is_refused_through_both_bindings_without_a_device():
    """The one refusal of the C entry point that needs no handle (os2r_create needs a device, and every other cause is written
    into the handle's own error text: tests/test_gpu_rollout_knots.py reads those).  Nothing is written: the buffers handed over
    as device memory are host memory and keep their pattern."""
    from gym_os2r_amd import _lib
    lib, pyb = _lib.load_record(), _lib._PybindLib()
    buf = (C.c_double * 256)(*([7.0] * 256))
    d = C.cast(buf, C.c_void_p)
    for b in (lib, pyb):
        for nsteps in (1, 0):
            rc = b.os2rr_rollout_policy_recorded(None, None, 0, abi.COPY_STATE, d, nsteps, d, 1, 0, 0, None, 0, d, None, d, d, None, d, None,
                                                d, None, None)
            assert rc == abi.ERR_INVALID
            assert b.os2rr_last_error() == b"os2rr_rollout_policy_recorded: null handle"
    assert list(buf) == [7.0] * 256


def _bare(dtype, n=8, nq=3, D=4):
    """A HipSim that never met a device: enough of it for the checks that run before the library is called."""
    import torch
    from gym_os2r_amd.sim import HipSim
    s = HipSim.__new__(HipSim)
    s.N, s.nq, s.D, s.dtype, s.device = n, nq, D, dtype, torch.device("cpu")
    s._h = None
    s._lib = None      # reaching the library would raise AttributeError (or Os2rError), not ValueError
    return s


def test_python_argument_errors_need_no_device():
    import torch
    s, big = _bare(torch.float64), _bare(torch.float64, n=8 * 5)
    w = torch.zeros(2, 2, 5, dtype=torch.float64)
    cases = [(dict(knots=object()), "knots must be a HipSim"),
             (dict(knots=s), "another handle"),
             (dict(knots=_bare(torch.float32, n=40)), "knots must be torch.float64 on cpu"),
             (dict(knots=big, first_knot=-1), "first_knot must be a non-negative"),
             (dict(knots=big, first_knot=True), "first_knot must be a non-negative"),
             (dict(knots=big, knot_state=False, knot_params=False), "nothing to record"),
             (dict(knots=big, first_knot=3), "knots has 40 environments, (first_knot + nsteps) * N = 48"),
             (dict(knots=_bare(torch.float64, n=23)), "knots has 23 environments, (first_knot + nsteps) * N = 24"),
             (dict(first_knot=1), "need a knots handle"),
             (dict(knot_params=False), "need a knots handle")]
    for kw, text in cases:
        for call in (lambda: s.rollout_schedule(3, w, **kw), lambda: s.rollout_policy(3, w[0], **kw)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value).startswith("rollout_schedule: ") and text in str(e.value), (kw, str(e.value))
    other = _bare(torch.float64, n=40)
    other.device = torch.device("meta")
    with pytest.raises(ValueError, match="rollout_schedule: knots must be"):
        s.rollout_schedule(3, w, knots=other)


class _FakeLib:
    """Stands in for the library of a bare HipSim: remembers the calls, returns OK."""

    def __init__(self, with_recorded=True):
        self.calls = []
        for name in ("os2r_rollout_policy", "os2r_rollout_policy_noisy", "os2r_rollout_policy_scheduled") + ((NAME,) if with_recorded else ()):
            setattr(self, name, (lambda n: lambda *a: self.calls.append((n, a)) or abi.OK)(name))

    def os2r_last_error(self, h):
        return b""


def _bare_with(lib, n=8, D=4):
    import torch
    s = _bare(torch.float64, n=n, D=D)
    s._lib = lib
    s._h = C.c_void_p(1)
    s._stream = lambda: None
    return s


def test_the_old_calls_return_what_they_returned_and_the_new_keywords_one_more_element():
    import torch
    lib = _FakeLib()
    s, k = _bare_with(lib), _bare_with(lib, n=8 * 6)
    k._h = C.c_void_p(2)
    w = torch.zeros(2, 2, 5, dtype=torch.float64)
    assert len(s.rollout_policy(3, w[0])) == 3 and lib.calls[-1][0] == "os2r_rollout_policy"
    assert len(s.rollout_policy(3, w[0], sigma=0.1)) == 4 and lib.calls[-1][0] == "os2r_rollout_policy_noisy"
    assert len(s.rollout_schedule(3, w)) == 4 and lib.calls[-1][0] == "os2r_rollout_policy_scheduled"
    n_before = len(lib.calls)
    out = s.rollout_schedule(3, w, knots=k, first_knot=2, knot_params=False, want_knot_obs=True, first_slot=1, want_actions=True)
    assert len(out) == 5 and tuple(out[4].shape) == (3, 8, 4) and tuple(out[3][0].shape) == (3, 8, 2)
    name, a = lib.calls[-1]
    assert name == NAME and len(lib.calls) == n_before + 1 and len(a) == 22
    # (sim, knots, first_knot, what, knot_obs, nsteps, weights, period, first_slot, ...)
    assert a[0].value == 1 and a[1].value == 2 and a[2:4] == (2, abi.COPY_STATE) and a[4].value == out[4].data_ptr()
    assert a[5] == 3 and a[7:9] == (2, 1)
    out = s.rollout_schedule(3, w, want_knot_obs=True)                      # the observations alone: no handle, nothing selected
    name, a = lib.calls[-1]
    assert len(out) == 5 and name == NAME and a[1] is None and a[2:4] == (0, 0) and a[4].value == out[4].data_ptr()
    out = s.rollout_policy(3, w[0], knots=k)                                # period 1 is os2r_rollout_policy itself
    name, a = lib.calls[-1]
    assert len(out) == 5 and out[3] == (None, None) and out[4] is None and name == NAME
    assert a[2:4] == (0, abi.COPY_STATE | abi.COPY_PARAMS) and a[4] is None and a[7:9] == (1, 0)


def test_a_missing_companion_library_is_named(monkeypatch, tmp_path):
    import torch
    from gym_os2r_amd import _lib
    from gym_os2r_amd.sim import Os2rError
    lib = _FakeLib(with_recorded=False)
    s = _bare_with(lib)
    w = torch.zeros(2, 2, 5, dtype=torch.float64)
    monkeypatch.setattr(_lib, "_record", None)
    monkeypatch.setattr(_lib, "RECORD_LIB_PATH", str(tmp_path / "libos2r_record.so"))
    with pytest.raises(Os2rError, match="libos2r_record.so"):
        s.rollout_schedule(3, w, want_knot_obs=True)
    assert lib.calls == []
    assert len(s.rollout_schedule(3, w)) == 4                               # what it has still works


def test_the_sink_is_appended_to_the_policy_arguments():
    """PolicyArgs grew at its end only: the StepArgs first, the fields of the earlier entry points in their order, then the sink's
    (a kernel built before them reads the same offsets)."""
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", "os2r_kernels.hpp")) as f:
        src = f.read()
    body = re.search(r"struct PolicyArgs \{(.*?)\n\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    fields = re.findall(r"(\w+)\s*;", body)
    old = ["s", "w", "flags", "ret", "len", "act", "open", "sigma", "act_out", "eps_out", "salt", "period", "first_slot"]
    assert fields[:len(old)] == old
    sink = fields[len(old):]
    assert sink[:3] == ["knot_what", "knot_stride", "knot_lane"] and sink[-1] == "knot_obs"
    assert set(sink[3:-1]) == {"kq", "kqd", "khist", "ksolver_l", "ksolver_flags", "ksteps", "kepisode", "kpose", "kmass_scale",
                               "kdamping", "kfriction", "kmu", "kgravity"}
    # step_kernel's template parameter list is the one tests/test_policy_rollout_host.py matches: nine parameters, ROLLOUT last
    at = src.index("void step_kernel(const StepArgs<T> A)")
    assert re.search(r"bool ROLLOUT = false>\s*__global__ OS2R_STEP_KERNEL_ATTRS\(T\) $", src[:at])


def _meta():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib
    if not os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")) or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("needs ROCm's llvm-readelf and the built libos2r.so")
    return kernel_meta.kernel_meta(_lib.LIB_PATH)


def test_recording_kernels_have_names_of_their_own_and_the_old_ones_keep_their_limits():
    """The recording is a template flag of step_body instantiated as policy_record_kernel, one beside every policy_rollout_kernel
    (as a run-time branch of those it cost the unrecorded calls 1.4 - 3 % of their rate: profiles/rollout_knots_rate.txt).  The
    existing variants keep their names and their limits -- no scratch, at most 8 spilled VGPRs, fp32 within 256 VGPRs for two
    waves per SIMD --, the new ones meet the same, and every kernel that takes a PolicyArgs sees it with the sink appended."""
    meta = _meta()

    def variants(kernel):
        out = {}
        for name, m in meta.items():
            k = re.search(kernel + r"<((float|double), os2r::StModel<\2, \d>, true, (?:true|false), os2r::StLayout<\d+ull, \d+ull, \d+>)\s*>", name)
            if k:
                out[k.group(1)] = m
        return out
    fused, recording = variants("policy_rollout_kernel"), variants("policy_record_kernel")
    loops = {k: m for k, m in meta.items() if re.search(r"policy_kernel<(float|double), [2-5]>", k)}
    assert len(fused) >= 20 and len(loops) == 8
    assert set(recording) == set(fused)
    for group in (fused, recording):
        for key, m in group.items():
            assert m["private_segment_fixed_size"] == 0, (key, m)
            assert m["vgpr_spill_count"] <= 8, (key, m)
            if key.startswith("float"):
                assert m["vgpr_count"] <= 256, (key, m["vgpr_count"])
    for m in loops.values():
        assert m["private_segment_fixed_size"] == 0, m
    sizes = {(key.startswith("float"), m["kernarg_segment_size"]) for group in (fused, recording) for key, m in group.items()}
    sizes |= {("policy_kernel<float" in k, m["kernarg_segment_size"]) for k, m in loops.items()}
    assert len(sizes) == 2, sizes                     # one PolicyArgs per dtype, in every kernel that takes it
    # nothing that is not a policy kernel carries the recording code: step_kernel's template parameters are what they were
    assert not any("record" in k for k in meta if "policy_record_kernel<" not in k)
