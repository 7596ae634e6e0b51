"""gym_os2r_amd._lib.ENTRY_POINTS, the one table both bindings are made from: held against the prototypes of include/os2r.h
(names, order, argument counts, argument and result classes), and every entry point called through both bindings -- the
ctypes library and the adapter over the pybind11 module -- with nothing in its arguments, which each refuses before it
looks for a device.  No GPU needed."""
import ctypes as C
import importlib
import inspect
import re

import pytest

from gym_os2r_amd import _lib, abi
from header_check import _agrees, _is_pointer, _prototypes

def test_the_table_is_the_header():
    protos = _prototypes("os2r.h", "os2r")
    assert len(protos) == 35
    assert [p[0] for p in protos] == list(_lib.ENTRY_POINTS) == _lib.SYMBOLS
    lib = _lib.load()
    for name, ret, args in protos:
        argtypes = _lib.ENTRY_POINTS[name]
        assert len(argtypes) == len(args), (name, args, argtypes)
        for text, ctype in zip(args, argtypes):
            assert _agrees(text, ctype, True), (name, text, ctype)
        fn = getattr(lib, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name               # load() took the table as it is
        assert _agrees(ret, fn.restype, False), (name, ret, fn.restype)
        assert fn.restype is (C.c_char_p if name == "os2r_last_error" else C.c_int)


def test_the_adapter_has_every_entry_point():
    for name in _lib.ENTRY_POINTS:
        assert callable(vars(_lib._PybindLib)[name]), name
    from gym_os2r_amd import sim
    assert sim._PybindLib is _lib._PybindLib
    written_out = set(re.findall(r"def (os2r_[a-z0-9_]+)\(", inspect.getsource(_lib._PybindLib)))
    assert written_out == {"os2r_create", "os2r_get_step_count", "os2r_get_violation_mirror", "os2r_bench_steps",
                           "os2r_bench_steps_multi", "os2r_linearize", "os2r_last_error"}


def test_what_a_pointer_argument_may_be():
    a = _lib._a
    buf, word = (C.c_double * 4)(), C.c_uint64(7)
    assert a(None) == 0 and a(0) == 0 and a(4096) == 4096
    assert a(C.c_void_p()) == 0 and a(C.c_void_p(4096)) == 4096
    assert a(buf) == C.addressof(buf) and a(word) == C.addressof(word) and a(C.byref(word)) == C.addressof(word)
    assert a(C.cast(buf, C.c_void_p)) == C.addressof(buf)


def test_both_bindings_take_every_entry_point_without_a_device():
    lib, pyb = _lib.load(), _lib._PybindLib()
    one_by_one = {"os2r_abi_version", "os2r_abi_minor", "os2r_last_error", "os2r_model_is_compiled_in", "os2r_get_violation_mirror"}
    for name, argtypes in _lib.ENTRY_POINTS.items():
        if name in one_by_one:
            continue
        # (the one char* is a path, which the module takes as a str: empty, and the null model is what is refused)
        nothing = [b"" if t is C.c_char_p else None if _is_pointer(t) else 0 for t in argtypes]
        assert getattr(lib, name)(*nothing) == abi.ERR_INVALID, name            # (a wrong arity raises)
        assert getattr(pyb, name)(*nothing) == abi.ERR_INVALID, name
        with pytest.raises((TypeError, ValueError)):
            getattr(pyb, name)(*nothing, 0)
        with pytest.raises((TypeError, ValueError)):
            getattr(pyb, name)(*nothing[:-1])
    for b in (lib, pyb):
        assert b.os2r_abi_version() == abi.ABI_VERSION and b.os2r_abi_minor() == abi.ABI_MINOR
        assert b.os2r_model_is_compiled_in(None) == 0
        words = C.c_void_p()
        assert b.os2r_get_violation_mirror(None, C.byref(words)) == abi.ERR_INVALID and not words.value
        assert b.os2r_create(None, C.byref(words)) == abi.ERR_INVALID and not words.value
        assert b.os2r_last_error(None) == b"null config"
        assert b.os2r_copy_envs(None, None, None, 0, None, None) == abi.ERR_INVALID
        assert b.os2r_last_error(None) == b"os2r_copy_envs: null destination handle"
        # of the three policy rollouts only the scheduled one names a null handle in the thread's error
        assert b.os2r_rollout_policy(*[None, 0, None, 0] + [None] * 8) == abi.ERR_INVALID
        assert b.os2r_rollout_policy_noisy(*[None, 0, None, 0, None, 0] + [None] * 10) == abi.ERR_INVALID
        assert b.os2r_last_error(None) == b"os2r_copy_envs: null destination handle"
        assert b.os2r_rollout_policy_scheduled(*[None, 0, None, 0, 0, 0, None, 0] + [None] * 10) == abi.ERR_INVALID
        assert b.os2r_last_error(None) == b"os2r_rollout_policy_scheduled: null handle"
    # the module's own shapes (tests/test_host_api.py and the test_*_host.py files pin the others)
    m = importlib.import_module("gym_os2r_amd._os2r_py")
    assert m.register_model_kernels(0, 0, 0, "nowhere.co") == abi.ERR_INVALID and "bad argument" in m.last_error(0)
    with pytest.raises(TypeError):
        m.register_model_kernels(0, 0, 0, None)
    assert m.get_step_count(0) == (abi.ERR_INVALID, 0) and m.get_violation_mirror(0) == (abi.ERR_INVALID, 0)
    assert m.bench_steps(0, 1, 0) == (abi.ERR_INVALID, 0.0) and m.bench_enqueue(0, 1, 0) == abi.ERR_INVALID
    assert m.bench_steps_multi([], [], 1) == abi.ERR_INVALID and m.bench_steps_multi([0], [], 1) == abi.ERR_INVALID
    assert m.linearize(0, 0, 1e-3, 1e-3, 1e-3, 0, 0, 0, 0) == abi.ERR_INVALID and "null handle" in m.last_error(0)
    assert m.set_step_count(0, 2 ** 64 - 1) == abi.ERR_INVALID
    with pytest.raises(TypeError):
        m.step(0, 0, 0, 0, 0, 0)               # six arguments for os2r_step's seven
    with pytest.raises(TypeError):
        m.step(None, 0, 0, 0, 0, 0, 0)         # an address is an integer
