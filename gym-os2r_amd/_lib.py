"""Loader of the C-ABI shared library ``libos2r.so`` (HIP kernels for gfx950).

There is no CPU fallback: if the library has not been built (``python -c 'import
__graft_entry__ as g; g.build()'`` or ``make -C gym-os2r_amd/csrc``) importing the
device path raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OS2R_LIBRARY") or os.path.join(_HERE, "libos2r.so")   # OS2R_LIBRARY: A/B builds of the same ABI
_lib = None

_vp, _i32 = C.c_void_p, C.c_int32
_cfg, _model, _f64p = C.POINTER(abi.Os2rConfig), C.POINTER(abi.Os2rModel), C.POINTER(C.c_double)

# Every entry point include/os2r.h declares, in the header's order, with its ctypes argument types: the one declaration both
# bindings are made from (load() below; _PybindLib; tests/test_bindings_host.py holds it against the header).  The result is
# c_int, except for os2r_last_error (c_char_p).
ENTRY_POINTS = {
    "os2r_abi_version": (),
    "os2r_abi_minor": (),
    "os2r_create": (_cfg, C.POINTER(_vp)),
    "os2r_destroy": (_vp,),
    "os2r_reset": (_vp,) * 4,
    "os2r_step": (_vp,) * 7,
    "os2r_rollout": (_vp, C.c_int) + (_vp,) * 7,
    "os2r_rollout_policy": (_vp, C.c_int, _vp, _i32) + (_vp,) * 8,
    "os2r_rollout_policy_noisy": (_vp, C.c_int, _vp, _i32, _vp, C.c_uint32) + (_vp,) * 10,
    "os2r_rollout_policy_scheduled": (_vp, C.c_int, _vp, _i32, _i32, _i32, _vp, C.c_uint32) + (_vp,) * 10,
    "os2r_model_is_compiled_in": (_model,),
    "os2r_register_model_kernels": (_model, _i32, _i32, C.c_char_p),
    "os2r_get_action_violations": (_vp, _vp, _i32, _vp),
    "os2r_get_violation_mirror": (_vp, C.POINTER(_vp)),
    "os2r_get_state": (_vp,) * 4,
    "os2r_set_state": (_vp,) * 4,
    "os2r_get_solver_state": (_vp,) * 4,
    "os2r_set_solver_state": (_vp,) * 4,
    "os2r_get_action_history": (_vp, C.c_int, _vp, _vp),
    "os2r_set_action_history": (_vp, C.c_int, _vp, _vp),
    "os2r_set_params": (_vp, C.c_int, _vp, _vp),
    "os2r_get_params": (_vp, C.c_int, _vp, _vp),
    "os2r_get_episode_info": (_vp,) * 5,
    "os2r_set_episode_info": (_vp,) * 5,
    "os2r_copy_envs": (_vp, _vp, _vp, _i32, _vp, _vp),
    "os2r_linearize": (_vp, _vp, _f64p, _vp, _vp, _vp, _vp),
    "os2r_lqr_gains": (_vp, _i32, C.c_int64, _i32, _vp, _vp, _f64p, _f64p) + (_vp,) * 8,
    "os2r_get_step_count": (_vp, C.POINTER(C.c_uint64)),
    "os2r_set_step_count": (_vp, C.c_uint64),
    "os2r_bench_steps": (_vp, C.c_int, _vp, C.POINTER(C.c_float)),
    "os2r_bench_steps_multi": (C.POINTER(_vp), C.POINTER(_vp), C.c_int, C.c_int),
    "os2r_set_work_counters": (_vp, _vp),
    "os2r_set_done_reasons": (_vp, _vp),
    "os2r_set_done_mask": (_vp, _vp),
    "os2r_last_error": (_vp,),
}
SYMBOLS = list(ENTRY_POINTS)


# The companion library libos2r_record.so (include/os2r_record.h): built from the same objects, working on the same handles.  A
# table of its own: libos2r.so's symbol table is ENTRY_POINTS and nothing else.
RECORD_LIB_PATH = os.environ.get("OS2R_RECORD_LIBRARY") or os.path.join(_HERE, "libos2r_record.so")
RECORD_ENTRY_POINTS = {
    "os2rr_rollout_policy_recorded": (_vp, _vp, _i32, _i32, _vp, C.c_int, _vp, _i32, _i32, _i32, _vp, C.c_uint32) + (_vp,) * 10,
    "os2rr_last_error": (),
    "os2rr_abi_version": (),
}
RECORD_ABI_VERSION = 1
_record = None


class Os2rLibraryMissing(ImportError):
    pass


class Os2rError(RuntimeError):
    """A call of one of the libraries returned a status that is not OK (gym_os2r_amd.sim re-exports it)."""


def _ptr(t):
    """A tensor (or None) as the pointer argument of a C call."""
    return None if t is None else C.c_void_p(t.data_ptr())


def load_library(path, entry_points, last_error, version, missing, build_hint, mismatch):
    """One C-ABI library through ctypes: argument and result types from its table of entry points (the result is c_int, c_char_p
    for `last_error`), the ABI number `version` = (symbol, expected) checked.  A file that is not there raises
    missing(f"{path} not found: {build_hint}"), another ABI ImportError(mismatch).  The loaders keep what this returns."""
    if not os.path.exists(path):
        raise missing(f"{path} not found: {build_hint}")
    # torch first: the library needs libamdhip64, and the process must hold ONE HIP runtime -- the one torch brings.  Loaded before
    # torch (e.g. build() and smoke() of __graft_entry__ in one process) the library pulls in the system's runtime, torch then
    # its own, and os2r_create sees no device through the first ("no HIP device visible").
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for name, argtypes in entry_points.items():
        fn = getattr(lib, name)  # AttributeError here means header and library disagree
        fn.argtypes = list(argtypes)
        fn.restype = C.c_char_p if name == last_error else C.c_int
    symbol, expected = version
    if getattr(lib, symbol)() != expected:
        raise ImportError(mismatch)
    return lib


def companion(scope, name, prefix, env_var, missing):
    """(LIB_PATH, load) of the loader module whose globals() are `scope`, for the companion library lib`name`.so whose symbols start
    with `prefix`: the path is `env_var` or next to this file; load(), at its first call, reads the module's LIB_PATH, ENTRY_POINTS
    and ABI_VERSION and keeps the library as the module's _lib."""
    def load():
        if scope.get("_lib") is None:
            scope["_lib"] = load_library(scope["LIB_PATH"], scope["ENTRY_POINTS"], f"{prefix}_last_error",
                                         (f"{prefix}_abi_version", scope["ABI_VERSION"]), missing,
                                         "build the HIP extension first (make -C gym-os2r_amd/csrc). There is no CPU fallback.",
                                         f"lib{name}.so ABI version does not match {scope['__name__']}")
        return scope["_lib"]
    return os.environ.get(env_var) or os.path.join(_HERE, f"lib{name}.so"), load


def load_record():
    """libos2r_record.so through ctypes (after libos2r.so, and so after torch: one HIP runtime per process)."""
    global _record
    if _record is None:
        load()
        _record = load_library(RECORD_LIB_PATH, RECORD_ENTRY_POINTS, "os2rr_last_error", ("os2rr_abi_version", RECORD_ABI_VERSION),
                               Os2rLibraryMissing, "it is built with libos2r.so (make -C gym-os2r_amd/csrc); without it no rollout can "
                               "record its knots", "libos2r_record.so ABI version does not match gym_os2r_amd._lib")
    return _record


def load():
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, ENTRY_POINTS, "os2r_last_error", ("os2r_abi_version", abi.ABI_VERSION), Os2rLibraryMissing,
                            "build the HIP extension first (make -C gym-os2r_amd/csrc). The stepper has no CPU fallback.",
                            "libos2r.so ABI version does not match gym_os2r_amd.abi")
    return _lib


def _a(x):
    """What a pointer parameter is given, as the address the pybind11 module takes: None, an int, a c_void_p, a byref(...),
    a ctypes array or a ctypes scalar."""
    if x is None:
        return 0
    if type(x) is C.c_void_p:
        return x.value or 0
    if isinstance(x, int):
        return x
    return C.addressof(getattr(x, "_obj", x))      # byref(v) keeps v as ._obj


def _s(x):
    return x.decode() if isinstance(x, bytes) else x


def _converter(argtype):
    if argtype is C.c_char_p:
        return _s
    return _a if issubclass(argtype, (C.c_void_p, C._Pointer)) else int


def _forward(name, argtypes, prefix="os2r_"):
    """`def os2r_x(self, a0, a1, ...): return self.m.x(_a(a0), int(a1), ...)`: the method of one entry point as it would be
    written by hand, the converter of every argument fixed here.  (Made from source, not as a closure over a tuple of
    converters: a loop over the arguments in every call cost a third more on os2r_step, and this one checks the arity.)"""
    args = [f"a{i}" for i in range(len(argtypes))]
    converted = ", ".join(f"{_converter(t).__name__}({a})" for t, a in zip(argtypes, args))
    scope = {"_a": _a, "_s": _s, "__name__": __name__}
    exec(f"def {name}(self, {', '.join(args)}): return self.m.{name[len(prefix):]}({converted})", scope)
    scope[name].__qualname__ = f"_PybindLib.{name}"
    return scope[name]


class _PybindLib:
    """Adapter giving the pybind11 module (`_os2r_py`) the call shapes of the ctypes library, so that gym_os2r_amd.sim is
    binding-agnostic.  Selected with OS2R_BINDING=pybind11.  Every method is made from its row of ENTRY_POINTS (below the
    class), with one converter per argument fixed there; written out are only the calls whose shape in the module differs
    from the C one."""

    def __init__(self):
        import importlib
        self.m = importlib.import_module("gym_os2r_amd._os2r_py")
        if self.m.abi_version() != abi.ABI_VERSION:
            raise ImportError("_os2r_py ABI version mismatch")

    @staticmethod
    def _result(out_ref, rc, value):
        """The module returns (status, value) where the C call writes through a pointer."""
        if out_ref is not None:
            out_ref._obj.value = value
        return rc

    def os2r_create(self, cfg_ref, out_ref):
        return self._result(out_ref, *self.m.create(_a(cfg_ref)))

    def os2r_get_step_count(self, h, out_ref):
        return self._result(out_ref, *self.m.get_step_count(_a(h)))

    def os2r_get_violation_mirror(self, h, out_ref):
        return self._result(out_ref, *self.m.get_violation_mirror(_a(h)))

    def os2r_bench_steps(self, h, n, st, ms_ref):
        if ms_ref is None:
            return self.m.bench_enqueue(_a(h), int(n), _a(st))
        return self._result(ms_ref, *self.m.bench_steps(_a(h), int(n), _a(st)))

    def os2r_bench_steps_multi(self, sims, streams, count, nsteps):
        n = range(int(count))                      # two arrays of c_void_p: an element reads as an int, or None for null
        return self.m.bench_steps_multi([sims[i] or 0 for i in n], [streams[i] or 0 for i in n], int(nsteps))

    def os2r_linearize(self, h, act, eps, nxt, ja, jb, st):
        e = (0.0, 0.0, 0.0) if eps is None else eps      # the module takes three doubles: it has no null eps (0 is refused too)
        return self.m.linearize(_a(h), _a(act), float(e[0]), float(e[1]), float(e[2]), _a(nxt), _a(ja), _a(jb), _a(st))

    def os2r_last_error(self, h):
        return self.m.last_error(_a(h)).encode()

    # libos2r_record.so: the module links it too
    def os2rr_last_error(self):
        return self.m.record_last_error().encode()


for _name, _argtypes in ENTRY_POINTS.items():
    if _name not in vars(_PybindLib):
        setattr(_PybindLib, _name, _forward(_name, _argtypes))
setattr(_PybindLib, "os2rr_rollout_policy_recorded",
        _forward("os2rr_rollout_policy_recorded", RECORD_ENTRY_POINTS["os2rr_rollout_policy_recorded"], prefix="os2rr_"))
