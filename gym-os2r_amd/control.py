"""Loader of ``libos2r_control.so`` (include/os2r_control.h), the companion library of ``libos2r.so``: the backward pass of iLQR
on the device arrays linearize() writes and rollout_schedule() reads.

ctypes only: the pybind11 module exists for the per-step call overhead of ``os2r_step``; a backward pass is one call per
iteration.  HipSim.ilqr_backward uses this loader whichever binding drives ``libos2r.so``.  There is no fallback: if the
library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C

from . import abi
from ._lib import companion as _companion

ABI_VERSION = 1          # OS2R_CONTROL_ABI_VERSION
MAX_ALPHAS = 16          # OS2RC_MAX_ALPHAS
MAX_OBS = 12             # OS2R_MAX_OBS


class Os2rControlLayout(C.Structure):
    """What a call needs of a simulator handle: dtype, chain length, device ordinal and observation layout."""
    _fields_ = [("dtype", C.c_int32), ("nq", C.c_int32), ("device", C.c_int32), ("obs_dim", C.c_int32),
                ("slot_col", C.c_int32 * MAX_OBS)]


_vp, _i32, _f64p = C.c_void_p, C.c_int32, C.POINTER(C.c_double)

# Every entry point include/os2r_control.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_ilqr_backward_host.py holds it against the header).  The result is c_int, except for
# os2rc_last_error (c_char_p).
ENTRY_POINTS = {
    "os2rc_abi_version": (),
    "os2rc_last_error": (),
    "os2rc_ilqr_backward": (C.POINTER(Os2rControlLayout), _i32, C.c_int64, _vp, _vp, _vp, _vp, _f64p, _f64p, C.c_double, _vp, _vp,
                            _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f64p, _i32, _vp, _vp),
}


class Os2rControlLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_CONTROL_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_control", "os2rc", "OS2R_CONTROL_LIBRARY", Os2rControlLibraryMissing)


def slot_columns(task, nq):
    """The state column each observation slot of `task` (an Os2rTaskSpec) shows where the slot is raw -- a joint position
    (column src) or velocity (column nq + src) as it is --, -1 for every other slot: os2r_lqr_gains, step 6."""
    cols = []
    for d in range(int(task.obs_dim)):
        kind, src = task.obs_kind[d], task.obs_src[d]
        if kind in (abi.OBS_POS_RAW, abi.OBS_POS_PERIODIC_RAW):
            cols.append(int(src))
        elif kind == abi.OBS_VEL_RAW:
            cols.append(int(nq) + int(src))
        else:
            cols.append(-1)
    return cols


def layout(dtype, nq, device, cols=None):
    """An Os2rControlLayout: dtype abi.F32 / abi.F64, the device ordinal, cols = slot_columns(...) or None (no weight table)."""
    out = Os2rControlLayout(dtype=int(dtype), nq=int(nq), device=int(device), obs_dim=len(cols or ()))
    for d in range(MAX_OBS):
        out.slot_col[d] = cols[d] if cols and d < len(cols) else -1
    return out
