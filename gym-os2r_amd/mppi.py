"""Loader of ``libos2r_mppi.so`` (include/os2r_mppi.h), the companion library of ``libos2r.so`` for sampling planners: the MPPI
update of many robots in one launch -- the softmax weights of every robot's samples, the weighted mean of their action sequences,
the action to apply now, the shifted nominal and the bias entries of the per-environment table the next noisy
rollout_schedule reads.

ctypes only, like gym_os2r_amd.steer, and with gym_os2r_amd.control's Os2rControlLayout and layout() as they are.
HipSim.mppi_update and HipSim.mppi_update_into use this loader whichever binding drives ``libos2r.so``.  There is no fallback: if
the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C

from ._lib import companion as _companion
from .control import MAX_OBS, Os2rControlLayout, layout  # noqa: F401  (re-exported)

ABI_VERSION = 1          # OS2R_MPPI_ABI_VERSION
TAIL_ZERO = 1            # OS2RM_TAIL_ZERO
CHUNKS = 8               # OS2RM_CHUNKS
TAILS = {"hold": 0, "zero": TAIL_ZERO}

_vp, _i32 = C.c_void_p, C.c_int32

# Every entry point include/os2r_mppi.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_mppi_host.py holds it against the header).  The result is c_int, except for os2rm_last_error
# (c_char_p).
ENTRY_POINTS = {
    "os2rm_abi_version": (),
    "os2rm_last_error": (),
    "os2rm_mppi_update": (C.POINTER(Os2rControlLayout), _i32, C.c_int64, _i32, _vp, _vp, _vp, C.c_double, _i32, C.c_uint32, _vp, _vp,
                          _vp, _vp, _vp, _vp, _vp),
}


class Os2rMppiLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_MPPI_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_mppi", "os2rm", "OS2R_MPPI_LIBRARY", Os2rMppiLibraryMissing)
