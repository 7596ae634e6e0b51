"""Loader of ``libos2r_cem.so`` (include/os2r_cem.h), the companion library of ``libos2r.so`` for the cross-entropy method: the
update of many robots in one call -- the best E of every robot's lanes, the mean and the width of the sampling distribution
refitted from them, the action to apply now, the shifted nominal, and the bias entries of the per-environment table and the
per-lane sigma the next noisy rollout_schedule reads.

ctypes only, like gym_os2r_amd.mppi, and with gym_os2r_amd.control's Os2rControlLayout and layout() as they are.
HipSim.cem_update and HipSim.cem_update_into use this loader whichever binding drives ``libos2r.so``.  There is no fallback: if
the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C

from ._lib import companion as _companion
from .control import MAX_OBS, Os2rControlLayout, layout  # noqa: F401  (re-exported)

ABI_VERSION = 1          # OS2R_CEM_ABI_VERSION
TAIL_ZERO = 1            # OS2RX_TAIL_ZERO
CHUNKS = 8               # OS2RX_CHUNKS
TAILS = {"hold": 0, "zero": TAIL_ZERO}

_vp, _i32, _f64 = C.c_void_p, C.c_int32, C.c_double

# Every entry point include/os2r_cem.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_cem_host.py holds it against the header).  The result is c_int, except for os2rx_last_error
# (c_char_p).
ENTRY_POINTS = {
    "os2rx_abi_version": (),
    "os2rx_last_error": (),
    "os2rx_cem_update": (C.POINTER(Os2rControlLayout), _i32, C.c_int64, _i32, _i32, _vp, _vp, _vp, _vp, _f64, _f64, _f64, _f64, _i32,
                         C.c_uint32) + (_vp,) * 10,
}


class Os2rCemLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_CEM_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_cem", "os2rx", "OS2R_CEM_LIBRARY", Os2rCemLibraryMissing)
