"""Loader of ``libos2r_pf.so`` (include/os2r_pf.h), the companion library of ``libos2r.so`` for state estimation: the
particle-filter update of many robots in one launch -- the weights of every robot's particles against a measurement, the weighted
estimate, the effective sample size and, where a robot resamples, the systematic-resampling index that copy_envs_from takes.

ctypes only, like gym_os2r_amd.mppi, and with gym_os2r_amd.control's Os2rControlLayout and layout() as they are.
HipSim.pf_update and HipSim.pf_update_into use this loader whichever binding drives ``libos2r.so``.  There is no fallback: if
the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C

from ._lib import companion as _companion
from .control import MAX_OBS, Os2rControlLayout, layout  # noqa: F401  (re-exported)

ABI_VERSION = 1          # OS2R_PF_ABI_VERSION
CHUNKS = 8               # OS2RP_CHUNKS

_vp, _i32 = C.c_void_p, C.c_int32

# Every entry point include/os2r_pf.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_pf_host.py holds it against the header).  The result is c_int, except for os2rp_last_error
# (c_char_p).
ENTRY_POINTS = {
    "os2rp_abi_version": (),
    "os2rp_last_error": (),
    "os2rp_pf_update": (C.POINTER(Os2rControlLayout), C.c_int64, _i32, _vp, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp,
                        _vp, _vp),
}


class Os2rPfLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_PF_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_pf", "os2rp", "OS2R_PF_LIBRARY", Os2rPfLibraryMissing)
