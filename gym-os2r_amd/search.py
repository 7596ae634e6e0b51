"""Loader of ``libos2r_search.so`` (include/os2r_search.h), the companion library of ``libos2r.so`` and ``libos2r_control.so``
for the forward-pass evaluation of iLQR: the cost of every line-search candidate, one accepted step size per trajectory and the
nominal updated in place, in one launch.

ctypes only, like gym_os2r_amd.control, whose Os2rControlLayout, layout() and slot_columns() it takes as they are: a line
search is one call per iteration.  HipSim.ilqr_line_search uses this loader whichever binding drives ``libos2r.so``.  There is
no fallback: if the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C

from ._lib import companion as _companion
from .control import MAX_ALPHAS, MAX_OBS, Os2rControlLayout, layout, slot_columns  # noqa: F401  (re-exported)

ABI_VERSION = 1          # OS2R_SEARCH_ABI_VERSION
ACCEPT_ALWAYS = 1        # OS2RS_ACCEPT_ALWAYS

_vp, _i32, _f64p = C.c_void_p, C.c_int32, C.POINTER(C.c_double)

# Every entry point include/os2r_search.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_ilqr_line_search_host.py holds it against the header).  The result is c_int, except for
# os2rs_last_error (c_char_p).
ENTRY_POINTS = {
    "os2rs_abi_version": (),
    "os2rs_last_error": (),
    "os2rs_ilqr_line_search": (C.POINTER(Os2rControlLayout), _i32, C.c_int64, _i32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _f64p, _f64p, _f64p,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
}


class Os2rSearchLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_SEARCH_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_search", "os2rs", "OS2R_SEARCH_LIBRARY", Os2rSearchLibraryMissing)
