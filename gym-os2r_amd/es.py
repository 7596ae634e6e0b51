"""Loader of ``libos2r_es.so`` (include/os2r_es.h), the companion library of ``libos2r.so`` for evolution-strategy search of the
linear policy the rollout kernels evaluate: before a rollout the antithetic perturbations theta +- nu delta of many policies along
S directions each, after it the ARS V1-t update of every policy from one return per lane.  The directions are a pure function of
(seed, population, direction, generation) under the stepper's counter RNG; the update regenerates the bits the perturbation
added.

ctypes only, like gym_os2r_amd.npg, and with gym_os2r_amd.control's Os2rControlLayout and layout() as they are.
HipSim.es_perturb, HipSim.es_update and their ``_into`` forms use this loader whichever binding drives ``libos2r.so``.  There is no
fallback: if the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C

from ._lib import companion as _companion
from .control import MAX_OBS, Os2rControlLayout, layout  # noqa: F401  (re-exported)

ABI_VERSION = 1                  # OS2R_ES_ABI_VERSION
STREAM = 6                       # OS2RA_STREAM: the stream of the counter RNG the directions are drawn from
CHUNKS = 64                      # OS2RA_CHUNKS
MAX_DIRECTIONS = 2 ** 27 - 1     # OS2RA_MAX_DIRECTIONS

_vp, _i32, _u32 = C.c_void_p, C.c_int32, C.c_uint32

# Every entry point include/os2r_es.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_es_host.py holds it against the header).  The result is c_int, except for os2ra_last_error (c_char_p).
ENTRY_POINTS = {
    "os2ra_abi_version": (),
    "os2ra_last_error": (),
    "os2ra_es_perturb": (C.POINTER(Os2rControlLayout), C.c_int64, _i32, _u32, C.c_uint64, _u32, _u32, _vp, C.c_double, _vp, _vp, _vp),
    "os2ra_es_update": (C.POINTER(Os2rControlLayout), C.c_int64, _i32, _i32, _u32, C.c_uint64, _u32, _u32, _vp, _vp, C.c_double, C.c_double)
                       + (_vp,) * 8,
}


class Os2rEsLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_ES_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_es", "os2ra", "OS2R_ES_LIBRARY", Os2rEsLibraryMissing)
