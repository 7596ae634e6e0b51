"""Loader of ``libos2r_pg.so`` (include/os2r_pg.h), the companion library of ``libos2r.so`` for the score-function policy gradient
of the linear-Gaussian policy the rollout kernels evaluate: the gradient of many policies in one call, on the device arrays a
noisy rollout_policy returned -- per lane the sums over the steps of its first episode, per policy the sums over its valid lanes.

ctypes only, like gym_os2r_amd.mppi, and with gym_os2r_amd.control's Os2rControlLayout and layout() as they are.
HipSim.policy_gradient and HipSim.policy_gradient_into use this loader whichever binding drives ``libos2r.so``.  There is no
fallback: if the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C

from ._lib import companion as _companion
from .control import MAX_OBS, Os2rControlLayout, layout  # noqa: F401  (re-exported)

ABI_VERSION = 1          # OS2R_PG_ABI_VERSION
TANH = 1                 # OS2RG_TANH
SIGMA_PER_LANE = 2       # OS2RG_SIGMA_PER_LANE
CHUNKS = 64              # OS2RG_CHUNKS
LANE_COUNTS = 4          # the rows of lane_count_dev: len, clip_0, clip_1, valid

_vp, _i32 = C.c_void_p, C.c_int32

# Every entry point include/os2r_pg.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_pg_host.py holds it against the header).  The result is c_int, except for os2rg_last_error
# (c_char_p).
ENTRY_POINTS = {
    "os2rg_abi_version": (),
    "os2rg_last_error": (),
    "os2rg_policy_gradient": (C.POINTER(Os2rControlLayout), _i32, C.c_int64, _i32, C.c_uint32) + (_vp,) * 9 + (C.c_double,) + (_vp,) * 11,
}


class Os2rPgLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_PG_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_pg", "os2rg", "OS2R_PG_LIBRARY", Os2rPgLibraryMissing)
