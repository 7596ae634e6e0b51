"""Loader of ``libos2r_norm.so`` (include/os2r_norm.h), the companion library of ``libos2r.so`` for running observation whitening
of the linear policy the rollout kernels evaluate: the running mean and deviation of every observation component of many
policies, merged batch by batch on the device (os2rz_obs_stats); the fold of a policy given in whitened coordinates into weights
on raw observations (os2rz_fold); and the gradient back through the fold (os2rz_unfold).  The policy is linear, so no rollout
kernel changes.

ctypes only, like gym_os2r_amd.es, and with gym_os2r_amd.control's Os2rControlLayout and layout() as they are.
HipSim.obs_stats, HipSim.norm_fold, HipSim.norm_unfold and their ``_into`` forms use this loader whichever binding drives
``libos2r.so``.  There is no fallback: if the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C

from ._lib import companion as _companion
from .control import MAX_OBS, Os2rControlLayout, layout  # noqa: F401  (re-exported)

ABI_VERSION = 1                  # OS2R_NORM_ABI_VERSION
PER_LANE = 1                     # OS2RZ_PER_LANE
POLICY_FASTEST = 2               # OS2RZ_POLICY_FASTEST
CHUNKS = 64                      # OS2RZ_CHUNKS
LANE_COUNTS = 2                  # OS2RZ_LANE_COUNTS: the rows of lane_count (len, valid)

_vp, _i32, _u32, _i64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_int64

# Every entry point include/os2r_norm.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_norm_host.py holds it against the header).  The result is c_int, except for os2rz_last_error (c_char_p).
ENTRY_POINTS = {
    "os2rz_abi_version": (),
    "os2rz_last_error": (),
    "os2rz_obs_stats": (C.POINTER(Os2rControlLayout), _i32, _i64, _i32, _u32) + (_vp,) * 14,
    "os2rz_fold": (C.POINTER(Os2rControlLayout), _i64, _i64, _i32, _u32, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp),
    "os2rz_unfold": (C.POINTER(Os2rControlLayout), _i64, _i32, _u32, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp),
}


class Os2rNormLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_NORM_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_norm", "os2rz", "OS2R_NORM_LIBRARY", Os2rNormLibraryMissing)
