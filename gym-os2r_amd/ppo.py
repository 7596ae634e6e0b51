"""Loader of ``libos2r_ppo.so`` (include/os2r_ppo.h), the companion library of ``libos2r.so`` for the clipped-surrogate (PPO)
gradient of the linear-Gaussian policy the rollout kernels evaluate: the gradient of many policies in one call, evaluated at new
weights on the stored batch of a noisy rollout_policy and the advantages of gae -- per lane the sums over the steps of its first
episode, per policy the sums over its valid lanes.

ctypes only, like gym_os2r_amd.pg, and with gym_os2r_amd.control's Os2rControlLayout and layout() as they are.
HipSim.ppo_gradient and HipSim.ppo_gradient_into use this loader whichever binding drives ``libos2r.so``.  There is no
fallback: if the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C

from ._lib import companion as _companion
from .control import MAX_OBS, Os2rControlLayout, layout  # noqa: F401  (re-exported)

ABI_VERSION = 1          # OS2R_PPO_ABI_VERSION
TANH = 1                 # OS2RO_TANH
SIGMA_PER_LANE = 2       # OS2RO_SIGMA_PER_LANE
CHUNKS = 64              # OS2RO_CHUNKS
LANE_COUNTS = 5          # OS2RO_LANE_COUNTS, the rows of lane_count_dev: len, clip_0, clip_1, gated, valid
STATS = 3                # OS2RO_STATS, the rows of stat_dev and lane_stat_dev: surr, dev, logr

_vp, _i32 = C.c_void_p, C.c_int32

# Every entry point include/os2r_ppo.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_ppo_host.py holds it against the header).  The result is c_int, except for os2ro_last_error
# (c_char_p).
ENTRY_POINTS = {
    "os2ro_abi_version": (),
    "os2ro_last_error": (),
    "os2ro_ppo_gradient": (C.POINTER(Os2rControlLayout), _i32, C.c_int64, _i32, C.c_uint32) + (_vp,) * 10 + (C.c_double,) + (_vp,) * 13,
}


class Os2rPpoLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_PPO_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_ppo", "os2ro", "OS2R_PPO_LIBRARY", Os2rPpoLibraryMissing)
