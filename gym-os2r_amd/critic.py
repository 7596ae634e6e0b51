"""Loader of ``libos2r_critic.so`` (include/os2r_critic.h), the companion library of ``libos2r.so`` for the critic of an
actor-critic iteration of many linear-Gaussian policies: a linear value function per policy, the generalised advantage estimate
of every step of every lane under it (os2rv_gae) and the ridge least-squares refit of its weights on the batch
(os2rv_value_fit), on the device arrays a rollout_policy returned.

ctypes only, like gym_os2r_amd.pg, and with gym_os2r_amd.control's Os2rControlLayout and layout() as they are.  HipSim.gae,
HipSim.gae_into, HipSim.value_fit and HipSim.value_fit_into use this loader whichever binding drives ``libos2r.so``.  There is no
fallback: if the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C

from ._lib import companion as _companion
from .control import MAX_OBS, Os2rControlLayout, layout  # noqa: F401  (re-exported)

ABI_VERSION = 1          # OS2R_CRITIC_ABI_VERSION
CHUNKS = 64              # OS2RV_CHUNKS
LANE_COUNTS = 2          # OS2RV_LANE_COUNTS, the rows of lane_count_dev: len, valid


def moments(obs_dim: int) -> int:
    """E: the entries of lane_mom_dev and mom_dev -- the upper triangle of the (D+1) x (D+1) moment matrix, then the D+1 of b."""
    n = int(obs_dim) + 1
    return n * (n + 1) // 2 + n


_vp, _i32 = C.c_void_p, C.c_int32

# Every entry point include/os2r_critic.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_critic_host.py holds it against the header).  The result is c_int, except for os2rv_last_error
# (c_char_p).
_SHAPE = (C.POINTER(Os2rControlLayout), _i32, C.c_int64, _i32)
ENTRY_POINTS = {
    "os2rv_abi_version": (),
    "os2rv_last_error": (),
    "os2rv_gae": _SHAPE + (_vp,) * 7 + (C.c_double, C.c_double) + (_vp,) * 4,
    "os2rv_value_fit": _SHAPE + (_vp,) * 5 + (C.c_double,) + (_vp,) * 8,
}


class Os2rCriticLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_CRITIC_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_critic", "os2rv", "OS2R_CRITIC_LIBRARY", Os2rCriticLibraryMissing)
