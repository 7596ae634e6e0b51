"""Loader of ``libos2r_cma.so`` (include/os2r_cma.h), the companion library of ``libos2r.so`` for CMA-ES of many populations of
the linear policy the rollout kernels evaluate: before a rollout the Cholesky factor of every population's covariance and its
correlated samples, after it the rank-mu / rank-one / path update of mean, step size, covariance and both evolution paths from
one return per lane.  The normals are a pure function of (seed, population, sample, generation) under the stepper's counter RNG;
the update regenerates the bits the sample call used.  ``constants`` has Hansen's default scalars.

ctypes only, like gym_os2r_amd.es, and with gym_os2r_amd.control's Os2rControlLayout and layout() as they are.
HipSim.cma_init, HipSim.cma_sample, HipSim.cma_update and their ``_into`` forms use this loader whichever binding drives
``libos2r.so``.  There is no fallback: if the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C
import math

from ._lib import companion as _companion
from .control import MAX_OBS, Os2rControlLayout, layout  # noqa: F401  (re-exported)

ABI_VERSION = 1                  # OS2R_CMA_ABI_VERSION
STREAM = 7                       # OS2RK_STREAM: the stream of the counter RNG the normals are drawn from
CHUNKS = 64                      # OS2RK_CHUNKS
MAX_SAMPLES = 2 ** 27 - 1        # OS2RK_MAX_SAMPLES

CONSTANT_NAMES = ("a_sigma", "b_sigma", "hsig_bound", "a_c", "b_c", "k0_moving", "k0_stalled", "c_1", "c_mu", "g_sigma", "chi",
                  "sigma_min", "sigma_max")


class Os2rkCmaConstants(C.Structure):
    """The scalars of os2rk_cma_update (include/os2r_cma.h), doubles on the host in the header's order."""
    _fields_ = [(name, C.c_double) for name in CONSTANT_NAMES]


_vp, _i32, _u32 = C.c_void_p, C.c_int32, C.c_uint32

# Every entry point include/os2r_cma.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_cma_host.py holds it against the header).  The result is c_int, except for os2rk_last_error (c_char_p).
ENTRY_POINTS = {
    "os2rk_abi_version": (),
    "os2rk_last_error": (),
    "os2rk_cma_sample": (C.POINTER(Os2rControlLayout), C.c_int64, _i32, _u32, C.c_uint64, _u32, _u32) + (_vp,) * 8,
    "os2rk_cma_update": (C.POINTER(Os2rControlLayout), C.c_int64, _i32, _i32, _u32, C.c_uint64, _u32, _u32) + (_vp,) * 9
                        + (C.POINTER(Os2rkCmaConstants),) + (_vp,) * 12,
}


class Os2rCmaLibraryMissing(ImportError):
    pass


def constants(E: int, S: int, parents=None, age: int = 0, sigma_min: float = 1e-8, sigma_max: float = 1.0):
    """Hansen's default constants of a population of S samples in E dimensions, in Python floats: -> (rankw, constants), the mu
    recombination weights (a list, rank 0 first, summing to 1) and the Os2rkCmaConstants of os2rk_cma_update.  parents = mu
    (None: S // 2); age is the number of updates already made, it enters hsig_bound only."""
    mu = S // 2 if parents is None else parents
    if not 1 <= mu <= S:
        raise ValueError(f"cma.constants: parents must be in 1..{S}, got {mu}")
    raw = [math.log(mu + 0.5) - math.log(r + 1) for r in range(mu)]
    total = math.fsum(raw)
    rankw = [w / total for w in raw]
    mu_eff = 1.0 / math.fsum(w * w for w in rankw)
    c_sigma = (mu_eff + 2.0) / (E + mu_eff + 5.0)
    d_sigma = 1.0 + 2.0 * max(0.0, math.sqrt((mu_eff - 1.0) / (E + 1.0)) - 1.0) + c_sigma
    c_c = (4.0 + mu_eff / E) / (E + 4.0 + 2.0 * mu_eff / E)
    c_1 = 2.0 / ((E + 1.3) ** 2 + mu_eff)
    c_mu = min(1.0 - c_1, 2.0 * (mu_eff - 2.0 + 1.0 / mu_eff) / ((E + 2.0) ** 2 + mu_eff))
    chi = math.sqrt(E) * (1.0 - 1.0 / (4.0 * E) + 1.0 / (21.0 * E * E))
    k0_moving = 1.0 - c_1 - c_mu
    k = Os2rkCmaConstants(
        a_sigma=1.0 - c_sigma, b_sigma=math.sqrt(c_sigma * (2.0 - c_sigma) * mu_eff),
        hsig_bound=(1.4 + 2.0 / (E + 1.0)) * chi * math.sqrt(1.0 - (1.0 - c_sigma) ** (2 * (age + 1))),
        a_c=1.0 - c_c, b_c=math.sqrt(c_c * (2.0 - c_c) * mu_eff),
        k0_moving=k0_moving, k0_stalled=k0_moving + c_1 * c_c * (2.0 - c_c), c_1=c_1, c_mu=c_mu,
        g_sigma=c_sigma / d_sigma, chi=chi, sigma_min=float(sigma_min), sigma_max=float(sigma_max))
    return rankw, k


# the library through ctypes, loaded once; OS2R_CMA_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_cma", "os2rk", "OS2R_CMA_LIBRARY", Os2rCmaLibraryMissing)
