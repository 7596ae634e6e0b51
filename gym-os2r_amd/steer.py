"""Loader of ``libos2r_steer.so`` (include/os2r_steer.h), the companion library of ``libos2r.so``, ``libos2r_control.so`` and
``libos2r_search.so`` for an iLQR iteration that no host value steers: the backward pass with one regularisation mu per
trajectory, and the line search that also applies an Armijo test, moves every trajectory's mu, and freezes what has converged
or stalled, in one launch.

ctypes only, like gym_os2r_amd.search, and with gym_os2r_amd.control's Os2rControlLayout, layout() and slot_columns() as they are.
HipSim.ilqr_backward(mu_dev=...) and HipSim.ilqr_steer use this loader whichever binding drives ``libos2r.so``.  There is no
fallback: if the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C

from ._lib import companion as _companion
from .control import MAX_ALPHAS, MAX_OBS, Os2rControlLayout, layout, slot_columns  # noqa: F401  (re-exported)

ABI_VERSION = 1          # OS2R_STEER_ABI_VERSION
ACTIVE, CONVERGED, STALLED = 0, 1, 2   # OS2RT_ACTIVE, OS2RT_CONVERGED, OS2RT_STALLED


class Os2rSteerRule(C.Structure):
    """How os2rt_ilqr_steer judges a step and moves mu (include/os2r_steer.h)."""
    _fields_ = [("armijo", C.c_double), ("shrink", C.c_double), ("grow", C.c_double), ("mu_floor", C.c_double),
                ("mu_start", C.c_double), ("mu_max", C.c_double), ("tol", C.c_double)]


# the rule of examples/ilqr_balancing.py: mu halved after an accepted step and dropped to 0 below 1e-3, ten times larger (0.1 at
# least) after a rejected iteration, no Armijo test, nothing ever converged
RULE_DEFAULTS = dict(armijo=0.0, shrink=0.5, grow=10.0, mu_floor=1e-3, mu_start=0.1, mu_max=1e6, tol=0.0)

_vp, _i32, _f64p = C.c_void_p, C.c_int32, C.POINTER(C.c_double)

# Every entry point include/os2r_steer.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_ilqr_steer_host.py holds it against the header).  The result is c_int, except for os2rt_last_error
# (c_char_p).
ENTRY_POINTS = {
    "os2rt_abi_version": (),
    "os2rt_last_error": (),
    "os2rt_ilqr_backward_mu": (C.POINTER(Os2rControlLayout), _i32, C.c_int64, _vp, _vp, _vp, _vp, _f64p, _f64p, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f64p, _i32, _vp, _vp),
    "os2rt_ilqr_steer": (C.POINTER(Os2rControlLayout), _i32, C.c_int64, _i32, _vp, _vp, _vp, _vp, _vp, _f64p, _f64p, _f64p,
                         _vp, _f64p, C.POINTER(Os2rSteerRule), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
}


class Os2rSteerLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_STEER_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_steer", "os2rt", "OS2R_STEER_LIBRARY", Os2rSteerLibraryMissing)


def rule(rule=None, **kw):
    """An Os2rSteerRule from a dict and / or keywords over RULE_DEFAULTS, checked as the library checks it (ValueError)."""
    import math
    given = dict(rule or {}, **kw)
    unknown = sorted(set(given) - set(RULE_DEFAULTS))
    if unknown:
        raise ValueError(f"ilqr_steer: unknown rule members {unknown} (known: {sorted(RULE_DEFAULTS)})")
    try:
        v = {k: float(given.get(k, d)) for k, d in RULE_DEFAULTS.items()}
    except (TypeError, ValueError):
        raise ValueError(f"ilqr_steer: every rule member must be a number, got {given}") from None
    if not all(math.isfinite(x) for x in v.values()):
        raise ValueError(f"ilqr_steer: every rule member must be finite, got {v}")
    if not (v["armijo"] >= 0 and 0 <= v["shrink"] <= 1 and v["grow"] >= 1 and v["mu_floor"] >= 0 and v["mu_start"] > 0
            and v["mu_max"] >= v["mu_start"] and v["tol"] >= 0):
        raise ValueError(f"ilqr_steer: the rule needs armijo >= 0, 0 <= shrink <= 1, grow >= 1, mu_floor >= 0, mu_start > 0, "
                         f"mu_max >= mu_start and tol >= 0, got {v}")
    return Os2rSteerRule(**v)
