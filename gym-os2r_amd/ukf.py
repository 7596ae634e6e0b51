"""Loader of ``libos2r_ukf.so`` (include/os2r_ukf.h), the companion library of ``libos2r.so`` for the unscented Kalman filter of
many robots: the sigma points of (x, P) in the layout set_state() takes, and the launch that turns what get_state() returns for
the propagated points back into (x, P), updates both against a measured observation and writes the next sigma points.

ctypes only, like gym_os2r_amd.ekf, and with gym_os2r_amd.control's Os2rControlLayout and layout() as they are.
HipSim.ukf_points, ukf_update and their ``*_into`` use this loader whichever binding drives ``libos2r.so``.  There is no
fallback: if the library has not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C
import math

from ._lib import companion as _companion
from .control import MAX_OBS, Os2rControlLayout, layout  # noqa: F401  (re-exported)

ABI_VERSION = 1          # OS2R_UKF_ABI_VERSION

_vp = C.c_void_p
_dbl = C.c_double

# Every entry point include/os2r_ukf.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_ukf_host.py holds it against the header).  The result is c_int, except for os2ru_last_error
# (c_char_p).
ENTRY_POINTS = {
    "os2ru_abi_version": (),
    "os2ru_last_error": (),
    "os2ru_ukf_points": (C.POINTER(Os2rControlLayout), C.c_int64, _vp, _vp, _dbl, _vp, _vp, _vp),
    "os2ru_ukf_update": (C.POINTER(Os2rControlLayout), C.c_int64, _vp, _vp, _vp, _vp, C.POINTER(C.c_double), _dbl, _dbl, _dbl, _dbl, _vp,
                         _vp, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
}


class Os2rUkfLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_UKF_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_ukf", "os2ru", "OS2R_UKF_LIBRARY", Os2rUkfLibraryMissing)


def npoints(nq):
    """The sigma points of one robot with nq joints: 2n + 1 with n = 2nq states."""
    return 4 * int(nq) + 1


def weights(n, alpha=1.0, beta=2.0, kappa=0.0):
    """The scalars of the scaled unscented transform for n states, in float64 -> (gamma, wm0, wc0, wi):
    lambda = alpha^2 (n + kappa) - n, gamma = sqrt(n + lambda), wm0 = lambda / (n + lambda), wc0 = wm0 + 1 - alpha^2 + beta,
    wi = 1 / (2 (n + lambda)).  ValueError unless n + lambda > 0 and all four are finite.
    The defaults give wm0 = 0 (and gamma = sqrt(n), wc0 = 2, wi = 1 / 2n).  They are chosen for fp32: the customary
    alpha = 1e-3 makes wm0 about -1e6 and the mean wm0 chi_0 + wi sum chi_s the small difference of two numbers a million times
    its size, which cancels catastrophically in fp32."""
    try:
        n, alpha, beta, kappa = int(n), float(alpha), float(beta), float(kappa)
    except (TypeError, ValueError):
        raise ValueError("ukf weights: n, alpha, beta and kappa must be numbers") from None
    if n < 1:
        raise ValueError(f"ukf weights: n must be >= 1, got {n}")
    if not all(math.isfinite(v) for v in (alpha, beta, kappa)):
        raise ValueError(f"ukf weights: alpha, beta and kappa must be finite, got {alpha}, {beta}, {kappa}")
    lam = alpha * alpha * (n + kappa) - n
    scale = n + lam
    if not scale > 0.0:
        raise ValueError(f"ukf weights: n + lambda must be > 0, got {scale} (alpha {alpha}, kappa {kappa})")
    try:
        out = (math.sqrt(scale), lam / scale, lam / scale + 1.0 - alpha * alpha + beta, 1.0 / (2.0 * scale))
    except (OverflowError, ZeroDivisionError):
        raise ValueError(f"ukf weights: not finite with alpha {alpha}, beta {beta}, kappa {kappa}") from None
    if not all(math.isfinite(v) for v in out):
        raise ValueError(f"ukf weights: not finite with alpha {alpha}, beta {beta}, kappa {kappa}: {out}")
    return out
