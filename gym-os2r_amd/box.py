"""Loader of ``libos2r_box.so`` (include/os2r_box.h), the companion library of ``libos2r.so``, ``libos2r_control.so`` and
``libos2r_steer.so`` for the backward pass of iLQR under box limits on the two actions: the feed-forward step is the exact
solution of the knot's box-constrained QP, the feedback rows of the clamped components are zero, and the value recursion sees
both (control-limited DDP), in one launch.

ctypes only, like gym_os2r_amd.steer, and with gym_os2r_amd.control's Os2rControlLayout, layout() and slot_columns() as they are.
HipSim.ilqr_backward(box=...) uses this loader whichever binding drives ``libos2r.so``.  There is no fallback: if the library has
not been built (``make -C gym-os2r_amd/csrc``), load() raises.
"""
from __future__ import annotations

import ctypes as C
import math

from ._lib import companion as _companion
from .control import MAX_ALPHAS, MAX_OBS, Os2rControlLayout, layout, slot_columns  # noqa: F401  (re-exported)

ABI_VERSION = 1          # OS2R_BOX_ABI_VERSION
# the clamp byte of a knot (include/os2r_box.h, B4): bit c: component c is held at a bound; bit 2 + c: at its upper one
CLAMPED_0, CLAMPED_1, UPPER_0, UPPER_1 = 1, 2, 4, 8
DEFAULT_BOX = (-1.0, 1.0)

_vp, _i32, _f64p = C.c_void_p, C.c_int32, C.POINTER(C.c_double)

# Every entry point include/os2r_box.h declares, in the header's order, with its ctypes argument types: the library's one
# declaration (tests/test_ilqr_box_host.py holds it against the header).  The result is c_int, except for os2rb_last_error
# (c_char_p).
ENTRY_POINTS = {
    "os2rb_abi_version": (),
    "os2rb_last_error": (),
    "os2rb_ilqr_backward_box": (C.POINTER(Os2rControlLayout), _i32, C.c_int64, _vp, _vp, _vp, _vp, _f64p, _f64p, C.c_double, _vp,
                                _f64p, _f64p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f64p, _i32, _vp, _vp),
}


class Os2rBoxLibraryMissing(ImportError):
    pass


# the library through ctypes, loaded once; OS2R_BOX_LIBRARY: A/B builds of the same ABI
LIB_PATH, load = _companion(globals(), "os2r_box", "os2rb", "OS2R_BOX_LIBRARY", Os2rBoxLibraryMissing)


def bounds(box, what="ilqr_backward"):
    """`box` of ilqr_backward -> (lo, hi), two ctypes double[2], checked as the library checks them (ValueError).  True: the
    default (-1, 1) on both components; else a pair (lo, hi), each a number for both components or a pair of numbers.  lo is
    -inf (no bound) or finite in [-1, 1], hi +inf or finite in [-1, 1], lo < hi."""
    if box is True:
        box = DEFAULT_BOX
    if isinstance(box, (bool, str)) or not hasattr(box, "__len__") or len(box) != 2:
        raise ValueError(f"{what}: box must be True or a pair (lo, hi), got {box!r}")
    sides = []
    for name, side in zip(("lo", "hi"), box):
        if hasattr(side, "tolist"):
            side = side.tolist()
        pair = list(side) if isinstance(side, (list, tuple)) else [side, side]
        try:
            pair = [float(v) for v in pair]
        except (TypeError, ValueError):
            raise ValueError(f"{what}: box {name} must be a number or a pair of numbers, got {side!r}") from None
        if len(pair) != 2:
            raise ValueError(f"{what}: box {name} must be a number or a pair of numbers, got {side!r}")
        sides.append(pair)
    lo, hi = sides
    for c in range(2):
        if math.isnan(lo[c]) or math.isnan(hi[c]):
            raise ValueError(f"{what}: a box bound must not be NaN, got lo {lo} hi {hi}")
        if lo[c] == math.inf or hi[c] == -math.inf:
            raise ValueError(f"{what}: box lo must be -inf or finite and hi +inf or finite, got lo {lo} hi {hi}")
        if any(math.isfinite(v) and not -1.0 <= v <= 1.0 for v in (lo[c], hi[c])):
            raise ValueError(f"{what}: a finite box bound must lie in [-1, 1], got lo {lo} hi {hi}")
        if not lo[c] < hi[c]:
            raise ValueError(f"{what}: box lo must be < hi in both components, got lo {lo} hi {hi}")
    return (C.c_double * 2)(*lo), (C.c_double * 2)(*hi)
