"""The math probe on the host: it compiles with the library's flags, and the exact-arithmetic restatements of `sincos_fast` and
of the series turn (tests/math_probe.py), which the GPU tests hold the device against bit for bit, are themselves measured
against mpmath at 200 bits on the seeded argument sets.

Yardstick.  The entries of a rotation matrix matter by their ABSOLUTE error.  A Cody-Waite reduction leaves a remainder with one
rounding at magnitude < 1; next to a multiple of pi/2 the result itself is tiny and its error in ulp OF THE RESULT is unbounded
(hundreds of ulp inside the fast range).  So the bound is absolute, in units of eps of the dtype, and the worst relative error
is printed with the argument where it occurs, not asserted.

  sincos_fast, |error| <= 1.0 eps: one rounding of the remainder at magnitude < 1 (<= 0.5 ulp(r) <= 2^-54 for |r| <= pi/4, which
  enters sin with slope <= 1), the polynomial's error < 1 ulp of a result <= 1 on [-pi/4, pi/4], and the residual of the reduction
  k |pi/2 - C1 - C2| < 2^-80 (fp32: three constants, < 2^-50).

  Teeth: the restatement without C2, and with the last hex digit of C1 changed, both trip the bound.  The last digit of a
  polynomial coefficient moves the result by less than half an eps: the bound cannot see it, the bit-for-bit comparison of the
  device with the restatement does (test_a_polynomial_digit_is_below_the_bound_but_changes_bits).

  series turn: measured here, recorded below with the sample size; asserted at 1.25 x the record (the margin covers a reseeded
  sample, nothing else).
"""
import math

import numpy as np
import pytest

import math_probe as mp_
from math_probe import EPS, sincos_fast_exact, turn_exact

mpmath = pytest.importorskip("mpmath")

# Worst |error| of the series turn against sin / cos of the exact angle q0 + m d (d the rounded increment dt * qd), in units of
# 2^-52, after m turns from sincos_fast(q0): measured with the restatement against mpmath at 200 bits on turn_arguments()
# (TURN_SAMPLE pairs, seed math_probe.SEED + 2).  {m: worst}
TURN_SAMPLE = 1506
MEASURED_TURN = {9: 1.592, 24: 2.571}
TURN_MARGIN = 1.25
SINCOS_BOUND = 1.0      # eps of the dtype, absolute (module docstring)


def _truth(x):
    with mpmath.workprec(200):
        v = mpmath.mpf(float(x))
        return mpmath.sin(v), mpmath.cos(v)


def _errors(dtype, xs, consts=None):
    """-> (worst absolute error in eps, worst relative error in eps and its argument) of the restatement on xs."""
    worst, worst_rel, at = 0.0, 0.0, None
    with mpmath.workprec(200):
        for x in xs:
            s, c = sincos_fast_exact(x, dtype, consts)
            ts, tc = _truth(x)
            for got, want in ((s, ts), (c, tc)):
                e = abs(mpmath.mpf(got) - want)
                worst = max(worst, float(e / EPS[dtype]))
                if want != 0 and float(e / abs(want) / EPS[dtype]) > worst_rel:
                    worst_rel, at = float(e / abs(want) / EPS[dtype]), float(x)
    return worst, worst_rel, at


def test_probe_cross_compiles_with_the_library_flags():
    """The probe builds for gfx950 with exactly jit.FLAGS (+ arch, -fPIC, -shared), and exports every entry point."""
    import subprocess
    path = mp_.build_probe()
    syms = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in mp_.ENTRY_POINTS:
        assert f" T {name}\n" in syms, name


def test_rounding_to_float32_is_single():
    """_rnd32 rounds a Fraction once: on a value that lies just above the middle of two floats but rounds to the middle in
    float64, the way through float64 gives the other neighbour."""
    from fractions import Fraction as F
    f = F(1) + F(2) ** -24 + F(2) ** -60          # above the tie between 1 and 1 + 2^-23
    assert mp_._rnd32(f) == 1.0 + 2.0 ** -23
    assert float(np.float32(float(f))) == 1.0     # double rounding: float64 drops 2^-60, the tie then goes to even
    rng = np.random.default_rng(3)
    for v in rng.standard_normal(200) * np.exp2(rng.integers(-140, 100, 200)):
        assert mp_._rnd32(F(float(v))) == float(np.float32(v)), v         # (a float64 to float32 is one rounding)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_sincos_fast_restatement_against_mpmath(dtype):
    xs = mp_.sincos_arguments(dtype)
    worst, worst_rel, at = _errors(dtype, xs)
    print(f"sincos_fast {dtype.__name__}, {len(xs)} arguments: worst absolute error {worst:.3f} eps; "
          f"worst relative error {worst_rel:.1f} eps at x = {at!r} (not asserted)")
    assert worst <= SINCOS_BOUND, worst


def _without_c2():
    k = dict(mp_.SC64)
    k["c"] = k["c"][:1]
    return k


def _digit(which, index, old, new):
    """One hex digit of one constant changed: `old` must be the constant's last hex digit."""
    k = {name: list(v) if isinstance(v, list) else v for name, v in mp_.SC64.items()}
    h = k[which][index].hex()
    m, e = h.split("p")
    assert m.endswith(old), h
    k[which][index] = float.fromhex(m[:-1] + new + "p" + e)
    return k


NEGATIVES = {
    "C2 dropped": _without_c2,
    # the last hex digit of the first reduction constant, 8 -> 9: one ulp of C1, times k
    "C1 last digit": lambda: _digit("c", 0, "8", "9"),
}


@pytest.mark.parametrize("what", list(NEGATIVES))
def test_the_bound_has_teeth(what):
    """A restatement of sincos_fast<double> with a defect of the size the bound is meant to see trips it."""
    xs = mp_.sincos_arguments(np.float64)
    xs = np.concatenate([xs[-400:], xs[:1200]])            # edges, random and far multiples: enough, in milliseconds each
    worst, _, _ = _errors(np.float64, xs, NEGATIVES[what]())
    print(f"{what}: worst absolute error {worst:.3f} eps")
    assert worst > SINCOS_BOUND, (what, worst)


def test_a_polynomial_digit_is_below_the_bound_but_changes_bits():
    """The last hex digit of the leading sine coefficient, 9 -> 1, moves the result by at most 2^-52 (pi/4)^3 = 0.48 eps: an
    absolute bound of 1.0 eps cannot see it everywhere (measured: worst 0.73 eps).  The bit-for-bit comparison of the device
    with the restatement (tests/test_gpu_math_probe.py) is what sees it: the restatement's own bits change."""
    xs = mp_.sincos_arguments(np.float64)[-400:]
    k = _digit("s", 5, "9", "1")
    changed = sum(sincos_fast_exact(x) != sincos_fast_exact(x, np.float64, k) for x in xs)
    print(f"S1 last digit: {changed} of {len(xs)} arguments change bits")
    assert changed > len(xs) // 10


def _turn_errors(ms):
    q0, qd, dt = mp_.turn_arguments()
    assert len(q0) == TURN_SAMPLE
    worst = {m: 0.0 for m in ms}
    with mpmath.workprec(200):
        for a, v in zip(q0, qd):
            d = float(np.float64(dt) * np.float64(v))
            s, c = sincos_fast_exact(a)
            for m in range(1, max(ms) + 1):
                s, c = turn_exact(s, c, d)
                if m in worst:
                    ang = mpmath.mpf(float(a)) + m * mpmath.mpf(d)
                    e = max(abs(mpmath.mpf(s) - mpmath.sin(ang)), abs(mpmath.mpf(c) - mpmath.cos(ang)))
                    worst[m] = max(worst[m], float(e / EPS[np.float64]))
    return worst


def test_series_turn_against_the_exact_angle():
    """m = 9 (substeps = 10) and m = 24 (substeps = 25) turns from sincos_fast(q0), against sin / cos of q0 + m d."""
    worst = _turn_errors(sorted(MEASURED_TURN))
    for m, w in worst.items():
        print(f"series turn, {TURN_SAMPLE} pairs, m = {m}: worst absolute error {w:.3f} eps (recorded {MEASURED_TURN[m]})")
    for m, w in worst.items():
        assert w <= TURN_MARGIN * MEASURED_TURN[m], (m, w)
    assert all(w > 0.5 for w in worst.values())          # (the turns do accumulate: the comparison is not vacuous)


def test_turn_of_zero_and_denormal_increment_is_the_identity():
    s0, c0 = sincos_fast_exact(1.0)
    assert turn_exact(s0, c0, 0.0) == (s0, c0)
    assert turn_exact(s0, c0, 5e-324) == (s0, c0)
    assert math.isclose(s0, math.sin(1.0), rel_tol=0, abs_tol=2 ** -52)
