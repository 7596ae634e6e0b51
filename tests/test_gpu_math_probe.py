"""The device math primitives of the step kernels, one by one, against high-precision references (needs an MI355X).

tests/probe/os2r_math_probe.hip calls each primitive of gym-os2r_amd/csrc/os2r_device.hpp, os2r_kernels.hpp and os2r_bits.hpp
on one argument per thread, compiled with the library's flags; tests/math_probe.py builds and loads it.  One launch per family
and dtype (module-scoped), every segment of a launch padded to whole workgroups of 256 so that a segment's waves hold that
segment's arguments only.

References: numpy.longdouble (64-bit mantissa, asserted) for fp64, float64 for fp32; for `sincos_fast` the exact-arithmetic
restatement of tests/math_probe.py, bit for bit.  Every test prints what it measured (pytest -s).

RECORDED values below: measured on an MI355X against those references with this file, 2026-10-21, with the ROCm whose
`hipcc --version` is ROCM below.  Each is asserted with the margin and for the reason stated beside it; none is taken
from a kernel's output as such.
"""
import math

import numpy as np
import pytest

import math_probe as mp_
from math_probe import EPS, GUARD

pytestmark = pytest.mark.gpu

ROCM = "HIP version: 7.2.26015-fc0010cf6a, AMD clang version 22.0.0git (roc-7.2.0)"
LD = np.longdouble
F64, F32 = np.float64, np.float32
IDS = {F64: "f64", F32: "f32"}
SUFFIX = {F64: "f64", F32: "f32"}
WG = 256

# sincos_lib (ROCm's sincos / sincosf) from the guard up to 1e15 / 1e7: worst absolute error in eps of the dtype.  Asserted at
# the record + 1 eps: it is ROCm's routine, the margin is for a ROCm update.
RECORDED_LIB = {F64: 0.385, F32: 0.582}
# rcp_t / rsqrt_t / sqrt_t: worst error in ulp of the correctly rounded result over every binade of the stated range.  Asserted
# at the record rounded up to the next quarter ulp + 0.25 ulp: the estimate instructions are deterministic, the margin is for
# the sample of mantissas only.
RECORDED_ULP = {("rcp_t", F64): 0.500, ("rsqrt_t", F64): 1.736, ("sqrt_t", F64): 0.500,
                ("rcp_t", F32): 0.500, ("rsqrt_t", F32): 1.523, ("sqrt_t", F32): 0.500}
SINCOS_BOUND = 1.0       # eps, absolute: derived in tests/test_math_probe_host.py
TANH_ULP = 4.0           # the bound the project already uses for tanh_t
NORMAL_EPS = 4.0         # eps * max(1, r): log, sqrt, cos / sin and two products, each about 1 ulp, with the angle <= 2 pi


def _quarter_up(v):
    return math.ceil(v * 4.0) / 4.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert np.finfo(LD).nmant >= 63, "numpy.longdouble is not the x87 extended format here"
    mp_.load_probe()


class Batch:
    """The arguments of one launch: named segments, each padded to whole workgroups."""

    def __init__(self, dtype, fill=1.0):
        self.dtype, self.fill, self.parts, self.where, self.n = dtype, fill, [], {}, 0

    def add(self, name, x):
        x = np.asarray(x, dtype=self.dtype)
        pad = (-len(x)) % WG
        self.where[name] = slice(self.n, self.n + len(x))
        self.parts += [x, np.full(pad, self.fill, dtype=self.dtype)]
        self.n += len(x) + pad

    def run(self, entry, rows):
        self.x = np.concatenate(self.parts)
        assert self.n == len(self.x) <= 2 ** 20
        self.out = mp_.run(entry, self.x, rows)
        return self

    def arg(self, name):
        return self.x[self.where[name]]

    def get(self, name):
        return self.out[:, self.where[name]]


def _same(a, b):
    """Bit for bit, +0 and -0 as one value (the library is built with -fno-signed-zeros); no NaN on either side."""
    a, b = np.asarray(a), np.asarray(b)
    assert not np.isnan(a).any() and not np.isnan(b).any()
    return a == b


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}")


def _three_ways(x, rng, first_half_is):
    """x (its first half one kind of argument, its second half the other) as it is -- every wave of one kind --, interleaved --
    every wave of both kinds --, and permuted -> (arrangements, index arrays that bring each back to the order of x)."""
    n = len(x)
    assert n % (2 * WG) == 0 and first_half_is(x[: n // 2]).all() and not first_half_is(x[n // 2:]).any()
    inter = np.arange(n).reshape(2, n // 2).T.ravel()
    perm = rng.permutation(n)
    orders = [np.arange(n), inter, perm]
    for o in orders[:2]:
        kinds = first_half_is(x[o]).reshape(-1, 64)
        mixed = kinds.any(axis=1) & ~kinds.all(axis=1)
        assert mixed.all() if o is inter else not mixed.any()
    return [x[o] for o in orders], [np.argsort(o) for o in orders]


# ---------------------------------------------------------------------------------------
# 1, 2. sin / cos
# ---------------------------------------------------------------------------------------
def _sweep(dtype, n, rng):
    g = GUARD[dtype]
    log = np.exp2(rng.uniform(-30.0, math.log2(g), n // 2)) * rng.choice([-1.0, 1.0], n // 2)
    x = np.concatenate([log, rng.uniform(-g, g, n - n // 2)]).astype(dtype)
    x[np.abs(x) >= dtype(g)] = dtype(1.0)
    return x


def _guard_arguments(dtype):
    g = dtype(GUARD[dtype])
    below = [g]
    for _ in range(4):
        below.append(np.nextafter(below[-1], dtype(0)))
    above = [g]
    for _ in range(4):
        above.append(np.nextafter(above[-1], dtype(np.inf)))
    x = np.array(below[1:] + above + [g * dtype(0.999), g * dtype(1.001)], dtype=dtype)
    return np.concatenate([x, -x])


def _company_arguments(dtype, rng):
    g, top = GUARD[dtype], {F64: 1e15, F32: 1e7}[dtype]
    inside = rng.uniform(-g, g, 2048).astype(dtype)
    inside[np.abs(inside) >= dtype(g)] = dtype(0.5)
    outside = (np.exp2(rng.uniform(math.log2(g) + 1e-3, math.log2(top), 2048)) * rng.choice([-1.0, 1.0], 2048)).astype(dtype)
    return np.concatenate([inside, outside])


@pytest.fixture(scope="module", params=[F64, F32], ids=lambda d: IDS[d])
def sincos(request):
    dtype = request.param
    rng = np.random.default_rng(mp_.SEED + 10)
    b = Batch(dtype)
    b.add("set", mp_.sincos_arguments(dtype))
    b.add("sweep", _sweep(dtype, 2 ** 20 - 2 ** 16 - 3 * 4096 - 16384, rng))
    b.add("guard", _guard_arguments(dtype))
    top = {F64: 1e15, F32: 1e7}[dtype]
    b.add("lib", (np.exp2(rng.uniform(math.log2(GUARD[dtype]), math.log2(top), 2 ** 16 - WG))
                  * rng.choice([-1.0, 1.0], 2 ** 16 - WG)).astype(dtype))
    ways, back = _three_ways(_company_arguments(dtype, rng), rng, lambda v: np.abs(v) < dtype(GUARD[dtype]))
    for k, w in enumerate(ways):
        b.add(f"company{k}", w)
    b.back = back
    return b.run(f"probe_sincos_{SUFFIX[dtype]}", 6)


def _reference(x):
    wide = LD if x.dtype == F64 else F64
    xx = x.astype(wide)
    return np.sin(xx), np.cos(xx)


def _abs_err_eps(got_s, got_c, x):
    s, c = _reference(x)
    e = np.maximum(np.abs(got_s.astype(s.dtype) - s), np.abs(got_c.astype(c.dtype) - c)) / EPS[x.dtype.type]
    k = int(np.argmax(e))
    return float(e[k]), x[k]


def test_sincos_fast_equals_the_restatement_bit_for_bit(sincos):
    """IEEE FMA and multiply in a fixed order: the device and the exact-arithmetic restatement agree in every bit on the
    committed argument set (multiples of pi/2 and their neighbours, the guard's last argument, 0, denormals)."""
    dtype = sincos.dtype
    x, out = sincos.arg("set"), sincos.get("set")
    want = np.array([mp_.sincos_fast_exact(v, dtype) for v in x], dtype=dtype).T
    ok = _same(out[0], want[0]) & _same(out[1], want[1])
    print(f"sincos_fast {IDS[dtype]}: {len(x)} arguments, {int((~ok).sum())} differ from the restatement")
    assert ok.all(), [(float(v), out[0][i], want[0][i], out[1][i], want[1][i]) for i, v in enumerate(x) if not ok[i]][:5]


def test_sincos_fast_dense_sweep(sincos):
    """|error| <= 1.0 eps on the dense sweep (log-spaced from 2^-30 to the guard, and uniform, both signs)."""
    x, out = sincos.arg("sweep"), sincos.get("sweep")
    worst, at = _abs_err_eps(out[0], out[1], x)
    print(f"sincos_fast {IDS[sincos.dtype]}: {len(x)} arguments, worst absolute error {worst:.3f} eps at x = {at!r}")
    assert worst <= SINCOS_BOUND, (worst, at)


def test_guard_selects_fast_below_and_lib_from_it_on(sincos):
    dtype = sincos.dtype
    for seg in ("guard", "set", "lib"):
        x, out = sincos.arg(seg), sincos.get(seg)
        inside = np.abs(x) < dtype(GUARD[dtype])
        fast = _same(out[4], out[0]) & _same(out[5], out[1])
        lib = _same(out[4], out[2]) & _same(out[5], out[3])
        assert fast[inside].all() and lib[~inside].all(), seg
        if seg == "guard":
            assert inside.sum() == 10 and (~inside).sum() == 12
        else:
            # the two routines do differ on these arguments (inside: in the last bit here and there; beyond the guard the two-constant
            # reduction is no longer exact), or the selection would show nothing
            assert (~(fast & lib)).any(), seg


def test_sincos_lib_beyond_the_guard(sincos):
    dtype = sincos.dtype
    x, out = sincos.arg("lib"), sincos.get("lib")
    worst, at = _abs_err_eps(out[2], out[3], x)
    print(f"sincos_lib {IDS[dtype]}: {len(x)} arguments from the guard to {np.abs(x).max():.3g}, worst absolute error {worst:.3f} eps "
          f"at x = {at!r} (recorded {RECORDED_LIB[dtype]})")
    assert RECORDED_LIB[dtype] is not None and worst <= RECORDED_LIB[dtype] + 1.0, (worst, at)


def test_sincos_selection_does_not_depend_on_company(sincos):
    """The same 4 096 arguments with every wave on one side of the guard, with both sides in every wave, and permuted."""
    base = sincos.get("company0")
    for k in (1, 2):
        again = sincos.get(f"company{k}")[:, sincos.back[k]]
        assert np.array_equal(_bits(base), _bits(again)), k


# ---------------------------------------------------------------------------------------
# 3. reciprocal, reciprocal square root, square root
# ---------------------------------------------------------------------------------------
RANGE = {F64: 100, F32: 60}


def _recip_arguments(dtype, rng):
    e = np.arange(-RANGE[dtype], RANGE[dtype] + 1)
    x = (np.exp2(e.astype(np.float64))[:, None] * rng.uniform(1.0, 2.0, (len(e), 4096))).astype(dtype)
    x[x >= np.exp2(e + 1.0)[:, None].astype(dtype)] = dtype(1.5)          # (a mantissa rounded up into the next binade in fp32)
    p = np.exp2(e.astype(np.float64)).astype(dtype)
    edges = np.concatenate([p, np.nextafter(p, dtype(0)), np.nextafter(p, dtype(np.inf))])
    x = np.concatenate([x.ravel(), edges])
    return x * rng.choice([-1.0, 1.0], len(x)).astype(dtype)


def _outside(dtype):
    f = np.finfo(dtype)
    return np.array([0.0, f.smallest_subnormal, f.tiny / 4, f.tiny, 2.0 ** (f.maxexp - 1), f.max, 2.0 ** (f.maxexp - 2) * 1.5],
                    dtype=dtype)


@pytest.fixture(scope="module", params=[F64, F32], ids=lambda d: IDS[d])
def recip(request):
    dtype = request.param
    b = Batch(dtype)
    b.add("range", _recip_arguments(dtype, np.random.default_rng(mp_.SEED + 20)))
    b.add("outside", np.concatenate([_outside(dtype), -_outside(dtype)]))
    return b.run(f"probe_recip_{SUFFIX[dtype]}", 5)


@pytest.mark.parametrize("fn", ["rcp_t", "rsqrt_t", "sqrt_t"])
def test_reciprocals_in_ulp_of_the_result(recip, fn):
    dtype = recip.dtype
    wide = LD if dtype == F64 else F64
    x, out = recip.arg("range"), recip.get("range")
    xx = x.astype(wide)
    truth, got = {"rcp_t": (1 / xx, out[0]), "rsqrt_t": (1 / np.sqrt(np.abs(xx)), out[3]), "sqrt_t": (np.sqrt(np.abs(xx)), out[4])}[fn]
    ulp = np.spacing(np.abs(truth.astype(dtype))).astype(wide)           # of the correctly rounded result
    err = np.abs(got.astype(wide) - truth) / ulp
    k = int(np.argmax(err))
    rec = RECORDED_ULP[(fn, dtype)]
    print(f"{fn} {IDS[dtype]}: {len(x)} arguments in 2^+-{RANGE[dtype]}, worst error {float(err[k]):.4f} ulp at x = {x[k]!r} "
          f"(recorded {rec}); {int((got != truth.astype(dtype)).sum())} not correctly rounded")
    assert np.isfinite(got).all()
    assert rec is not None and float(err[k]) <= _quarter_up(rec) + 0.25, (fn, float(err[k]), x[k])


def test_rcp_group_equals_rcp_t_bit_for_bit(recip):
    """Slot i mod N of rcp_group<N> holds argument i next to its neighbours: every argument, in and outside the range."""
    out = recip.out
    bits = _bits(out)
    assert np.array_equal(bits[1], bits[0]) and np.array_equal(bits[2], bits[0])


def test_reciprocals_outside_their_domain_return(recip):
    """Zero, denormal arguments, reciprocals that are denormal: what comes back is printed, nothing is asserted about it."""
    x, out = recip.arg("outside"), recip.get("outside")
    for i, v in enumerate(x):
        print(f"{IDS[recip.dtype]} x = {v!r}: rcp_t {out[0][i]!r}, rsqrt_t(|x|) {out[3][i]!r}, sqrt_t(|x|) {out[4][i]!r}")
    assert out.shape[1] == len(x)


# ---------------------------------------------------------------------------------------
# 4. tanh_t
# ---------------------------------------------------------------------------------------
def _tanh_company(rng):
    small = rng.uniform(-0.55, 0.55, 2048)
    small[np.abs(small) >= 0.55] = 0.1
    large = rng.uniform(0.55, 30.0, 2048) * rng.choice([-1.0, 1.0], 2048)
    return np.concatenate([small, large])


@pytest.fixture(scope="module")
def tanh64():
    rng = np.random.default_rng(mp_.SEED + 30)
    b = Batch(F64, fill=0.25)
    half = np.concatenate([rng.uniform(0.0, 40.0, 2 ** 19 - 8 * 4096), np.exp2(np.arange(-1000.0, 11.0)),
                           [np.nextafter(0.55, 0.0), 0.55, np.nextafter(0.55, 1.0), 20.0, 354.0, 355.0, np.finfo(F64).max, 0.0]])
    b.add("pos", half)
    b.add("neg", -half)
    ways, back = _three_ways(_tanh_company(rng), rng, lambda v: np.abs(v) < 0.55)
    for k, w in enumerate(ways):
        b.add(f"company{k}", w)
    b.back = back
    return b.run("probe_tanh_f64", 1)


def test_tanh_within_4_ulp(tanh64):
    for seg in ("pos", "neg"):
        x, got = tanh64.arg(seg), tanh64.get(seg)[0]
        truth = np.tanh(x.astype(LD))
        err = np.abs(got.astype(LD) - truth) / np.spacing(np.abs(truth.astype(F64))).astype(LD)
        k = int(np.argmax(err))
        print(f"tanh_t f64 ({seg}): {len(x)} arguments, worst error {float(err[k]):.3f} ulp at x = {x[k]!r}")
        assert np.isfinite(got).all() and float(err[k]) <= TANH_ULP, (float(err[k]), x[k])


def test_tanh_is_odd_monotone_across_the_switch_and_saturates(tanh64):
    x, pos, neg = tanh64.arg("pos"), tanh64.get("pos")[0], tanh64.get("neg")[0]
    assert _same(neg, -pos).all()
    i = int(np.flatnonzero(x == 0.55)[0])
    assert x[i - 1] < 0.55 < x[i + 1] and pos[i - 1] <= pos[i] <= pos[i + 1], pos[i - 1:i + 2]
    assert (pos[x >= 20.0] == 1.0).all() and (neg[x >= 20.0] == -1.0).all() and (x >= 20.0).sum() > 1000
    assert (np.abs(pos[x < 20.0]) <= 1.0).all()


def test_tanh_does_not_depend_on_company(tanh64):
    """The two wave-level skips: a wave of arguments below 0.55, a wave above, a mixed wave give every lane the same bits."""
    base = tanh64.get("company0")
    for k in (1, 2):
        assert np.array_equal(_bits(base), _bits(tanh64.get(f"company{k}")[:, tanh64.back[k]])), k


def test_tanh_f32_is_the_library_routine_within_4_ulp():
    rng = np.random.default_rng(mp_.SEED + 31)
    x = np.concatenate([rng.uniform(-12.0, 12.0, 2 ** 16 - 64), np.exp2(np.arange(-60.0, 4.0))]).astype(F32)
    got = mp_.run("probe_tanh_f32", x, 1)[0]
    truth = np.tanh(x.astype(F64))
    err = np.abs(got.astype(F64) - truth) / np.spacing(np.abs(truth.astype(F32))).astype(F64)
    print(f"tanh_t f32: {len(x)} arguments, worst error {err.max():.3f} ulp at x = {x[int(np.argmax(err))]!r}")
    assert err.max() <= TANH_ULP


# ---------------------------------------------------------------------------------------
# 5. wrap_pi
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=lambda d: IDS[d])
def test_wrap_pi_is_numpy_mod_bit_for_bit(dtype):
    rng = np.random.default_rng(mp_.SEED + 40)
    pi, up, dn = dtype(np.pi), dtype(np.inf), dtype(-np.inf)
    two_pi = dtype(2) * pi
    f = np.finfo(dtype)
    near_pi = [pi, np.nextafter(pi, up), np.nextafter(pi, dn), -pi, np.nextafter(-pi, up), np.nextafter(-pi, dn)]
    k = np.unique(np.concatenate([np.arange(1, 65), rng.integers(65, int(1e6 / (2 * np.pi)), 1000)]))
    mult = (k.astype(dtype) * two_pi).astype(dtype)
    mult = np.concatenate([mult, np.nextafter(mult, up), np.nextafter(mult, dn), mult + pi, mult - pi])
    x = np.concatenate([near_pi, mult, -mult, [0.0, -0.0, 1e15, -1e15, 3e5, -3e5],
                        [-f.smallest_subnormal, -f.tiny / 2, -f.tiny, f.smallest_subnormal, f.tiny],
                        rng.uniform(-50.0, 50.0, 4096), rng.uniform(-1e6, 1e6, 4096)]).astype(dtype)
    want = np.mod(x + pi, two_pi) - pi
    assert want.dtype == dtype
    got = mp_.run(f"probe_wrap_{SUFFIX[dtype]}", x, 1)[0]
    ok = _same(got, want)
    print(f"wrap_pi {IDS[dtype]}: {len(x)} arguments, {int((~ok).sum())} differ from numpy.mod(x + pi, 2 pi) - pi")
    assert ok.all(), [(x[i], got[i], want[i]) for i in np.flatnonzero(~ok)[:5]]
    # a negative remainder, however small, is brought up by 2 pi: m + 2 pi rounds to 2 pi, the result is +pi (numpy's too)
    m = np.fmod(x + pi, two_pi)
    tiny = (m < 0) & (m + two_pi == two_pi)
    assert (want[tiny] == two_pi - pi).all()
    assert (got >= -pi).all() and (got <= pi).all()


# ---------------------------------------------------------------------------------------
# 6. class tests on bit patterns
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=lambda d: IDS[d])
def test_class_tests_on_bit_patterns(dtype):
    """Every class test on zeros, denormals, the ends of the normal range, infinities, quiet and signalling NaNs with varied
    payloads, negative NaNs, and random words.  The arguments travel as integers; the expected bytes come from the bits."""
    u = np.uint64 if dtype == F64 else np.uint32
    nbits, nman = (64, 52) if dtype == F64 else (32, 23)
    one = u(1)
    sign, exp_all = one << u(nbits - 1), ((one << u(nbits - 1 - nman)) - one) << u(nman)
    mag_mask, quiet = sign - one, one << u(nman - 1)
    rng = np.random.default_rng(mp_.SEED + 50)
    payloads = [one, u(2), u(0x1234), quiet - one, (quiet >> one) | one] + [u(v) for v in rng.integers(1, int(quiet), 64)]
    pos = [u(0), one, (one << u(nman)) - one,                      # zero, smallest and largest denormal
           one << u(nman), exp_all - one,                          # smallest and largest normal
           exp_all,                                                # infinity
           exp_all | quiet]                                        # the default quiet NaN
    pos += [exp_all | quiet | p for p in payloads]                 # quiet NaNs with payloads
    pos += [exp_all | p for p in payloads]                         # signalling NaNs
    pos = np.array(pos, dtype=u)
    bits = np.concatenate([pos, pos | sign, rng.integers(0, 2 ** nbits, 4096, dtype=np.uint64).astype(u)])
    mag = bits & mag_mask
    finite = (bits & exp_all) != exp_all
    nan = mag > exp_all
    invalid = ~finite | (((bits & sign) != 0) & (mag != 0))
    want = np.stack([finite, finite, finite, nan, invalid]).astype(np.uint8)
    cls, got_mag = mp_.run_class(dtype, bits)
    names = ["finite_t", "hi_finite", "steer_finite", "steer_nan", "steer_invalid"]
    wrong = {}
    for r, name in enumerate(names):
        bad = np.flatnonzero(cls[r] != want[r])
        print(f"{name} {IDS[dtype]}: {len(bits)} patterns, {len(bad)} wrong" + "".join(f" {int(bits[i]):#x}" for i in bad[:4]))
        if len(bad):
            wrong[name] = len(bad)
    assert not wrong, wrong
    assert np.array_equal(got_mag, mag), "steer_abs"
    assert nan.sum() > 200 and (~finite & ~nan).sum() == 2 and (finite & invalid).sum() > 1000


# ---------------------------------------------------------------------------------------
# 7. normal2 / uniform2
# ---------------------------------------------------------------------------------------
def philox(c, k):
    """Philox4x32-10 on uint64 arrays c [4, n], k [2, n] holding 32-bit words (tests/test_oracle_rng.py's statement, vectorised;
    held against it below)."""
    M0, M1, W0, W1, lo = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (c[i].astype(np.uint64) for i in range(4))
    k0, k1 = k[0].astype(np.uint64), k[1].astype(np.uint64)
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> s) ^ c1 ^ k0) & lo, p1 & lo, ((p0 >> s) ^ c3 ^ k1) & lo, p0 & lo
        k0, k1 = (k0 + W0) & lo, (k1 + W1) & lo
    return np.stack([c0, c1, c2, c3])


def _u53(a, b):
    return ((a >> np.uint64(5)).astype(F64) * 67108864.0 + (b >> np.uint64(6)).astype(F64)) / 9007199254740992.0


def _box_muller(u0, u1):
    """normal2 restated in longdouble: the angle is the double constant 2 pi times u1, the product not rounded."""
    r = np.sqrt(-2 * np.log(1 - u0.astype(LD)))
    th = LD(6.283185307179586476925286766559) * u1.astype(LD)
    return r, r * np.cos(th), r * np.sin(th)


def test_normal2_against_longdouble():
    from test_oracle_rng import KAT, _philox_py
    for ctr, key, want in KAT:
        got = philox(np.array(ctr, dtype=np.uint64)[:, None], np.array(key, dtype=np.uint64)[:, None])[:, 0]
        assert [int(v) for v in got] == want == _philox_py(ctr, key)
    rng = np.random.default_rng(mp_.SEED + 60)
    n = 2 ** 16
    tup = rng.integers(0, 2 ** 32, (6, n), dtype=np.uint64)
    tup[3] = rng.integers(1, 7, n)                                   # the streams of the specification
    tup[2, :8] = [0, 1, 2 ** 32 - 1, 5, 0, 0, 7, 2 ** 31]
    tup[4, :8] = [0, 0, 2 ** 32 - 1, 0, 2 ** 32 - 1, 150, 3, 0]
    o = philox(tup[2:6], tup[0:2])                                   # counter (env, stream, ctr, blk), key (seed lo, seed hi)
    u0, u1 = _u53(o[0], o[1]), _u53(o[2], o[3])
    out = mp_.run("probe_normal", tup.astype(np.uint32), 4, out_dtype=F64)
    assert np.array_equal(out[2], u0) and np.array_equal(out[3], u1)
    r, z0, z1 = _box_muller(u0, u1)
    scale = EPS[F64] * np.maximum(1.0, r)
    err = np.maximum(np.abs(out[0].astype(LD) - z0), np.abs(out[1].astype(LD) - z1)) / scale
    k = int(np.argmax(err))
    print(f"normal2: {n} tuples, worst absolute error {float(err[k]):.3f} eps max(1, r) at u0 = {u0[k]!r}, u1 = {u1[k]!r}; "
          f"u0 in [{u0.min():.3g}, {u0.max():.12f}], max r {float(r.max()):.3f}")
    assert np.isfinite(out).all() and float(err[k]) <= NORMAL_EPS, float(err[k])
    # the word path (u53 and the Box-Muller lines of normal2, on given words) gives normal2's bits on these tuples: what it
    # shows below on crafted words is what normal2 does with them
    words = mp_.run("probe_words", o.astype(np.uint32), 5, out_dtype=F64)
    assert np.array_equal(words[0], u0) and np.array_equal(words[1], u1)
    assert np.array_equal(_bits(words[3]), _bits(out[0])) and np.array_equal(_bits(words[4]), _bits(out[1]))


def test_normal2_at_the_extremes_of_u0():
    """u53 on crafted words: u0 = 0 (every word pair whose upper 27 and 26 bits are clear) gives r = 0 exactly, u0 = 1 - 2^-53
    the largest radius; u1 at its extremes and at the quarter turns.  Everything finite, within the bound."""
    full = 0xFFFFFFFF
    u1_words = [(0, 0), (full, full), (1 << 30, 0), (1 << 31, 0), (3 << 30, 0), (0x12345678, 0x9ABCDEF0), (31, 63), (32, 0), (0, 64)]
    rows = [(a, b, c, d) for a, b in [(0, 0), (31, 63), (17, 5), (full, full), (32, 0), (0, 64), (full, full - 63), (1 << 31, 0)]
            for c, d in u1_words]
    w = np.array(rows, dtype=np.uint64).T
    u0, u1 = _u53(w[0], w[1]), _u53(w[2], w[3])
    assert (u0[: 3 * len(u1_words)] == 0.0).all() and u0.max() == 1.0 - 2.0 ** -53 and u1.max() == 1.0 - 2.0 ** -53
    out = mp_.run("probe_words", w.astype(np.uint32), 5, out_dtype=F64)
    assert np.array_equal(out[0], u0) and np.array_equal(out[1], u1)
    assert np.isfinite(out).all()
    zero = u0 == 0.0
    assert (out[2][zero] == 0.0).all() and (out[3][zero] == 0.0).all() and (out[4][zero] == 0.0).all()
    r, z0, z1 = _box_muller(u0, u1)
    scale = EPS[F64] * np.maximum(1.0, r)
    err = np.maximum(np.abs(out[3].astype(LD) - z0), np.abs(out[4].astype(LD) - z1)) / scale
    print(f"normal2 at the extremes: max r {out[2].max()!r} (sqrt(106 log 2) = {math.sqrt(106 * math.log(2))!r}), "
          f"worst absolute error {float(err.max()):.3f} eps max(1, r)")
    assert abs(out[2].max() - math.sqrt(106 * math.log(2))) <= 4 * np.spacing(out[2].max())
    assert float(err.max()) <= NORMAL_EPS
