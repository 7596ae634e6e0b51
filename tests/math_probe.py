"""The math probe (tests/probe/os2r_math_probe.hip): its build and loader, the exact-arithmetic restatements of the
primitives it exposes, and the seeded argument sets the host and the GPU tests share.  Test infrastructure only.

Restatements.  `sincos_fast_exact` and `turn_exact` perform the operations of `sincos_fast` and of the series turn of
`substep` step 1 (gym-os2r_amd/csrc/os2r_device.hpp) in the order written there, every product, sum and FMA evaluated in
`fractions.Fraction` and rounded ONCE to the format (`rnd`): float64 through Python's correctly rounded int / int, float32
by rounding the Fraction to 24 bits directly (through float64 it would be rounded twice).
"""
import ctypes as C
import hashlib
import math
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

from conftest import KERNEL_CACHE, ROOT

PROBE_SRC = os.path.join(ROOT, "tests", "probe", "os2r_math_probe.hip")
GUARD = {np.float64: 8.2e5, np.float32: 200.0}           # sincos_in_range: |x| < GUARD
TURN_LIMIT = 0.06                                         # the series turn: |dt * qd| < TURN_LIMIT

_vp, _ll = C.c_void_p, C.c_longlong
ENTRY_POINTS = {name: (_vp, _vp, _ll, _vp) for name in
                ("probe_sincos_f64", "probe_sincos_f32", "probe_recip_f64", "probe_recip_f32", "probe_tanh_f64", "probe_tanh_f32",
                 "probe_wrap_f64", "probe_wrap_f32", "probe_normal", "probe_words")}
ENTRY_POINTS.update(probe_class_f64=(_vp, _vp, _vp, _ll, _vp), probe_class_f32=(_vp, _vp, _vp, _ll, _vp))


# ---------------------------------------------------------------------------------------
# build and load
# ---------------------------------------------------------------------------------------
def _digest(jit):
    h = hashlib.sha256()
    names = [PROBE_SRC] + [os.path.join(jit.CSRC, n) for n in ("os2r_kernels.hpp", "os2r_device.hpp", "os2r_models_gen.hpp",
                                                               "os2r_partials.hpp", "os2r_bits.hpp")]
    for name in names + [os.path.join(ROOT, "include", "os2r.h")]:
        with open(name, "rb") as f:
            h.update(f.read())
    h.update(f"|{jit.ARCH}|{' '.join(jit.FLAGS)}".encode())
    return h.hexdigest()


def build_probe(force=False):
    """Compile the probe as a shared library with the library's own flags (or fetch it from the cache); returns its path.
    Skips the calling test where there is no hipcc."""
    import pytest
    from gym_os2r_amd import jit
    hipcc = jit.hipcc_path()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    os.makedirs(KERNEL_CACHE, exist_ok=True)
    out = os.path.join(KERNEL_CACHE, f"os2r_math_probe_{_digest(jit)[:24]}.so")
    if os.path.exists(out) and not force:
        return out
    with tempfile.TemporaryDirectory(prefix="os2r_probe_") as tmp:
        obj = os.path.join(tmp, "probe.so")
        cmd = [hipcc, *jit.FLAGS, f"--offload-arch={jit.ARCH}", "-fPIC", "-shared", PROBE_SRC, "-o", obj]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0 and os.path.exists(obj), "hipcc failed on the math probe:\n" + r.stdout[-4000:]
        tmp_out = f"{out}.{os.getpid()}.tmp"
        os.replace(_copy(obj, tmp_out), out)
    return out


def _copy(src, dst):
    import shutil
    shutil.copyfile(src, dst)
    return dst


_lib = None


def load_probe():
    global _lib
    if _lib is None:
        path = build_probe()
        import torch  # noqa: F401  -- first: the process holds one HIP runtime, the one torch brings (gym_os2r_amd/_lib.py)
        _lib = C.CDLL(path)
        for name, argtypes in ENTRY_POINTS.items():
            fn = getattr(_lib, name)
            fn.argtypes, fn.restype = list(argtypes), C.c_int
    return _lib


def run(name, x, rows, out_dtype=None):
    """One launch of entry point `name` on the 1-D numpy array x (uploaded as it is, bit for bit); -> numpy [rows, n]."""
    import torch
    lib = load_probe()
    n = x.shape[-1]
    dev = torch.device("cuda")
    out = torch.zeros((rows, n), dtype=torch.from_numpy(np.zeros(1, out_dtype or x.dtype)).dtype, device=dev)
    if x.dtype.kind == "u":
        x = x.view(f"i{x.dtype.itemsize}")            # words travel as the signed integers of their width
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rc = getattr(lib, name)(xd.data_ptr(), out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_class(dtype, bits):
    """The class tests on bit patterns (an unsigned integer array of the width of dtype, uploaded as integers: nothing on the
    host sees them as floats) -> (bytes [5, n], bits of steer_abs [n])."""
    import torch
    lib = load_probe()
    n = bits.shape[0]
    dev = torch.device("cuda")
    signed = np.int64 if dtype == np.float64 else np.int32
    bd = torch.from_numpy(np.ascontiguousarray(bits).view(signed)).to(dev)
    cls = torch.zeros((5, n), dtype=torch.uint8, device=dev)
    mag = torch.zeros_like(bd)
    name = "probe_class_f64" if dtype == np.float64 else "probe_class_f32"
    rc = getattr(lib, name)(bd.data_ptr(), cls.data_ptr(), mag.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return cls.cpu().numpy(), mag.cpu().numpy().view(bits.dtype)


# ---------------------------------------------------------------------------------------
# one rounding per operation
# ---------------------------------------------------------------------------------------
def _rnd64(f):
    return float(f)                       # Fraction.__float__ is int / int, correctly rounded (ties to even)


def _rnd32(f):
    """The float32 nearest to the Fraction f (ties to even), as a Python float."""
    if f == 0:
        return 0.0
    a = abs(f)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # 2^(e-1) <= a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1                                                      # 2^e <= a < 2^(e+1)
    q = Fraction(2) ** (max(e, -126) - 23)
    n = round(a / q)                                                # round half to even
    v = float(n * q)                                                # exact: n < 2^25
    assert v <= 3.4028234663852886e38
    return -v if f < 0 else v


RND = {np.float64: _rnd64, np.float32: _rnd32}
EPS = {np.float64: 2.0 ** -52, np.float32: 2.0 ** -23}
F = Fraction

# the constants of sincos_fast, as written in os2r_device.hpp (float literals: the decimal text rounded to float32)
_f32 = lambda s: float(np.float32(s))  # noqa: E731
SC64 = dict(two_over_pi=float.fromhex("0x1.45f306dc9c883p-1"),
            c=[float.fromhex("0x1.921fb54442d18p+0"), float.fromhex("0x1.1a62633145c07p-54")],
            s=[float.fromhex(h) for h in ("0x1.5d93a5acfd57cp-33", "-0x1.ae5e68a2b9cebp-26", "0x1.71de357b1fe7dp-19",
                                          "-0x1.a01a019c161d5p-13", "0x1.111111110f8a6p-7", "-0x1.5555555555549p-3")],
            k=[float.fromhex(h) for h in ("-0x1.8fae9be8838d4p-37", "0x1.1ee9ebdb4b1c4p-29", "-0x1.27e4f809c52adp-22",
                                          "0x1.a01a019cb1590p-16", "-0x1.6c16c16c15177p-10", "0x1.555555555554cp-5")])
SC32 = dict(two_over_pi=_f32("0.636619772"),
            c=[_f32("1.5703125"), _f32("4.837512969970703125e-4"), _f32("7.54978995489188e-8")],
            s=[_f32("-1.9515295891e-4"), _f32("8.3321608736e-3"), _f32("-1.6666654611e-1")],
            k=[_f32("2.443315711809948e-5"), _f32("-1.388731625493765e-3"), _f32("4.166664568298827e-2")])
SC = {np.float64: SC64, np.float32: SC32}


def _rint(v):
    """Round a float to the nearest integer, ties to even (v_rndne)."""
    return float(round(F(v)))


def sincos_fast_exact(x, dtype=np.float64, consts=None):
    """sincos_fast(x) of os2r_device.hpp, operation by operation -> (sin, cos) as Python floats holding values of dtype.
    `consts` replaces the constants (the negative tests of the host suite)."""
    rnd, k_ = RND[dtype], consts or SC[dtype]
    x = float(x)
    k = _rint(rnd(F(x) * F(k_["two_over_pi"])))
    r = x
    for c in k_["c"]:
        r = rnd(F(-k) * F(c) + F(r))
    z = rnd(F(r) * F(r))
    ps = k_["s"][0]
    for c in k_["s"][1:]:
        ps = rnd(F(ps) * F(z) + F(c))
    sr = rnd(F(rnd(F(r) * F(z))) * F(ps) + F(r))
    pc = k_["k"][0]
    for c in k_["k"][1:]:
        pc = rnd(F(pc) * F(z) + F(c))
    cr = rnd(F(rnd(F(z) * F(z))) * F(pc) + F(rnd(F(-0.5) * F(z) + 1)))
    n = int(k)
    a, b = (cr, sr) if n & 1 else (sr, cr)
    return (-a if n & 2 else a), (-b if (n + 1) & 2 else b)


def _series_consts(dtype):
    c = lambda v: float(dtype(v))  # noqa: E731  -- T(-1.0 / 39916800.0): the double quotient, then the conversion
    return ([c(-1.0 / 39916800.0), c(1.0 / 362880.0), c(-1.0 / 5040.0), c(1.0 / 120.0), c(-1.0 / 6.0)],
            [c(-1.0 / 3628800.0), c(1.0 / 40320.0), c(-1.0 / 720.0), c(1.0 / 24.0), c(-0.5)])


def turn_exact(sn, cs, d, dtype=np.float64):
    """One series turn of substep step 1: (sin, cos) advanced by the angle d = dt * qd (already rounded) -> (sin, cos)."""
    rnd = RND[dtype]
    P, R = _series_consts(dtype)
    z = rnd(F(d) * F(d))
    p = rnd(F(z) * F(P[0]) + F(P[1]))
    for c in P[2:]:
        p = rnd(F(z) * F(p) + F(c))
    sd = rnd(F(rnd(F(d) * F(z))) * F(p) + F(d))
    r = rnd(F(z) * F(R[0]) + F(R[1]))
    for c in R[2:]:
        r = rnd(F(z) * F(r) + F(c))
    cm = rnd(F(z) * F(r))
    s1 = rnd(F(sn) + F(rnd(F(cs) * F(sd) + F(rnd(F(sn) * F(cm))))))
    c1 = rnd(F(cs) + F(rnd(F(-sn) * F(sd) + F(rnd(F(cs) * F(cm))))))
    return s1, c1


# ---------------------------------------------------------------------------------------
# argument sets (seeded; the same on every machine)
# ---------------------------------------------------------------------------------------
SEED = 20261021


def _below(v, dtype):
    return dtype(np.nextafter(dtype(v), dtype(0)))


def sincos_arguments(dtype, n_multiples=1000, n_random=1500):
    """Arguments of sincos_fast inside its guard: both floating-point neighbours of multiples of pi/2 across the whole fast
    range (every multiple in fp32, a seeded sample plus the first and the last in fp64), seeded random arguments (uniform, and
    log-uniform down to 2^-30), the last argument below the guard, 0, denormals, and the largest turn increment."""
    import mpmath
    rng = np.random.default_rng(SEED + (0 if dtype == np.float64 else 1))
    guard = GUARD[dtype]
    kmax = int(guard / (math.pi / 2))
    if dtype == np.float32:
        ks = np.arange(1, kmax + 1)
    else:
        ks = np.unique(np.concatenate([np.arange(1, 41), [kmax - 1, kmax], rng.integers(41, kmax - 1, n_multiples - 42)]))
    out = []
    with mpmath.workprec(200):
        for k in ks:
            m = int(k) * mpmath.pi / 2
            near = dtype(float(m)) if dtype == np.float64 else dtype(np.float64(float(m)))
            lo = near if mpmath.mpf(float(near)) <= m else dtype(np.nextafter(near, dtype(0)))
            hi = dtype(np.nextafter(lo, dtype(np.inf)))
            out += [lo, hi, -lo, -hi]
    out += list(rng.uniform(-guard, guard, n_random).astype(dtype))
    out += list((rng.choice([-1.0, 1.0], n_random // 3) * np.exp2(rng.uniform(-30, math.log2(guard), n_random // 3))).astype(dtype))
    tiny = np.finfo(dtype).tiny
    edge = [_below(guard, dtype), 0.0, np.finfo(dtype).smallest_subnormal, tiny / 2, tiny, _below(TURN_LIMIT, dtype), TURN_LIMIT,
            math.pi / 4, _below(math.pi / 4, dtype), 1.0, guard / 2]
    out += [dtype(v) for v in edge] + [dtype(-v) for v in edge]
    x = np.array(out, dtype=dtype)
    assert (np.abs(x) < dtype(guard)).all()
    return x


def turn_arguments(n_random=1500, dt=1e-4):
    """(q0, qd, dt) of the series turn, fp64: seeded random start angles in +-pi and speeds with |dt * qd| < 0.06, plus the
    speeds whose rounded increment dt * qd is the last below +-0.06, a zero and a denormal increment."""
    rng = np.random.default_rng(SEED + 2)
    q0 = rng.uniform(-math.pi, math.pi, n_random)
    qd = rng.uniform(-TURN_LIMIT, TURN_LIMIT, n_random) / dt
    top = (TURN_LIMIT / dt) * (1 - 2.0 ** -50)
    while dt * np.nextafter(top, np.inf) < TURN_LIMIT:
        top = float(np.nextafter(top, np.inf))
    assert dt * top < TURN_LIMIT <= dt * float(np.nextafter(top, np.inf))
    q0 = np.concatenate([q0, [0.3, -2.9, 0.0, 1.0, 1.0, math.pi / 2]])
    qd = np.concatenate([qd, [top, -top, top, 0.0, 5e-320, -top]])
    assert (np.abs(dt * qd) < TURN_LIMIT).all()
    return q0, qd, dt
