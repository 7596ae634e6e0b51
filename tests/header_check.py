"""What the host tests of the C-ABI libraries share: the prototypes of a header under include/ and the rule by which a C
parameter or result type agrees with a ctypes type (test_bindings_host.py, test_ilqr_backward_host.py,
test_ilqr_line_search_host.py), and the reading of the shared check helpers of csrc/os2r_host.hpp."""
import ctypes as C
import os
import re

from conftest import ROOT

INTEGERS = {"int": (C.c_int, C.c_int32), "int32_t": (C.c_int, C.c_int32), "int64_t": (C.c_int64,), "uint32_t": (C.c_uint32, C.c_uint),
            "uint64_t": (C.c_uint64,)}
HIP_CALL = r"\bhip[A-Z]\w*\("


def _is_pointer(ctype):
    return ctype in (C.c_void_p, C.c_char_p) or issubclass(ctype, C._Pointer)


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def _prototypes(header, prefix):
    """-> [(name, result type text, [argument text, ...])] of the `prefix`_* entry points of include/`header`, in its order."""
    text = re.sub(r"/\*.*?\*/", " ", _header(header), flags=re.S)
    out = []
    for ret, name, args in re.findall(r"OS2R_API\s+([^;()]*?)\s*\b(" + prefix + r"_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text, re.S):
        args = [" ".join(a.split()) for a in args.split(",")]
        out.append((name, " ".join(ret.split()), [] if args == ["void"] else args))
    return out


def _agrees(c_text, ctype, with_name):
    """One parameter (`with_name`) or result type of the header against its ctypes type, class by class."""
    if "*" in c_text or "[" in c_text:
        return _is_pointer(ctype)
    base = c_text.split()[:-1] if with_name else c_text.split()
    if base == ["double"]:
        return ctype is C.c_double                                   # by value
    return len(base) == 1 and ctype in INTEGERS.get(base[0], ())


def _csrc(name):
    with open(os.path.join(ROOT, "gym-os2r_amd", "csrc", name)) as f:
        return f.read()


def _function(src, signature):
    """The text of the function whose definition starts with the regular expression `signature`, up to its closing brace."""
    return re.search(signature + r"\(.*?\n}\n", src, re.S).group(0)


def checks_before_the_device(unit, entry_point, helpers):
    """An entry point of csrc/`unit` and the check helpers of os2r_host.hpp it calls: no HIP call and every refusal of an argument
    before check_device / DeviceGuard / launch.  -> the distinct refusal texts, the entry point's own and the helpers'."""
    body = _function(_csrc(unit), "int " + entry_point)
    host = _csrc("os2r_host.hpp")
    first_hip = min(body.index(t) for t in ("check_device(", "DeviceGuard", "auto launch", "launched("))
    assert not re.search(HIP_CALL, body[:first_hip])               # no HIP call of its own before that point
    texts = re.findall(r'fail\(OS2R_ERR_INVALID, "([^"]+)"', body)
    assert all(body.index(m) < first_hip for m in texts)
    # a helper gives the refusal's text, which the entry point hands to fail(OS2R_ERR_INVALID, ...) where it stands
    assert len(re.findall(r"fail\(OS2R_ERR_INVALID", body)) == len(texts) + len(helpers)
    for helper in helpers:
        use = f"if (const char* why = {helper}(layout)) return fail(OS2R_ERR_INVALID, why);"
        assert body.count(use) == 1 and body.index(use) < first_hip, helper
        text = _function(host, r"const char\* " + helper)
        assert not re.search(HIP_CALL + r"|check_device|DeviceGuard|launch", text), helper
        returned = re.findall(r'return "([^"]+)";', text)
        assert len(returned) + 1 == len(re.findall(r"\breturn\b", text)) and "return nullptr;" in text, helper
        texts += returned
    assert len(texts) == len(set(texts))
    return texts


def the_finite_and_symmetric_tests_make_no_hip_call():
    """... and they test what they are named for: bit patterns read from memory (the libraries are built without NaN semantics),
    entries compared exactly."""
    host = _csrc("os2r_host.hpp")
    text = {helper: _function(host, "bool " + helper) for helper in ("is_finite", "all_finite", "symmetric")}
    assert not re.search(HIP_CALL, "".join(text.values()))
    assert "__attribute__((noinline)) bool is_finite(const double* x)" in host and "std::memcpy(&b, x, sizeof(b))" in text["is_finite"]
    assert "!is_finite(&x[i])" in text["all_finite"] and "x[i * n + j] != x[j * n + i]" in text["symmetric"]
