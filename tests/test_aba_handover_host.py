"""Resource budgets of the kernels that inline `os2r::substep` (csrc/os2r_device.hpp), read from the gfx950 code objects inside the
built libos2r.so with tools/kernel_meta.py -- metadata only, no GPU.  Round 7 keeps the joint rotations and the articulated-body
hand-over of the compiled-in robots in registers instead of rebuilding them / passing them through LDS; that is only worth having
while nothing spills: no scratch in any step, linearize or policy kernel, the fp32 ones inside 256 registers (two waves per
SIMD), the 5-dof fp64 ones inside the 512 unified registers of a lone wave."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def families():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    from gym_os2r_amd import _lib
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")), "needs ROCm's llvm-readelf"
    assert os.path.exists(_lib.LIB_PATH), "needs the built libos2r.so"
    meta = kernel_meta.kernel_meta(_lib.LIB_PATH)
    out = {"step": {k: v for k, v in meta.items() if "step_kernel<" in k},
           "linearize": {k: v for k, v in meta.items() if "linearize_kernel<" in k},
           "policy": {k: v for k, v in meta.items() if "policy" in k.split("(")[0]}}
    assert len(out["step"]) >= 80 and len(out["linearize"]) >= 16 and len(out["policy"]) >= 8, {f: len(v) for f, v in out.items()}
    return out


def _fp32(name):
    return re.search(r"_kernel<float\b", name) is not None


def _five_dof_fp64(name):
    return re.search(r"_kernel<double\b", name) is not None and re.search(r"(StModel<double, 0>|RtModel<double, 5>)", name) is not None


@pytest.mark.parametrize("family", ["step", "linearize", "policy"])
def test_no_scratch(families, family):
    bad = {k: v["private_segment_fixed_size"] for k, v in families[family].items() if v["private_segment_fixed_size"] != 0}
    assert not bad, bad


@pytest.mark.parametrize("family", ["step", "linearize", "policy"])
def test_fp32_kernels_fit_two_waves_per_simd(families, family):
    fp32 = {k: v["vgpr_count"] for k, v in families[family].items() if _fp32(k)}
    assert fp32, family
    bad = {k: r for k, r in fp32.items() if r > 256}
    assert not bad, bad


@pytest.mark.parametrize("family", ["step", "linearize", "policy"])
def test_five_dof_fp64_kernels_fit_the_register_file(families, family):
    fp64 = {k: v["vgpr_count"] for k, v in families[family].items() if _five_dof_fp64(k)}
    assert fp64, family
    bad = {k: r for k, r in fp64.items() if r > 512}
    assert not bad, bad
