"""Round 8 (docs/studies/round8_chain_interleave.md): the serialised chains of `os2r::substep` interleaved, the rows of the factor
taken from registers in the kernels of the compiled-in robots.  What that may cost is registers, so the budgets are read from the
gfx950 code objects inside the built libos2r.so with tools/kernel_meta.py, and the LDS instructions that went are counted in the
disassembly of the C4 bench kernel with tools/isa_histogram.py -- metadata and static code only, no GPU.

Budgets: no kernel with scratch, no kernel with a VGPR spill the parent build has not (it has them in one kernel), fp32 step
kernels within 256 registers and the C4 fp32 kernel within 256 unified registers (two waves per SIMD), 5-dof fp64 kernels within 512.
The parent's C4 kernel holds 58 `ds_*` instructions (profiles/r07_isa_histogram_C4.txt); without the mirror's 15 stores and the
loads of the three bodies' row set-ups fewer must be left."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C4_F64 = "step_kernel<double, os2r::StModel<double, 0>, true, true, true, os2r::StLayout"
C4_F32 = "step_kernel<float, os2r::StModel<float, 0>, true, true, true, os2r::StLayout"
PARENT_C4_DS = 58
# the one kernel of the parent build with VGPR spills (two, to AGPRs: no scratch): the 5-dof fp64 sweeps-only step kernel without
# per-env parameters; the fp64 sweeps-only kernels of the compiled-in robots keep the parent's form, this one with them
PARENT_SPILL = "step_kernel<double, os2r::StModel<double, 0>, true, false, false, os2r::RtLayout, false, 2, false>"


@pytest.fixture(scope="module")
def tools():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_histogram
    import kernel_meta
    from gym_os2r_amd import _lib
    assert os.path.exists(os.path.join(kernel_meta.LLVM, "llvm-readelf")), "needs ROCm's llvm-readelf"
    assert os.path.exists(_lib.LIB_PATH), "needs the built libos2r.so"
    return kernel_meta, isa_histogram, _lib.LIB_PATH


@pytest.fixture(scope="module")
def meta(tools):
    kernel_meta, _, path = tools
    m = kernel_meta.kernel_meta(path)
    assert len(m) >= 400, len(m)
    return m


def _bench_kernel(meta, prefix):
    """the plain step kernel of the bench: not the counting variant, not the fused rollout (`..., false, 1|2, false>`)"""
    hit = [k for k in meta if prefix in k and re.search(r">, false, \d, false>\(", k)]
    assert len(hit) == 1, hit
    return hit[0]


def test_no_kernel_has_scratch_or_a_new_vgpr_spill(meta):
    scratch = {k: v["private_segment_fixed_size"] for k, v in meta.items() if v["private_segment_fixed_size"] != 0}
    assert not scratch, scratch
    spills = {k: v["vgpr_spill_count"] for k, v in meta.items() if v["vgpr_spill_count"] != 0}
    new = {k: n for k, n in spills.items() if not (PARENT_SPILL in k and n <= 2)}
    assert not new, new


def test_fp32_step_kernels_within_256_registers(meta):
    fp32 = {k: v["vgpr_count"] for k, v in meta.items() if "step_kernel<float" in k}
    assert len(fp32) >= 40, len(fp32)
    bad = {k: r for k, r in fp32.items() if r > 256}
    assert not bad, bad


def test_c4_fp32_kernel_keeps_two_waves_per_simd(meta):
    v = meta[_bench_kernel(meta, C4_F32)]
    assert v["vgpr_count"] <= 256 and v["group_segment_fixed_size"] <= 160 * 1024 // 8, v     # 512 registers, two waves per SIMD; LDS for 8 waves per CU


def test_five_dof_fp64_kernels_within_512_registers(meta):
    fp64 = {k: v["vgpr_count"] for k, v in meta.items()
            if re.search(r"_kernel<double\b", k) and re.search(r"(StModel<double, 0>|RtModel<double, 5>)", k)}
    assert len(fp64) >= 20, len(fp64)
    bad = {k: r for k, r in fp64.items() if r > 512}
    assert not bad, bad


def test_c4_kernel_has_fewer_lds_instructions_than_the_parent(tools, meta):
    _, isa_histogram, path = tools
    assert C4_F64 == isa_histogram.DEFAULT_KERNEL
    name, _, insts = isa_histogram.disassemble(path, C4_F64)
    assert name.strip() == _bench_kernel(meta, C4_F64).strip(), name
    n = sum(1 for _, mn, _ in insts if mn.startswith("ds_"))
    print(f"[chain interleave] ds_* instructions in the C4 kernel: {n} (parent {PARENT_C4_DS})")
    assert 0 < n < PARENT_C4_DS, n
