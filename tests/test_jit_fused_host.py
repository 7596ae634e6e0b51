"""gym_os2r_amd/jit.py beyond the step object: the code objects of the fused rollout, the fused policy rollout and linearize
for a custom robot (csrc/os2r_jit_fused_unit.hip), built by hipcc --genco without a GPU.  Loading and running them is
tests/test_gpu_jit_fused.py, which imports the robot and the configuration from here and finds the cache filled."""
import os
import warnings

import numpy as np
import pytest

from conftest import KERNEL_CACHE
from helpers import make_config, perturbed_model
from gym_os2r_amd import abi, jit

FUSED_NAMES = {"rollout": (b"os2r_jit_rollout_c1_d0", b"os2r_jit_rollout_c1_d1"),
               "policy": (b"os2r_jit_policy_c1_d0", b"os2r_jit_policy_c1_d1"),
               "linearize": (b"os2r_jit_lin_c1_d0", b"os2r_jit_lin_c1_d1", b"os2r_jit_lin_c1_d0_s", b"os2r_jit_lin_c1_d1_s")}


def robot():
    """No other test uses this robot, so none can have registered code objects for it."""
    return perturbed_model("free_hip", np.random.default_rng(79))


def config(dtype=abi.F64, n=200, contact=True, **kw):
    """free_hip, BalancingV1, N = 200: three full waves and a tail of 8."""
    return make_config("free_hip", "BalancingV1", True, num_envs=n, contact=contact, dtype=dtype, model_overrides=robot(), **kw)[0]


@pytest.fixture
def cache(monkeypatch):
    if jit.hipcc_path() is None:
        pytest.skip("no hipcc on this machine")
    monkeypatch.setenv("OS2R_KERNEL_CACHE", KERNEL_CACHE)
    monkeypatch.delenv("OS2R_JIT_FUSED", raising=False)
    return KERNEL_CACHE


def test_every_kind_builds_and_exports_its_kernels(cache):
    for dtype in (abi.F64, abi.F32):
        cfg = config(dtype)
        layout = jit.task_layout(cfg.task)
        assert layout is not None and layout[2] == 10
        with warnings.catch_warnings():
            warnings.simplefilter("error")                      # a kind that fails to build only warns
            paths = jit.build_all(cfg.model, dtype, True, layout)
        assert tuple(paths) == jit.KINDS == ("step", "rollout", "policy", "linearize")
        assert paths["step"] == jit.code_object_path(cfg.model, dtype, True, layout)      # as called without a kind
        assert len(set(paths.values())) == 4
        for kind, path in paths.items():
            assert path == jit.code_object_path(cfg.model, dtype, True, layout, kind)
            blob = open(path, "rb").read()
            assert b"\x7fELF" in blob[:8192], kind             # (hipcc --genco wraps the gfx950 ELF in an offload bundle)
            if kind == "step":
                assert b"os2r_jit_step_c1_d0_l" in blob and b"os2r_jit_step_c1_d1_s" in blob
                assert not any(n in blob for names in FUSED_NAMES.values() for n in names)
                continue
            assert all(n in blob for n in FUSED_NAMES[kind]), kind
            assert b"os2r_jit_step_" not in blob, kind
            other = [n for k, names in FUSED_NAMES.items() if k != kind for n in names]
            assert not any(n in blob for n in other), kind
            # the fused kernels have the task's layout folded in and say so; linearize has no epilogue
            assert (b"os2r_jit_layout" in blob) == (kind != "linearize"), kind
            assert b"os2r_jit_lin_c0" not in blob
    # without ground contact there are no fused rollouts: the step object and the linearize object of that flag
    cfg = config(contact=False)
    paths = jit.build_all(cfg.model, abi.F64, False, jit.task_layout(cfg.task))
    assert tuple(paths) == ("step", "linearize")
    blob = open(paths["linearize"], "rb").read()
    assert all(n in blob for n in (b"os2r_jit_lin_c0_d0", b"os2r_jit_lin_c0_d1_s")) and b"os2r_jit_lin_c1" not in blob
    assert b"os2r_jit_step_" not in blob


def test_cache_keys_and_the_build_plan(cache, monkeypatch):
    cfg = config()
    layout = jit.task_layout(cfg.task)
    seen = set()
    for kind in jit.KINDS:
        path = jit.build(cfg.model, abi.F64, True, layout=layout, kind=kind)
        mtime = os.path.getmtime(path)
        assert jit.build(cfg.model, abi.F64, True, layout=layout, kind=kind) == path and os.path.getmtime(path) == mtime
        for other in (jit.code_object_path(cfg.model, abi.F32, True, layout, kind), jit.code_object_path(cfg.model, abi.F64, False, layout, kind)):
            assert other != path
            seen.add(other)
        seen.add(path)
    assert len(seen) == 12                                      # kinds x {dtype, contact flag}: all different
    # a folded layout is part of the key where there is one to fold
    assert jit.code_object_path(cfg.model, abi.F64, True, None, "rollout") != jit.code_object_path(cfg.model, abi.F64, True, layout, "rollout")
    assert jit.code_object_path(cfg.model, abi.F64, True, None, "linearize") == jit.code_object_path(cfg.model, abi.F64, True, layout, "linearize")
    with pytest.raises(ValueError):
        jit.code_object_path(cfg.model, abi.F64, True, layout, "mlp")
    # the plan: fused rollouts exist with ground contact only; OS2R_JIT_FUSED=0 is the step object alone
    assert jit.planned_kinds(True) == jit.KINDS and jit.planned_kinds(False) == ("step", "linearize")
    monkeypatch.setenv("OS2R_JIT_FUSED", "0")
    assert jit.planned_kinds(True) == jit.planned_kinds(False) == ("step",)
    assert jit.build_all(cfg.model, abi.F64, True, layout) == {"step": jit.code_object_path(cfg.model, abi.F64, True, layout)}


def test_a_failed_extra_build_warns_and_keeps_the_step_kernels(cache, monkeypatch, tmp_path):
    cfg = config()
    layout = jit.task_layout(cfg.task)
    step = jit.build(cfg.model, abi.F64, True, layout=layout)
    monkeypatch.setenv("OS2R_KERNEL_CACHE", str(tmp_path))      # a cache that holds the step object and nothing else
    cached = jit.code_object_path(cfg.model, abi.F64, True, layout)
    assert os.path.dirname(cached) == str(tmp_path)
    with open(step, "rb") as src, open(cached, "wb") as dst:
        dst.write(src.read())
    monkeypatch.setenv("HIPCC", "/bin/false")
    assert jit.hipcc_path() == "/bin/false"
    with pytest.warns(UserWarning) as caught:
        paths = jit.build_all(cfg.model, abi.F64, True, layout)
    assert paths == {"step": cached}
    assert sorted(str(w.message).split()[1] for w in caught) == ["linearize", "policy", "rollout"]
    assert os.listdir(tmp_path) == [os.path.basename(cached)]   # no half-written file left behind

    class Lib:                                                  # what specialise() asks of the library, recorded
        registered = []

        def os2r_model_is_compiled_in(self, model):
            return 0

        def os2r_register_model_kernels(self, model, dtype, device, path):
            self.registered.append(path.decode())
            return 0

    monkeypatch.setenv("OS2R_JIT", "1")
    with pytest.warns(UserWarning):
        assert jit.specialise(Lib(), cfg) is True               # the step kernels serve the handle
    assert Lib.registered == [cached]
    # ... while a step object that cannot be built is an error of the whole specialisation
    os.remove(cached)
    with pytest.raises(RuntimeError):
        jit.build_all(cfg.model, abi.F64, True, layout)
