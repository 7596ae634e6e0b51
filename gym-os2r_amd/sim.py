"""Thin Python handle over one ``Os2rSim`` of the C-ABI: torch tensors in, torch tensors out.

torch is used only for device memory and the current HIP stream; every call goes straight
to ``libos2r.so``.  All tensors stay on the GPU.  The simulator is here: create, step, rollouts, state, copies and linearize;
the controller calls on top of it (LQR, iLQR, MPPI, the particle filter) are in gym_os2r_amd.controllers.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib, abi
from ._lib import Os2rError, _PybindLib, _ptr  # noqa: F401  (Os2rError and _ptr are taken from here)
from .controllers import Controllers


class HipSim(Controllers):
    """N environments resident on one GPU."""

    def __init__(self, cfg: abi.Os2rConfig, device: Optional[torch.device] = None, binding: Optional[str] = None):
        import os
        binding = binding or os.environ.get("OS2R_BINDING", "ctypes")
        _lib.load()                                   # the C-ABI library must be there either way
        self._lib = _PybindLib() if binding == "pybind11" else _lib.load()
        self.binding = binding
        if not torch.cuda.is_available():
            raise Os2rError("no GPU visible: the stepper runs on MI355X only (no CPU fallback)")
        self.device = torch.device(device if device is not None else f"cuda:{cfg.device}")
        if self.device.index is not None:
            cfg.device = self.device.index
        self.cfg = cfg
        self.N, self.nq, self.D = int(cfg.num_envs), int(cfg.model.nq), int(cfg.task.obs_dim)
        self.dtype = torch.float64 if cfg.dtype == abi.F64 else torch.float32
        # a robot that is not compiled in gets its own kernels (gym_os2r_amd/jit.py; OS2R_JIT=0: generic ones)
        from . import jit
        self.specialised = jit.specialise(_lib.load(), cfg)
        self._counters = None                         # count_work(True) allocates the work counters
        self._mirror = None                           # violation_mirror(): numpy view of the handle's two host words
        self.reasons = None                           # done_reasons(True) allocates the done-reason output
        self._h = C.c_void_p()
        rc = self._lib.os2r_create(C.byref(cfg), C.byref(self._h))
        if rc != abi.OK:
            raise Os2rError(f"os2r_create failed ({rc}): {self._lib.os2r_last_error(None).decode()}")

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != abi.OK:
            raise Os2rError(f"{what} failed ({rc}): {self._lib.os2r_last_error(self._h).decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _layout(self):
        """The handle as the companion libraries take it (an Os2rControlLayout), filled once from the handle's config."""
        lay = self.__dict__.get("_control_layout")
        if lay is None:
            from . import control
            lay = self._control_layout = control.layout(abi.F64 if self.dtype == torch.float64 else abi.F32, self.nq, self.cfg.device,
                                                        control.slot_columns(self.cfg.task, self.nq))
        return lay

    def _new(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or self.dtype, device=self.device)

    def _in(self, t, shape, dtype=None):
        # anything that speaks DLPack (`__dlpack__`: another framework's device array, a capsule) is taken over without a
        # copy when it already lives on this device in the handle's dtype; torch tensors and host arrays as before
        if not isinstance(t, torch.Tensor) and (hasattr(t, "__dlpack__") or type(t).__name__ == "PyCapsule") and not hasattr(t, "__array_interface__"):
            t = torch.from_dlpack(t)
        t = torch.as_tensor(t, device=self.device).to(dtype or self.dtype).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def close(self):
        if getattr(self, "_h", None):
            self._lib.os2r_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- hot path ---------------------------------------------------------------------------
    def step(self, actions: Optional[torch.Tensor] = None, want_terminal: bool = True, want_mask: bool = False):
        """-> obs [N,D], reward [N], done [N] uint8 flags, terminal_obs [N,D] or None (and, want_mask: done_mask [N] bool --
        `flags != 0`, written by the same launch: include/os2r.h, os2r_set_done_mask)."""
        a = None if actions is None else self._in(actions, (self.N, 2))
        obs, rew = self._new(self.N, self.D), self._new(self.N)
        done = self._new(self.N, dtype=torch.uint8)
        term = self._new(self.N, self.D) if want_terminal else None
        if want_mask:
            mask = self._new(self.N, dtype=torch.bool)     # one byte per element; the kernel stores 0 / 1
            self._check(self._lib.os2r_set_done_mask(self._h, _ptr(mask)), "os2r_set_done_mask")
        self._check(self._lib.os2r_step(self._h, _ptr(a), _ptr(obs), _ptr(rew), _ptr(done), _ptr(term),
                                        self._stream()), "os2r_step")
        if want_mask:
            self._check(self._lib.os2r_set_done_mask(self._h, None), "os2r_set_done_mask")   # the handle keeps no pointer to a tensor it does not own
            return obs, rew, done, term, mask
        return obs, rew, done, term

    def violation_mirror(self):
        """numpy uint32 [2] view of the handle's two words of pinned host memory (include/os2r.h: os2r_get_violation_mirror):
        [0] the running count of clamped caller actions as the launches before the newest one that has STARTED left it,
        [1] the low 32 bits of that launch's step counter.  Reading it costs a load: no copy, no event, no wait."""
        if self._mirror is None:
            import numpy as np
            p = C.c_void_p()
            self._check(self._lib.os2r_get_violation_mirror(self._h, C.byref(p)), "os2r_get_violation_mirror")
            self._mirror = np.ctypeslib.as_array((C.c_uint32 * 2).from_address(p.value))
        return self._mirror

    def step_into(self, actions, obs, rew, done, term=None):
        """Allocation-free variant writing into caller tensors."""
        self._check(self._lib.os2r_step(self._h, _ptr(actions), _ptr(obs), _ptr(rew), _ptr(done), _ptr(term),
                                        self._stream()), "os2r_step")

    def rollout(self, nsteps: int, actions=None, want_terminal: bool = False, want_reasons: bool = False):
        """`nsteps` env-steps in one call (include/os2r.h: os2r_rollout; one launch where a fused kernel exists): open-loop
        actions [K,N,2] or None (on-device random actions).  -> obs [K,N,D], reward [K,N], done [K,N] uint8 flags,
        terminal_obs [K,N,D] or None, reasons [K,N] int16 or None -- what K calls of step() return, bit for bit."""
        K = int(nsteps)
        a = None if actions is None else self._in(actions, (K, self.N, 2))
        obs, rew, done, term, why = self._steps_out(K, want_terminal, want_reasons)
        self._check(self._lib.os2r_rollout(self._h, K, _ptr(a), _ptr(obs), _ptr(rew), _ptr(done), _ptr(term), _ptr(why),
                                           self._stream()), "os2r_rollout")
        return obs, rew, done, term, why

    def _out(self, t, shape, dtype, what):
        """A caller-owned output (or raw input) tensor handed to the library by address: it must be what the kernel assumes."""
        if t is None:
            return
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"{what}: expected a contiguous {dtype} tensor of shape {tuple(shape)} on {self.device}, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")

    def _steps_out(self, K, want_terminal=False, want_reasons=False, given=None):
        """The per-step outputs of a K-step rollout, (obs [K,N,D], rew [K,N], done [K,N] uint8, term [K,N,D], reasons [K,N] int16):
        new tensors, term and reasons only where wanted; or the caller's own (`given`), checked."""
        specs = (("obs", (K, self.N, self.D), self.dtype), ("rew", (K, self.N), self.dtype), ("done", (K, self.N), torch.uint8),
                 ("term", (K, self.N, self.D), self.dtype), ("reasons", (K, self.N), torch.int16))
        if given is not None:
            for (what, shape, dtype), t in zip(specs, given):
                self._out(t, shape, dtype, what)
            return given
        return tuple(self._new(*shape, dtype=dtype) if want else None
                     for (_, shape, dtype), want in zip(specs, (True, True, True, want_terminal, want_reasons)))

    def rollout_into(self, nsteps: int, actions, obs, rew, done, term=None, reasons=None):
        """Allocation-free variant of rollout() writing into caller tensors ([K,N,...]); shapes, dtypes, device and
        contiguity are checked (the library takes addresses: a wrong K or dtype would write out of bounds)."""
        K = int(nsteps)
        if obs is None or rew is None or done is None:
            raise ValueError("rollout_into: obs, rew and done are required")
        self._out(actions, (K, self.N, 2), self.dtype, "actions")
        self._steps_out(K, given=(obs, rew, done, term, reasons))
        self._check(self._lib.os2r_rollout(self._h, int(nsteps), _ptr(actions), _ptr(obs), _ptr(rew), _ptr(done), _ptr(term),
                                           _ptr(reasons), self._stream()), "os2r_rollout")

    def _sigma(self, sigma):
        """sigma of rollout_policy -> (contiguous tensor in the kernel's layout, flag bits)."""
        if isinstance(sigma, bool):
            raise ValueError("rollout_policy: sigma must be a float, a [2] tensor or an [N, 2] tensor")
        if isinstance(sigma, (int, float)):
            return torch.full((2,), float(sigma), dtype=self.dtype, device=self.device), 0
        if not isinstance(sigma, torch.Tensor):
            raise ValueError(f"rollout_policy: sigma must be a float, a [2] tensor or an [N, 2] tensor, got {type(sigma)}")
        shape = tuple(sigma.shape)
        if shape not in ((2,), (self.N, 2)):
            raise ValueError(f"rollout_policy: sigma must be [2] or [{self.N}, 2], got {shape}")
        if sigma.dtype != self.dtype or sigma.device != self.device:
            raise ValueError(f"rollout_policy: sigma must be {self.dtype} on {self.device}, got {sigma.dtype} on {sigma.device}")
        if shape == (2,):
            return sigma.contiguous(), 0
        return sigma.t().contiguous(), abi.POLICY_SIGMA_PER_ENV      # the kernel's layout: [2][N], env index fastest

    def _noise_args(self, name, sigma, salt, **wants):
        """sigma and salt of rollout_policy / rollout_schedule (`name`) -> (sigma tensor or None, its flag bits, salt), checked;
        `wants` are the outputs that exist only with sigma."""
        if sigma is None and (any(wants.values()) or salt):
            raise ValueError(f"{name}: {', '.join(wants)} and salt need sigma (sigma=0.0: the deterministic policy)")
        if not 0 <= int(salt) < 2 ** 32:
            raise ValueError(f"{name}: salt must be a 32-bit unsigned value")
        return ((None, 0) if sigma is None else self._sigma(sigma)) + (int(salt),)

    def _policy_weights(self, name, weights, table):
        """weights of rollout_policy ([2, D+1], or one set per environment [N, 2, D+1]) or, `table`, of rollout_schedule (the
        same behind a T: [T, 2, D+1] or [N, T, 2, D+1]) -> (contiguous tensor in the kernel's layout, the per-env flag bit, T)."""
        R = self.D + 1
        if not isinstance(weights, torch.Tensor):
            weights = torch.as_tensor(weights)
        shape = tuple(weights.shape)
        lead = shape[:-2]                          # what stands before the [2, D+1] of one set: (), (N,), (T,) or (N, T)
        per_env = len(lead) == 1 + table and lead[0] == self.N
        T = lead[-1] if table and lead else 1
        if shape[-2:] != (2, R) or len(lead) != table + per_env or T < 1:
            want = f"[T, 2, {R}] or [{self.N}, T, 2, {R}] with T >= 1" if table else f"[2, {R}] or [{self.N}, 2, {R}]"
            raise ValueError(f"{name}: weights must be {want}, got {shape}")
        if weights.dtype != self.dtype or weights.device != self.device:
            raise ValueError(f"{name}: weights must be {self.dtype} on {self.device}, got {weights.dtype} on {weights.device}")
        # the kernel's layout per environment: [T][2][D+1][N], env index fastest
        return (weights.movedim(0, -1) if per_env else weights).contiguous(), abi.POLICY_PER_ENV if per_env else 0, T

    def _knot_args(self, K, knots, first_knot, knot_state, knot_params, want_knot_obs):
        """The recording keywords of rollout_schedule / rollout_policy -> None when none of them is used (the call is then the one
        it always was), else (knots handle or None, first_knot, what); everything that needs no device is refused here."""
        if knots is None and first_knot == 0 and knot_state is True and knot_params is True and not want_knot_obs:
            return None
        name = "rollout_schedule"
        if knots is None:
            if not want_knot_obs:
                raise ValueError(f"{name}: first_knot, knot_state and knot_params need a knots handle (or want_knot_obs)")
            return None, 0, 0
        if not isinstance(knots, HipSim):
            raise ValueError(f"{name}: knots must be a HipSim, got {type(knots)}")
        if knots is self:
            raise ValueError(f"{name}: knots must be another handle than the one that rolls out")
        if knots.dtype != self.dtype or knots.device != self.device:
            raise ValueError(f"{name}: knots must be {self.dtype} on {self.device}, got {knots.dtype} on {knots.device}")
        if isinstance(first_knot, bool) or not isinstance(first_knot, int) or not 0 <= first_knot < 2 ** 31:
            raise ValueError(f"{name}: first_knot must be a non-negative 32-bit integer, got {first_knot!r}")
        if not knot_state and not knot_params:
            raise ValueError(f"{name}: nothing to record (knot_state and knot_params are both off)")
        if (first_knot + K) * self.N > knots.N:
            raise ValueError(f"{name}: knots has {knots.N} environments, (first_knot + nsteps) * N = {(first_knot + K) * self.N} are needed")
        return knots, first_knot, (abi.COPY_STATE if knot_state else 0) | (abi.COPY_PARAMS if knot_params else 0)

    def _recorded(self, rec, want_knot_obs, K, w, T, first_slot, flags, sg, salt, ret, length, outs, act, eps):
        """os2rr_rollout_policy_recorded (include/os2r_record.h: the companion library libos2r_record.so, or the pybind11 module,
        which links it) with the arguments of the scheduled call behind the sink's; -> knot_obs [K, N, D] | None"""
        call = getattr(self._lib, "os2rr_rollout_policy_recorded", None)
        if call is None:
            try:
                call = _lib.load_record().os2rr_rollout_policy_recorded
            except (ImportError, OSError, AttributeError) as e:
                raise Os2rError(f"no rollout can record its knots without libos2r_record.so: {e}") from e
        knots, first_knot, what = rec
        knot_obs = self._new(K, self.N, self.D) if want_knot_obs else None
        obs, rew, done, term, why = outs
        self._check(call(
            self._h, None if knots is None else knots._h, first_knot, what, _ptr(knot_obs), K, _ptr(w), T, int(first_slot), flags,
            _ptr(sg), salt, _ptr(ret), _ptr(length), _ptr(obs), _ptr(rew), _ptr(done), _ptr(term), _ptr(why), _ptr(act), _ptr(eps),
            self._stream()), "os2rr_rollout_policy_recorded")
        return knot_obs

    def rollout_policy(self, nsteps: int, weights, *, tanh: bool = False, first_episode: bool = False, want_outputs: bool = False,
                       want_terminal: bool = False, want_reasons: bool = False, sigma=None, salt: int = 0,
                       want_actions: bool = False, want_noise: bool = False, knots: Optional["HipSim"] = None, first_knot: int = 0,
                       knot_state: bool = True, knot_params: bool = True, want_knot_obs: bool = False):
        """`nsteps` env-steps with the linear policy a = squash(W.o + b) in the loop, evaluated on the device on every environment's
        own observation (include/os2r.h: os2r_rollout_policy; one launch where os2r_rollout has a fused kernel).
        weights: [2, D+1] shared by all environments or [N, 2, D+1] one set per environment; row j (0 hip, 1 knee) holds
        W_j0 .. W_j,D-1, b_j.  squash: clip to [-1, 1], or tanh.  first_episode: the sums stop after an environment's first
        done flag in the window.  -> (returns [N], lengths [N] int32, outputs): outputs is the rollout() tuple
        (obs, reward, done, terminal_obs, reasons) when want_outputs, else None (nothing per step is written then).
        sigma (a float, a [2] tensor or an [N, 2] tensor in the handle's dtype): Gaussian exploration noise, a = squash(W.o + b +
        sigma * eps) with eps ~ N(0, 1) a pure function of (seed, global env index, step counter, salt) (include/os2r.h:
        os2r_rollout_policy_noisy); the call then returns a fourth element (actions [K, N, 2] if want_actions else None,
        noise eps [K, N, 2] if want_noise else None): rollout(K, actions) replays the window bit for bit.
        knots, first_knot, knot_state, knot_params, want_knot_obs: the recording of rollout_schedule
        (include/os2r_record.h: os2rr_rollout_policy_recorded with period = 1); with any of them the call returns one more element,
        knot_obs [K, N, D] | None,
        behind the (actions, noise) pair, which is then there without sigma too (as (None, None))."""
        K = int(nsteps)
        if K < 1:
            raise ValueError("rollout_policy: nsteps must be >= 1")
        rec = self._knot_args(K, knots, first_knot, knot_state, knot_params, want_knot_obs)
        sg, sg_flags, salt = self._noise_args("rollout_policy", sigma, salt, want_actions=want_actions, want_noise=want_noise)
        w, per_env, _ = self._policy_weights("rollout_policy", weights, table=False)
        flags = (abi.POLICY_TANH if tanh else 0) | (abi.POLICY_FIRST_EPISODE if first_episode else 0) | per_env
        ret, length = self._new(self.N), self._new(self.N, dtype=torch.int32)
        outs = self._steps_out(K, want_terminal, want_reasons) if want_outputs else (None,) * 5
        obs, rew, done, term, why = outs
        if rec is not None:
            act = self._new(K, self.N, 2) if want_actions else None
            eps = self._new(K, self.N, 2) if want_noise else None
            knot_obs = self._recorded(rec, want_knot_obs, K, w, 1, 0, flags | sg_flags, sg, salt, ret, length, outs, act, eps)
            return ret, length, (outs if want_outputs else None), (act, eps), knot_obs
        if sg is not None:
            act = self._new(K, self.N, 2) if want_actions else None
            eps = self._new(K, self.N, 2) if want_noise else None
            self._check(self._lib.os2r_rollout_policy_noisy(self._h, K, _ptr(w), flags | sg_flags, _ptr(sg), salt, _ptr(ret),
                                                            _ptr(length), _ptr(obs), _ptr(rew), _ptr(done), _ptr(term), _ptr(why),
                                                            _ptr(act), _ptr(eps), self._stream()), "os2r_rollout_policy_noisy")
            return ret, length, (outs if want_outputs else None), (act, eps)
        self._check(self._lib.os2r_rollout_policy(self._h, K, _ptr(w), flags, _ptr(ret), _ptr(length), _ptr(obs), _ptr(rew),
                                                  _ptr(done), _ptr(term), _ptr(why), self._stream()), "os2r_rollout_policy")
        return ret, length, (outs if want_outputs else None)

    def rollout_schedule(self, nsteps: int, weights, *, clock: str = "window", wrap: bool = False, first_slot: int = 0,
                         tanh: bool = False, first_episode: bool = False, sigma=None, salt: int = 0, want_outputs: bool = False,
                         want_terminal: bool = False, want_reasons: bool = False, want_actions: bool = False,
                         want_noise: bool = False, knots: Optional["HipSim"] = None, first_knot: int = 0, knot_state: bool = True,
                         knot_params: bool = True, want_knot_obs: bool = False):
        """`nsteps` env-steps with a time-scheduled linear policy in the loop (include/os2r.h: os2r_rollout_policy_scheduled; one
        launch where os2r_rollout has a fused kernel): a table of T weight sets, each as rollout_policy takes one, of which every
        environment evaluates the set of its slot in each env-step.
        weights: [T, 2, D+1] shared by all environments or [N, T, 2, D+1] one table per environment.
        clock: "window": t = first_slot + k in env-step k of the call; "episode": t = first_slot + the environment's elapsed
        episode steps (episode_info()[0] at the top of the env-step; 0 right after a reset or an auto-reset).
        The slot is min(t, T-1) -- the last set is held --, or t mod T with wrap.  On the window clock a window may be split:
        K steps equal K1 steps followed by K - K1 steps with first_slot + K1, bit for bit.
        sigma, salt, want_noise: the exploration noise of rollout_policy.  want_actions works with and without sigma:
        rollout(K, actions) replays the window bit for bit.
        knots (include/os2r_record.h: os2rr_rollout_policy_recorded; the same launch): another HipSim of the same dtype, device and robot
        with at least (first_knot + K) N environments; at the top of env-step k, before the action is formed, environment e -- after
        its reset, if the previous env-step auto-reset it -- becomes environment (first_knot + k) N + e of `knots`, exactly as
        knots.copy_envs_from(self, index, state=knot_state, params=knot_params) would copy it; every other environment of `knots`
        stays as it is.  knots.linearize then returns the Jacobians of every knot, knot-major.  first_knot splits a window as
        first_slot does.  want_knot_obs: the observation the policy evaluates at the top of each env-step, [K, N, D]: the `obs` of
        lqr_gains / ilqr_backward as [K N, D], with or without `knots`.
        -> (returns [N], lengths [N] int32, outputs | None, (actions [K, N, 2] | None, noise [K, N, 2] | None)), and with any of the
        recording keywords one more element: knot_obs [K, N, D] | None."""
        K = int(nsteps)
        if K < 1:
            raise ValueError("rollout_schedule: nsteps must be >= 1")
        if clock not in ("window", "episode"):
            raise ValueError(f"rollout_schedule: clock must be 'window' or 'episode', got {clock!r}")
        if not 0 <= int(first_slot) < 2 ** 31:
            raise ValueError("rollout_schedule: first_slot must be a non-negative 32-bit value")
        sg, sg_flags, salt = self._noise_args("rollout_schedule", sigma, salt, want_noise=want_noise)
        rec = self._knot_args(K, knots, first_knot, knot_state, knot_params, want_knot_obs)
        w, per_env, T = self._policy_weights("rollout_schedule", weights, table=True)
        flags = ((abi.POLICY_TANH if tanh else 0) | (abi.POLICY_FIRST_EPISODE if first_episode else 0) | per_env |
                 (abi.POLICY_CLOCK_EPISODE if clock == "episode" else 0) | (abi.POLICY_SCHEDULE_WRAP if wrap else 0))
        ret, length = self._new(self.N), self._new(self.N, dtype=torch.int32)
        outs = self._steps_out(K, want_terminal, want_reasons) if want_outputs else (None,) * 5
        obs, rew, done, term, why = outs
        act = self._new(K, self.N, 2) if want_actions else None
        eps = self._new(K, self.N, 2) if want_noise else None
        if rec is not None:
            knot_obs = self._recorded(rec, want_knot_obs, K, w, T, first_slot, flags | sg_flags, sg, salt, ret, length, outs, act, eps)
            return ret, length, (outs if want_outputs else None), (act, eps), knot_obs
        self._check(self._lib.os2r_rollout_policy_scheduled(self._h, K, _ptr(w), T, int(first_slot), flags | sg_flags, _ptr(sg), salt,
                                                            _ptr(ret), _ptr(length), _ptr(obs), _ptr(rew), _ptr(done), _ptr(term),
                                                            _ptr(why), _ptr(act), _ptr(eps), self._stream()),
                    "os2r_rollout_policy_scheduled")
        return ret, length, (outs if want_outputs else None), (act, eps)

    def reset(self, mask: Optional[torch.Tensor] = None):
        m = None if mask is None else self._in(mask, (self.N,), torch.uint8)
        obs = self._new(self.N, self.D)
        self._check(self._lib.os2r_reset(self._h, _ptr(m), _ptr(obs), self._stream()), "os2r_reset")
        return obs

    def bench_steps(self, nsteps: int) -> float:
        """GPU milliseconds (HIP events on the current stream) for nsteps random-action steps."""
        ms = C.c_float()
        self._check(self._lib.os2r_bench_steps(self._h, int(nsteps), self._stream(), C.byref(ms)), "os2r_bench_steps")
        return float(ms.value)

    def done_reasons(self, on: bool = True):
        """Switch the done-reason output on (include/os2r.h: os2r_set_done_reasons) or off.  While on, `self.reasons`
        ([N] int16: bit d = observation slot d was outside the reset space at the end of the last step) is rewritten by
        every step; -> the tensor (the same one every step) or None."""
        new = torch.zeros(self.N, dtype=torch.int16, device=self.device) if on else None
        torch.cuda.current_stream(self.device).synchronize()
        self._check(self._lib.os2r_set_done_reasons(self._h, _ptr(new)), "os2r_set_done_reasons")
        self.reasons = new
        return new

    def bench_enqueue(self, nsteps: int):
        """Enqueue nsteps random-action steps on the current stream and return at once (no events, no wait): for
        callers that drive several handles on several streams -- shards of one batch advancing independently."""
        self._check(self._lib.os2r_bench_steps(self._h, int(nsteps), self._stream(), None), "os2r_bench_steps")

    @staticmethod
    def bench_enqueue_shards(sims, streams, nsteps: int):
        """Enqueue nsteps random-action steps of every shard `sims[i]` on `streams[i]` (torch streams), round robin and
        without waiting (include/os2r.h: os2r_bench_steps_multi): all the streams start together."""
        hs = (C.c_void_p * len(sims))(*[s._h for s in sims])
        sts = (C.c_void_p * len(sims))(*[C.c_void_p(st.cuda_stream) for st in streams])
        rc = sims[0]._lib.os2r_bench_steps_multi(hs, sts, len(sims), int(nsteps))
        sims[0]._check(rc, "os2r_bench_steps_multi")

    WORK_COUNTERS = ("wave_iterations", "scanned_bodies", "row_bodies", "body_sweeps", "sweeps", "lane_contacts",
                     "live_lane_sweeps", "full_sincos", "exact_solves", "lane_exact_solves")

    def count_work(self, on: bool = True):
        """Switch the counting variant of the step kernel on (include/os2r.h: os2r_set_work_counters) or off.
        While on, `work_counters()` returns what the launches since have added up."""
        new = torch.zeros(len(self.WORK_COUNTERS), dtype=torch.int64, device=self.device) if on else None
        # nothing may still be writing the old buffer, and the handle must stop pointing at it, before it is released
        torch.cuda.current_stream(self.device).synchronize()
        self._check(self._lib.os2r_set_work_counters(self._h, _ptr(new)), "os2r_set_work_counters")
        self._counters = new

    def work_counters(self, clear: bool = True) -> dict:
        if getattr(self, "_counters", None) is None:
            raise Os2rError("work counting is off: call count_work(True) first")
        torch.cuda.current_stream(self.device).synchronize()
        v = self._counters.cpu().tolist()
        if clear:
            self._counters.zero_()
        return dict(zip(self.WORK_COUNTERS, v))

    # -- state ------------------------------------------------------------------------------
    def get_state(self):
        q, qd = self._new(self.nq, self.N), self._new(self.nq, self.N)
        self._check(self._lib.os2r_get_state(self._h, _ptr(q), _ptr(qd), self._stream()), "os2r_get_state")
        return q, qd

    def set_state(self, q=None, qd=None):
        """Set q and / or qd ([nq, N]).  Either way the contact solver's state is cleared (include/os2r.h: a state set from
        outside starts like a reset, also when only one of the two is given): a caller that nudges qd every step gives up the
        warm start of the contact solve -- restore it with set_solver_state() afterwards if the old impulses still apply."""
        q = None if q is None else self._in(q, (self.nq, self.N))
        qd = None if qd is None else self._in(qd, (self.nq, self.N))
        self._check(self._lib.os2r_set_state(self._h, _ptr(q), _ptr(qd), self._stream()), "os2r_set_state")
        torch.cuda.current_stream(self.device).synchronize()  # inputs may be temporaries

    def get_solver_state(self):
        """(lambda [4*nq, N], flags [N] int32 holding the uint32 payload): the impulses that ended every environment's last
        physics iteration and which of them are remembered (include/os2r.h: os2r_get_solver_state)."""
        lam, flags = self._new(4 * self.nq, self.N), self._new(self.N, dtype=torch.int32)
        self._check(self._lib.os2r_get_solver_state(self._h, _ptr(lam), _ptr(flags), self._stream()), "os2r_get_solver_state")
        return lam, flags

    def set_solver_state(self, lam, flags):
        lam = self._in(lam, (4 * self.nq, self.N))
        if not isinstance(flags, torch.Tensor):
            import numpy as np
            flags = torch.from_numpy(np.ascontiguousarray(flags).astype(np.uint32).view(np.int32))
        flags = self._in(flags, (self.N,), torch.int32)
        self._check(self._lib.os2r_set_solver_state(self._h, _ptr(lam), _ptr(flags), self._stream()), "os2r_set_solver_state")
        torch.cuda.current_stream(self.device).synchronize()  # inputs may be temporaries

    def get_action_history(self, which: int):
        out = self._new(2, self.N)
        self._check(self._lib.os2r_get_action_history(self._h, int(which), _ptr(out), self._stream()),
                    "os2r_get_action_history")
        return out

    def set_action_history(self, which: int, value):
        v = self._in(value, (2, self.N))
        self._check(self._lib.os2r_set_action_history(self._h, int(which), _ptr(v), self._stream()),
                    "os2r_set_action_history")
        torch.cuda.current_stream(self.device).synchronize()

    def get_params(self, field: int):
        out = self._new(1 if field == abi.PARAM_GRAVITY else self.nq, self.N)
        self._check(self._lib.os2r_get_params(self._h, int(field), _ptr(out), self._stream()), "os2r_get_params")
        return out

    def set_params(self, field: int, value):
        v = self._in(value, (1 if field == abi.PARAM_GRAVITY else self.nq, self.N))
        self._check(self._lib.os2r_set_params(self._h, int(field), _ptr(v), self._stream()), "os2r_set_params")
        torch.cuda.current_stream(self.device).synchronize()

    def episode_info(self):
        steps = self._new(self.N, dtype=torch.int32)
        epi = self._new(self.N, dtype=torch.int32)   # uint32 payload
        pose = self._new(self.N, dtype=torch.uint8)
        self._check(self._lib.os2r_get_episode_info(self._h, _ptr(steps), _ptr(epi), _ptr(pose), self._stream()),
                    "os2r_get_episode_info")
        return steps, epi, pose

    def set_episode_info(self, steps=None, episode=None, pose=None):
        s = None if steps is None else self._in(steps, (self.N,), torch.int32)
        e = None if episode is None else self._in(episode, (self.N,), torch.int32)
        p = None if pose is None else self._in(pose, (self.N,), torch.uint8)
        self._check(self._lib.os2r_set_episode_info(self._h, _ptr(s), _ptr(e), _ptr(p), self._stream()), "os2r_set_episode_info")
        torch.cuda.current_stream(self.device).synchronize()  # inputs may be temporaries

    # -- checkpoint / resume ----------------------------------------------------------------
    def checkpoint(self) -> dict:
        """Everything that determines the future of this handle, as device tensors (+ the step counter)."""
        q, qd = self.get_state()
        steps, episode, pose = self.episode_info()
        lam, flags = self.get_solver_state()
        return {"q": q, "qd": qd, "solver_lambda": lam, "solver_flags": flags, "hist0": self.get_action_history(0), "hist1": self.get_action_history(1),
                "params": {f: self.get_params(f) for f in (abi.PARAM_MASS_SCALE, abi.PARAM_DAMPING, abi.PARAM_FRICTION,
                                                            abi.PARAM_MU, abi.PARAM_GRAVITY)},
                "steps": steps, "episode": episode, "pose": pose, "step_count": self.step_count}

    def restore(self, ck: dict):
        """Continue from a `checkpoint()` (of this or of another handle with the same configuration)."""
        self.set_state(ck["q"], ck["qd"])
        if "solver_lambda" in ck and "solver_flags" in ck:     # (after set_state, which clears it; a checkpoint written before
            self.set_solver_state(ck["solver_lambda"], ck["solver_flags"])   # ABI 4 has none: the solver starts cold, as after a reset)
        self.set_action_history(0, ck["hist0"]); self.set_action_history(1, ck["hist1"])
        for f, v in ck["params"].items():
            self.set_params(f, v)
        self.set_episode_info(ck["steps"], ck["episode"], ck["pose"])
        self.step_count = ck["step_count"]

    # -- fork / resample -------------------------------------------------------------------
    def copy_envs_from(self, src: "HipSim", index=None, *, state: bool = True, params: bool = True, want_obs: bool = False,
                       check: bool = False):
        """Environment e of this handle becomes environment index[e] of `src` in one launch (include/os2r.h: os2r_copy_envs):
        fork one environment into many, resample a population, permute, or take over a whole batch.
        index: None (the identity map: equal sizes), an int (every environment becomes that one of `src`; the index tensor is
        made once and kept), or an int32 [N] tensor on this device, passed by address; a negative entry keeps the environment
        as it is, and so does an entry >= src.N (check=True looks for those on the host -- one synchronisation -- and raises
        ValueError instead).  state / params: which arrays move (abi.COPY_STATE / abi.COPY_PARAMS); the step counter, the seed
        and env_offset, the task and the solver settings stay this handle's.  `src` may be this handle.  `src` must have
        finished its pending work on another stream before the call; on one stream the order is the call order.
        -> the observation [N, D] of every environment after the copy (want_obs), else None."""
        if not isinstance(src, HipSim):
            raise ValueError(f"copy_envs_from: src must be a HipSim, got {type(src)}")
        if isinstance(index, bool):
            raise ValueError("copy_envs_from: index must be None, an int or an int32 tensor")
        if isinstance(index, int):
            if not 0 <= index < src.N:
                raise ValueError(f"copy_envs_from: environment {index} is not one of the source's {src.N}")
            forks = self.__dict__.setdefault("_fork_index", {})
            if index not in forks:
                forks[index] = torch.full((self.N,), index, dtype=torch.int32, device=self.device)
            index = forks[index]
        elif index is not None:
            self._out(index, (self.N,), torch.int32, "copy_envs_from: index")
            if check and bool((index >= src.N).any().item()):
                raise ValueError(f"copy_envs_from: index holds entries >= the source's {src.N} environments")
        what = (abi.COPY_STATE if state else 0) | (abi.COPY_PARAMS if params else 0)
        obs = self._new(self.N, self.D) if want_obs else None
        self._check(self._lib.os2r_copy_envs(self._h, src._h, _ptr(index), what, _ptr(obs), self._stream()), "os2r_copy_envs")
        return obs

    # -- linearisation ---------------------------------------------------------------------
    def _linearize_eps(self, eps):
        """eps of linearize() -> (eps_q, eps_qd, eps_a) as Python floats, checked."""
        import math
        if eps is None:
            # the textbook central-difference step (cube root of the machine epsilon) for all three: a starting point, not tuned
            # to the robot, the time step or the contact state
            eps = float(torch.finfo(self.dtype).eps) ** (1.0 / 3.0)
        if isinstance(eps, bool):
            raise ValueError("linearize: eps must be a float or a sequence of three floats")
        if isinstance(eps, (int, float)):
            eps = (eps, eps, eps)
        try:
            eps = tuple(float(v) for v in eps)
        except (TypeError, ValueError):
            raise ValueError(f"linearize: eps must be a float or a sequence of three floats, got {type(eps)}") from None
        if len(eps) != 3:
            raise ValueError(f"linearize: eps must hold three values (eps_q, eps_qd, eps_a), got {len(eps)}")
        if not all(math.isfinite(v) and v > 0.0 for v in eps):
            raise ValueError(f"linearize: every eps must be finite and > 0, got {eps}")
        if eps[2] >= 1.0:
            raise ValueError(f"linearize: eps_a (the action step) must be < 1, got {eps[2]}")
        return eps

    def linearize_into(self, actions, eps=None, next_out=None, A_out=None, B_out=None):
        """Allocation-free variant of linearize() writing into caller tensors in the kernel's layout (include/os2r.h:
        os2r_linearize): actions [N, 2], next_out [2nq, N], A_out [2nq, 2nq, N], B_out [2nq, 2, N], the environment index
        fastest; each output may be None, not all three.  Shapes, dtypes, device and contiguity are checked before the library
        is called (it takes addresses)."""
        n2 = 2 * self.nq
        eps = self._linearize_eps(eps)
        if actions is None:
            raise ValueError("linearize: actions are required")
        if next_out is None and A_out is None and B_out is None:
            raise ValueError("linearize: nothing asked for (next, A and B are all off)")
        self._out(actions, (self.N, 2), self.dtype, "linearize: actions")
        self._out(next_out, (n2, self.N), self.dtype, "linearize: next_out")
        self._out(A_out, (n2, n2, self.N), self.dtype, "linearize: A_out")
        self._out(B_out, (n2, 2, self.N), self.dtype, "linearize: B_out")
        self._check(self._lib.os2r_linearize(self._h, _ptr(actions), (C.c_double * 3)(*eps), _ptr(next_out), _ptr(A_out), _ptr(B_out),
                                             self._stream()), "os2r_linearize")

    def linearize(self, actions, eps=None, want_next: bool = True, want_A: bool = True, want_B: bool = True):
        """Finite-difference Jacobians of one env-step about every environment's stored state and `actions` [N, 2], in one
        launch (include/os2r.h: os2r_linearize).  With x = (q, qd) and x' = f(x, a) what step(actions) would leave in
        get_state() (no observation, reward, done or reset; actions clamped to [-1, 1] silently):
        -> (next_q [nq, N], next_qd [nq, N], A [N, 2nq, 2nq] = dx'/dx, B [N, 2nq, 2] = dx'/da), None where not wanted.
        The handle is not advanced or changed in any way.  A and B are permuted views of the kernel's [2nq][.][N] layout: they
        are NOT contiguous (call .contiguous() before handing them to code that needs it); next_q / next_qd are the two halves
        of one [2nq, N] tensor.  eps: a float, or (eps_q [rad], eps_qd [rad/s], eps_a [action units]); central differences,
        one-sided at a torque limit.  The default, torch.finfo(dtype).eps ** (1/3) for all three, is the textbook
        central-difference step and is not tuned: across a change of contact mode the quotient is a secant, whatever eps."""
        n2 = 2 * self.nq
        eps = self._linearize_eps(eps)
        if not (want_next or want_A or want_B):
            raise ValueError("linearize: nothing asked for (next, A and B are all off)")
        a = self._in(actions, (self.N, 2))
        nxt = self._new(n2, self.N) if want_next else None
        ja = self._new(n2, n2, self.N) if want_A else None
        jb = self._new(n2, 2, self.N) if want_B else None
        self.linearize_into(a, eps, nxt, ja, jb)
        return (nxt[:self.nq] if want_next else None, nxt[self.nq:] if want_next else None,
                ja.permute(2, 0, 1) if want_A else None, jb.permute(2, 0, 1) if want_B else None)

    def action_violations_into(self, dst: torch.Tensor, clear: bool = True):
        """Copy the running count of out-of-range caller actions into ``dst`` (one int32/uint32 element,
        device or pinned host memory) on the current stream; nothing waits."""
        self._check(self._lib.os2r_get_action_violations(self._h, C.c_void_p(dst.data_ptr()), 1 if clear else 0,
                                                        self._stream()), "os2r_get_action_violations")

    @property
    def step_count(self) -> int:
        v = C.c_uint64()
        self._check(self._lib.os2r_get_step_count(self._h, C.byref(v)), "os2r_get_step_count")
        return int(v.value)

    @step_count.setter
    def step_count(self, value: int):
        self._check(self._lib.os2r_set_step_count(self._h, int(value)), "os2r_set_step_count")
