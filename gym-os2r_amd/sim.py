"""Thin Python handle over one ``Os2rSim`` of the C-ABI: torch tensors in, torch tensors out.

torch is used only for device memory and the current HIP stream; every call goes straight
to ``libos2r.so``.  All tensors stay on the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib, abi
from ._lib import _PybindLib


class Os2rError(RuntimeError):
    pass


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class HipSim:
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

    # -- LQR gains --------------------------------------------------------------------------
    def _lqr_cost(self, Q, R, what="lqr_gains"):
        """Q [2nq, 2nq] and R [2, 2] of lqr_gains() -> two ctypes double arrays (row-major), checked: host values, finite and
        exactly symmetric (include/os2r.h: os2r_lqr_gains).  `what`: the method the errors name."""
        n = 2 * self.nq
        out = []
        for name, m, k in (("Q", Q, n), ("R", R, 2)):
            try:
                if isinstance(m, torch.Tensor):
                    t = m.detach().to("cpu", torch.float64)
                else:                              # (through numpy: torch would make float32 of a list of Python floats)
                    import numpy as np
                    t = torch.from_numpy(np.array(m, dtype=np.float64))
            except (TypeError, ValueError, RuntimeError):
                raise ValueError(f"{what}: {name} must be a [{k}, {k}] array of numbers, got {type(m)}") from None
            if tuple(t.shape) != (k, k):
                raise ValueError(f"{what}: {name} must have shape ({k}, {k}), got {tuple(t.shape)}")
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"{what}: {name} must be finite")
            if not bool((t == t.T).all()):
                raise ValueError(f"{what}: {name} must be exactly symmetric")
            out.append((C.c_double * (k * k))(*t.reshape(-1).tolist()))
        return out

    def lqr_gains_into(self, A, B, Q, R, *, knots: int = 1, sweeps: int = 1, P_final=None, gains_out=None, P_out=None, flags_out=None,
                       actions=None, obs=None, weights_out=None):
        """Allocation-free variant of lqr_gains() on tensors in the kernel's layout (include/os2r.h: os2r_lqr_gains), the
        trajectory index fastest: with K = knots, L = K M and n = 2nq, A [n, n, L], B [n, 2, L], P_final [n, n, M] or None (Q),
        gains_out [K, 2, n, M], P_out [n, n, M] (may be P_final), flags_out [K, M] uint8, weights_out [K, 2, D+1, M] with
        actions [L, 2] and obs [L, D]; each output may be None, not all of gains_out, P_out and weights_out.  Shapes, dtypes,
        device and contiguity are checked before the library is called (it takes addresses)."""
        n = 2 * self.nq
        K, sweeps = int(knots), int(sweeps)
        if K < 1 or sweeps < 1:
            raise ValueError(f"lqr_gains: knots and sweeps must be >= 1, got {K} and {sweeps}")
        q, r = self._lqr_cost(Q, R)
        if not isinstance(A, torch.Tensor) or A.dim() != 3:
            raise ValueError(f"lqr_gains: A must be a tensor of shape ({n}, {n}, knots * M)")
        L = int(A.shape[2])
        if L < K or L % K:
            raise ValueError(f"lqr_gains: the {L} lanes of A are no multiple of knots = {K}")
        M = L // K
        if gains_out is None and P_out is None and weights_out is None:
            raise ValueError("lqr_gains: nothing asked for (gains, P and weights are all off)")
        if weights_out is not None and (actions is None or obs is None):
            raise ValueError("lqr_gains: weights need actions and obs (the point each knot was linearised about)")
        self._out(A, (n, n, L), self.dtype, "lqr_gains: A")
        self._out(B, (n, 2, L), self.dtype, "lqr_gains: B")
        self._out(P_final, (n, n, M), self.dtype, "lqr_gains: P_final")
        self._out(gains_out, (K, 2, n, M), self.dtype, "lqr_gains: gains_out")
        self._out(P_out, (n, n, M), self.dtype, "lqr_gains: P_out")
        self._out(flags_out, (K, M), torch.uint8, "lqr_gains: flags_out")
        self._out(weights_out, (K, 2, self.D + 1, M), self.dtype, "lqr_gains: weights_out")
        if weights_out is not None:
            self._out(actions, (L, 2), self.dtype, "lqr_gains: actions")
            self._out(obs, (L, self.D), self.dtype, "lqr_gains: obs")
        else:
            actions = obs = None
        if B is None:
            raise ValueError("lqr_gains: B is required")
        self._check(self._lib.os2r_lqr_gains(self._h, K, M, sweeps, _ptr(A), _ptr(B), q, r, _ptr(P_final), _ptr(gains_out), _ptr(P_out),
                                             _ptr(flags_out), _ptr(actions), _ptr(obs), _ptr(weights_out), self._stream()), "os2r_lqr_gains")

    def lqr_gains(self, A, B, Q, R, *, knots: int = 1, sweeps: int = 1, P_final=None, actions=None, obs=None, want_gains: bool = True,
                  want_P: bool = False, want_flags: bool = True, want_weights: bool = False):
        """The backward Riccati recursion of L = knots * M independent LQR problems in one launch (include/os2r.h:
        os2r_lqr_gains; the arithmetic and its order are spelled out there).  A [L, 2nq, 2nq] and B [L, 2nq, 2] as linearize()
        returns them -- permuted views of the kernel's layout are taken without a copy, anything else is copied once --, lane
        k * M + m is knot k of trajectory m (a knot handle filled knot-major by copy_envs).  Q [2nq, 2nq] and R [2, 2]: host
        values, finite, exactly symmetric.  P_final [M, 2nq, 2nq] or None (Q): the cost-to-go behind the last knot.  The knots
        are passed `sweeps` times from the last to the first, P carried across: knots=1 with many sweeps is the stationary
        iteration, several knots with several sweeps the periodic one of a wrapped schedule.
        -> (gains [K, M, 2, 2nq], P [M, 2nq, 2nq], flags [K, M] uint8, weights [M, K, 2, D+1]), None where not wanted; all are
        permuted views of the kernel's layouts.  flags is 1 where a knot's 2 x 2 system R + B'PB was refused (not positive
        definite, or not finite): that knot's gain is 0.  weights (needs actions [L, 2] and obs [L, D], the point each knot was
        linearised about) is the per-environment table rollout_schedule takes for a handle of M environments, holding
        a = a0 - K_k (x - x_k) on the raw observation slots; rollout_schedule's .contiguous() on it is a no-op."""
        n = 2 * self.nq
        K = int(knots)
        if K < 1 or int(sweeps) < 1:
            raise ValueError(f"lqr_gains: knots and sweeps must be >= 1, got {K} and {int(sweeps)}")
        if not (want_gains or want_P or want_weights):
            raise ValueError("lqr_gains: nothing asked for (gains, P and weights are all off)")
        if want_weights and (actions is None or obs is None):
            raise ValueError("lqr_gains: weights need actions and obs (the point each knot was linearised about)")
        self._lqr_cost(Q, R)
        for name, t, w in (("A", A, n), ("B", B, 2)):
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or tuple(t.shape[1:]) != (n, w):
                raise ValueError(f"lqr_gains: {name} must be a tensor of shape (knots * M, {n}, {w}), got "
                                 f"{tuple(getattr(t, 'shape', ())) or type(t)}")
            if t.dtype != self.dtype or t.device != self.device:
                raise ValueError(f"lqr_gains: {name} must be {self.dtype} on {self.device}, got {t.dtype} on {t.device}")
        L = int(A.shape[0])
        if int(B.shape[0]) != L:
            raise ValueError(f"lqr_gains: A has {L} lanes, B {int(B.shape[0])}")
        if L < K or L % K:
            raise ValueError(f"lqr_gains: the {L} lanes of A are no multiple of knots = {K}")
        M = L // K
        a, b = A.permute(1, 2, 0).contiguous(), B.permute(1, 2, 0).contiguous()     # no copy for what linearize() returned
        pf = None
        if P_final is not None:
            pf = self._in(P_final, (M, n, n)).permute(1, 2, 0).contiguous()
        act = ob = None
        if want_weights:
            act, ob = self._in(actions, (L, 2)), self._in(obs, (L, self.D))
        gains = self._new(K, 2, n, M) if want_gains else None
        pout = self._new(n, n, M) if want_P else None
        flags = self._new(K, M, dtype=torch.uint8) if want_flags else None
        wts = self._new(K, 2, self.D + 1, M) if want_weights else None
        self.lqr_gains_into(a, b, Q, R, knots=K, sweeps=sweeps, P_final=pf, gains_out=gains, P_out=pout, flags_out=flags, actions=act,
                            obs=ob, weights_out=wts)
        return (gains.permute(0, 3, 1, 2) if want_gains else None, pout.permute(2, 0, 1) if want_P else None, flags,
                wts.permute(3, 0, 1, 2) if want_weights else None)

    # -- iLQR backward pass -----------------------------------------------------------------
    def _ilqr_scalars(self, mu, alphas, want_weights, what="ilqr_backward"):
        """mu and alphas of ilqr_backward() (the alphas of ilqr_steer()) -> (float, ctypes double array or None), checked.
        `what`: the method the errors name."""
        import math
        try:
            mu = float(mu)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: mu must be a number, got {type(mu)}") from None
        if not math.isfinite(mu) or mu < 0.0:
            raise ValueError(f"{what}: mu must be finite and >= 0, got {mu}")
        if not want_weights:
            return mu, None
        try:
            al = [float(v) for v in (alphas.tolist() if hasattr(alphas, "tolist") else alphas)]
        except (TypeError, ValueError):
            raise ValueError(f"{what}: alphas must be a sequence of numbers, got {type(alphas)}") from None
        if not 1 <= len(al) <= 16:
            raise ValueError(f"{what}: between 1 and 16 alphas, got {len(al)}")
        if not all(math.isfinite(v) for v in al):
            raise ValueError(f"{what}: every alpha must be finite, got {al}")
        return mu, (C.c_double * len(al))(*al)

    def ilqr_backward_into(self, A, B, Q, R, *, knots: int = 1, lx=None, lu=None, mu: float = 0.0, P_final=None, p_final=None,
                           gains_out=None, ff_out=None, P_out=None, p_out=None, flags_out=None, dv_out=None, actions=None, obs=None,
                           alphas=None, weights_out=None, mu_dev=None):
        """Allocation-free variant of ilqr_backward() on tensors in the kernel's layout (include/os2r_control.h:
        os2rc_ilqr_backward), the trajectory index fastest: with K = knots, L = K M and n = 2nq, A [n, n, L], B [n, 2, L],
        lx [n, L], lu [2, L], P_final [n, n, M], p_final [n, M] (each of the four None for its default), gains_out [K, 2, n, M],
        ff_out [K, 2, M], P_out [n, n, M] (may be P_final), p_out [n, M] (may be p_final), flags_out [K, M] uint8,
        dv_out [K, 2, M], weights_out [K, 2, D+1, len(alphas) M] with actions [L, 2], obs [L, D] and alphas; each output may be
        None, not all of them but flags_out.  mu_dev [M]: one mu per trajectory, read on the device (include/os2r_steer.h:
        os2rt_ilqr_backward_mu; mu itself must then be 0).  Shapes, dtypes, device and contiguity are checked before the library is
        called (it takes addresses)."""
        n = 2 * self.nq
        K = int(knots)
        if K < 1:
            raise ValueError(f"ilqr_backward: knots must be >= 1, got {K}")
        q, r = self._lqr_cost(Q, R, "ilqr_backward")
        if not isinstance(A, torch.Tensor) or A.dim() != 3:
            raise ValueError(f"ilqr_backward: A must be a tensor of shape ({n}, {n}, knots * M)")
        L = int(A.shape[2])
        if L < K or L % K:
            raise ValueError(f"ilqr_backward: the {L} lanes of A are no multiple of knots = {K}")
        M = L // K
        if all(t is None for t in (gains_out, ff_out, P_out, p_out, dv_out, weights_out)):
            raise ValueError("ilqr_backward: nothing asked for (gains, ff, P, p, dv and weights are all off)")
        if weights_out is not None and (actions is None or obs is None or alphas is None):
            raise ValueError("ilqr_backward: weights need actions, obs (the point each knot was linearised about) and alphas")
        mu, al = self._ilqr_scalars(mu, alphas, weights_out is not None)
        if mu_dev is not None and mu != 0.0:
            raise ValueError(f"ilqr_backward: mu_dev and a nonzero mu ({mu}) are both given; the regularisation is one or the other")
        self._out(mu_dev, (M,), self.dtype, "ilqr_backward: mu_dev")
        if B is None:
            raise ValueError("ilqr_backward: B is required")
        for t, shape, name in ((A, (n, n, L), "A"), (B, (n, 2, L), "B"), (lx, (n, L), "lx"), (lu, (2, L), "lu"),
                               (P_final, (n, n, M), "P_final"), (p_final, (n, M), "p_final"), (gains_out, (K, 2, n, M), "gains_out"),
                               (ff_out, (K, 2, M), "ff_out"), (P_out, (n, n, M), "P_out"), (p_out, (n, M), "p_out"),
                               (dv_out, (K, 2, M), "dv_out")):
            self._out(t, shape, self.dtype, f"ilqr_backward: {name}")
        self._out(flags_out, (K, M), torch.uint8, "ilqr_backward: flags_out")
        nal = 0
        if weights_out is not None:
            nal = len(al)
            self._out(weights_out, (K, 2, self.D + 1, nal * M), self.dtype, "ilqr_backward: weights_out")
            self._out(actions, (L, 2), self.dtype, "ilqr_backward: actions")
            self._out(obs, (L, self.D), self.dtype, "ilqr_backward: obs")
        else:
            actions = obs = None
        lay = self._layout()
        if mu_dev is not None:
            from . import steer
            lib = steer.load()
            rc = lib.os2rt_ilqr_backward_mu(C.byref(lay), K, M, _ptr(A), _ptr(B), _ptr(lx), _ptr(lu), q, r, _ptr(mu_dev), _ptr(P_final),
                                            _ptr(p_final), _ptr(gains_out), _ptr(ff_out), _ptr(P_out), _ptr(p_out), _ptr(flags_out),
                                            _ptr(dv_out), _ptr(actions), _ptr(obs), al, nal, _ptr(weights_out), self._stream())
            if rc != abi.OK:
                raise Os2rError(f"os2rt_ilqr_backward_mu failed ({rc}): {lib.os2rt_last_error().decode()}")
            return
        from . import control
        lib = control.load()
        rc = lib.os2rc_ilqr_backward(C.byref(lay), K, M, _ptr(A), _ptr(B), _ptr(lx), _ptr(lu), q, r, mu, _ptr(P_final), _ptr(p_final),
                                     _ptr(gains_out), _ptr(ff_out), _ptr(P_out), _ptr(p_out), _ptr(flags_out), _ptr(dv_out), _ptr(actions),
                                     _ptr(obs), al, nal, _ptr(weights_out), self._stream())
        if rc != abi.OK:
            raise Os2rError(f"os2rc_ilqr_backward failed ({rc}): {lib.os2rc_last_error().decode()}")

    def ilqr_backward(self, A, B, Q, R, *, knots, lx=None, lu=None, mu=0.0, P_final=None, p_final=None, actions=None, obs=None,
                      alphas=None, want_gains=True, want_ff=True, want_P=False, want_p=False, want_flags=True, want_dv=True,
                      want_weights=False, mu_dev=None):
        """The backward pass of iLQR for M = L / knots independent trajectories in one launch (include/os2r_control.h:
        os2rc_ilqr_backward; the arithmetic and its order are spelled out there): lqr_gains(sweeps=1) with its affine terms.
        A [L, 2nq, 2nq] and B [L, 2nq, 2] as linearize() returns them (taken without a copy), lane k * M + m knot k of trajectory
        m; lx [L, 2nq] and lu [L, 2] the cost gradients at the knots (None: zeros); Q, R the cost Hessians as in lqr_gains;
        mu >= 0 the control-space regularisation; P_final [M, 2nq, 2nq] (None: Q) and p_final [M, 2nq] (None: zeros) the value
        function behind the last knot.
        -> (gains [K, M, 2, 2nq], ff [K, M, 2], P [M, 2nq, 2nq], p [M, 2nq], flags [K, M] uint8, dv [K, M, 2],
        weights [len(alphas) M, K, 2, D+1]), None where not wanted; all are permuted views of the kernel's layouts.  The control
        law of knot k is a = a_k + alpha ff_k - gains_k (x - x_k); flags is 1 where a knot's regularised 2 x 2 system was refused
        (gains and ff are 0 there); alpha dv[..., 0].sum(0) + alpha^2 dv[..., 1].sum(0) is the model's cost change under step size
        alpha.  weights (needs actions [L, 2], obs [L, D] and alphas) is the per-environment table rollout_schedule takes for a
        handle of len(alphas) M environments, environment i M + m being trajectory m under alphas[i].
        mu_dev [M] (the handle's dtype, on its device, contiguous; mu must then be 0): one mu per trajectory, read on the device
        -- the array ilqr_steer keeps up to date.  Trajectory m gets what mu = mu_dev[m] gives it, bit for bit; a negative or
        non-finite entry runs as 0 with every knot of that trajectory refused (include/os2r_steer.h: os2rt_ilqr_backward_mu)."""
        n = 2 * self.nq
        K = int(knots)
        if K < 1:
            raise ValueError(f"ilqr_backward: knots must be >= 1, got {K}")
        if not (want_gains or want_ff or want_P or want_p or want_dv or want_weights):
            raise ValueError("ilqr_backward: nothing asked for (gains, ff, P, p, dv and weights are all off)")
        if want_weights and (actions is None or obs is None or alphas is None):
            raise ValueError("ilqr_backward: weights need actions, obs (the point each knot was linearised about) and alphas")
        self._lqr_cost(Q, R, "ilqr_backward")
        mu_host, al = self._ilqr_scalars(mu, alphas, want_weights)
        if mu_dev is not None and mu_host != 0.0:
            raise ValueError(f"ilqr_backward: mu_dev and a nonzero mu ({mu_host}) are both given; the regularisation is one or the other")
        for name, t, w in (("A", A, n), ("B", B, 2)):
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or tuple(t.shape[1:]) != (n, w):
                raise ValueError(f"ilqr_backward: {name} must be a tensor of shape (knots * M, {n}, {w}), got "
                                 f"{tuple(getattr(t, 'shape', ())) or type(t)}")
            if t.dtype != self.dtype or t.device != self.device:
                raise ValueError(f"ilqr_backward: {name} must be {self.dtype} on {self.device}, got {t.dtype} on {t.device}")
        L = int(A.shape[0])
        if int(B.shape[0]) != L:
            raise ValueError(f"ilqr_backward: A has {L} lanes, B {int(B.shape[0])}")
        if L < K or L % K:
            raise ValueError(f"ilqr_backward: the {L} lanes of A are no multiple of knots = {K}")
        M = L // K
        self._out(mu_dev, (M,), self.dtype, "ilqr_backward: mu_dev")
        a, b = A.permute(1, 2, 0).contiguous(), B.permute(1, 2, 0).contiguous()     # no copy for what linearize() returned

        def given(t, shape, name, perm):
            if t is None:
                return None
            if (isinstance(t, torch.Tensor) and t.dtype == self.dtype and t.device == self.device and tuple(t.shape) == tuple(shape)
                    and t.permute(*perm).is_contiguous()):
                return t.permute(*perm)          # a permuted view of the kernel's layout (ilqr_line_search's *_view): no copy
            try:
                return self._in(t, shape).permute(*perm).contiguous()
            except ValueError as e:
                raise ValueError(f"ilqr_backward: {name}: {e}") from None
        gx, gu = given(lx, (L, n), "lx", (1, 0)), given(lu, (L, 2), "lu", (1, 0))
        pf, vf = given(P_final, (M, n, n), "P_final", (1, 2, 0)), given(p_final, (M, n), "p_final", (1, 0))
        act = ob = None
        nal = 0
        if want_weights:
            nal = len(al)
            act, ob = given(actions, (L, 2), "actions", (0, 1)), given(obs, (L, self.D), "obs", (0, 1))
        gains = self._new(K, 2, n, M) if want_gains else None
        ff = self._new(K, 2, M) if want_ff else None
        pout = self._new(n, n, M) if want_P else None
        vout = self._new(n, M) if want_p else None
        flags = self._new(K, M, dtype=torch.uint8) if want_flags else None
        dv = self._new(K, 2, M) if want_dv else None
        wts = self._new(K, 2, self.D + 1, nal * M) if want_weights else None
        self.ilqr_backward_into(a, b, Q, R, knots=K, lx=gx, lu=gu, mu=mu, P_final=pf, p_final=vf, gains_out=gains, ff_out=ff, P_out=pout,
                                p_out=vout, flags_out=flags, dv_out=dv, actions=act, obs=ob, alphas=alphas, weights_out=wts, mu_dev=mu_dev)
        return (gains.permute(0, 3, 1, 2) if want_gains else None, ff.permute(0, 2, 1) if want_ff else None,
                pout.permute(2, 0, 1) if want_P else None, vout.permute(1, 0) if want_p else None, flags,
                dv.permute(0, 2, 1) if want_dv else None, wts.permute(3, 0, 1, 2) if want_weights else None)

    # -- iLQR line search ------------------------------------------------------------------
    def ilqr_line_search_into(self, knot_obs, end_obs, actions, target, Q, R, *, cost, choice, done=None, Q_final=None, always=False,
                              act_nom=None, obs_nom=None, end_nom=None, lx=None, lu=None, p_final=None, index=None, cand_cost=None):
        """Allocation-free line search of iLQR on tensors in the kernel's layouts (include/os2r_search.h: os2rs_ilqr_line_search;
        the arithmetic and its order are spelled out there).  With M trajectories (target [M, D]), N = nalpha M candidate lanes
        (lane i M + m: trajectory m under step size i), K knots, L = K M and n = 2nq: knot_obs [K, N, D], end_obs [N, D],
        actions [K, N, 2] and done [K, N] uint8 (or None) are what the candidates' recorded rollout returned; Q, R and Q_final
        (None: Q) host values as in ilqr_backward.  The nominal, updated in place where a trajectory accepted a candidate and left
        alone elsewhere: cost [M] (required; a candidate must lower it unless always=True), act_nom [K, M, 2], obs_nom [K, M, D],
        end_nom [M, D], lx [n, L], lu [2, L], p_final [n, M] (the last three as ilqr_backward_into reads them), each or None.
        Written on every call: choice [M] int32 (the accepted candidate or -1, required), index [L] int32 (what
        copy_envs_from(cand_knots, index) takes on the K M-lane knots handle) and cand_cost [nalpha, M], each or None.  Shapes,
        dtypes, device and contiguity are checked before the library is called (it takes addresses)."""
        what = "ilqr_line_search"
        n, D = 2 * self.nq, self.D
        q, r = self._lqr_cost(Q, R, what)
        qf = None if Q_final is None else self._lqr_cost(Q_final, R, f"{what}: Q_final")[0]
        if not isinstance(target, torch.Tensor) or target.dim() != 2:
            raise ValueError(f"{what}: target must be a tensor of shape (M, {D})")
        if not isinstance(knot_obs, torch.Tensor) or knot_obs.dim() != 3:
            raise ValueError(f"{what}: knot_obs must be a tensor of shape (K, nalpha * M, {D})")
        M, K, N = int(target.shape[0]), int(knot_obs.shape[0]), int(knot_obs.shape[1])
        if M < 1 or K < 1 or N < M or N % M:
            raise ValueError(f"{what}: the {N} candidate lanes of knot_obs [{K} knots] are no multiple of the {M} trajectories of target")
        nal, L = N // M, K * M
        if not 1 <= nal <= 16:
            raise ValueError(f"{what}: between 1 and 16 candidates per trajectory, got {nal}")
        if K * N > 2 ** 31 - 1:
            raise ValueError(f"{what}: {K} knots of {N} candidate lanes exceed what an int32 index addresses")
        if cost is None or choice is None:
            raise ValueError(f"{what}: cost and choice are required")
        for t, shape, name in ((knot_obs, (K, N, D), "knot_obs"), (end_obs, (N, D), "end_obs"), (actions, (K, N, 2), "actions"),
                               (target, (M, D), "target"), (cost, (M,), "cost"), (act_nom, (K, M, 2), "act_nom"),
                               (obs_nom, (K, M, D), "obs_nom"), (end_nom, (M, D), "end_nom"), (lx, (n, L), "lx"), (lu, (2, L), "lu"),
                               (p_final, (n, M), "p_final"), (cand_cost, (nal, M), "cand_cost")):
            self._out(t, shape, self.dtype, f"{what}: {name}")
        self._out(done, (K, N), torch.uint8, f"{what}: done")
        self._out(choice, (M,), torch.int32, f"{what}: choice")
        self._out(index, (L,), torch.int32, f"{what}: index")
        if end_obs is None or actions is None:
            raise ValueError(f"{what}: end_obs and actions are required")
        from . import search
        lib = search.load()
        lay = self._layout()
        rc = lib.os2rs_ilqr_line_search(C.byref(lay), K, M, nal, search.ACCEPT_ALWAYS if always else 0, _ptr(knot_obs), _ptr(end_obs),
                                        _ptr(actions), _ptr(done), _ptr(target), q, r, qf, _ptr(cost), _ptr(act_nom), _ptr(obs_nom),
                                        _ptr(end_nom), _ptr(lx), _ptr(lu), _ptr(p_final), _ptr(choice), _ptr(index), _ptr(cand_cost),
                                        self._stream())
        if rc != abi.OK:
            raise Os2rError(f"os2rs_ilqr_line_search failed ({rc}): {lib.os2rs_last_error().decode()}")

    def ilqr_line_search(self, knot_obs, end_obs, actions, target, Q, R, *, nominal=None, done=None, Q_final=None,
                         want_cand_cost: bool = True):
        """The line search of iLQR for M trajectories in one launch (include/os2r_search.h: os2rs_ilqr_line_search): the cost
        sum_k 1/2 e_k'Q e_k + 1/2 a_k'R a_k + 1/2 e_K'Q_final e_K of every candidate, e the observation minus target on the raw
        slots, one accepted step size per trajectory, and the nominal updated in place where a step was accepted.  knot_obs
        [K, nalpha M, D], end_obs [nalpha M, D], actions [K, nalpha M, 2] and done [K, nalpha M] are what the candidates'
        recorded rollout_schedule returned (knot observations, row K-1 of obs, applied actions, done), target [M, D].
        nominal=None: a new nominal is allocated and every candidate with a finite cost and no episode end is acceptable (with
        one candidate per trajectory, the first nominal's own rollout, this initialises it); a dict: the one an earlier call
        returned, updated in place -- a candidate must lower its trajectory's cost.  The dict holds cost [M], actions [K, M, 2],
        obs [K, M, D], end_obs [M, D], lx [n, K M], lu [2, K M], p_final [n, M] (the kernel's layouts) and lx_view [K M, n],
        lu_view [K M, 2], p_final_view [M, n], permuted views ilqr_backward takes without a copy.
        -> (choice [M] int32: the accepted candidate or -1, index [K M] int32 for knots.copy_envs_from(cand_knots, index),
        cand_cost [nalpha, M] or None, nominal)."""
        what = "ilqr_line_search"
        if not isinstance(target, torch.Tensor) or target.dim() != 2 or not isinstance(knot_obs, torch.Tensor) or knot_obs.dim() != 3:
            raise ValueError(f"{what}: target must be a tensor of shape (M, {self.D}) and knot_obs one of shape (K, nalpha * M, {self.D})")
        M, K, N, n = int(target.shape[0]), int(knot_obs.shape[0]), int(knot_obs.shape[1]), 2 * self.nq
        if M < 1 or K < 1 or N < M or N % M:
            raise ValueError(f"{what}: the {N} candidate lanes of knot_obs [{K} knots] are no multiple of the {M} trajectories of target")
        always = nominal is None
        if always:
            nominal = dict(cost=self._new(M), actions=self._new(K, M, 2), obs=self._new(K, M, self.D), end_obs=self._new(M, self.D),
                           lx=self._new(n, K * M), lu=self._new(2, K * M), p_final=self._new(n, M))
            for name in ("lx", "lu", "p_final"):
                nominal[name + "_view"] = nominal[name].permute(1, 0)
            for t in nominal.values():           # a trajectory none of whose candidates is acceptable keeps zeros, not garbage
                t.zero_()
        elif not isinstance(nominal, dict) or any(k not in nominal for k in ("cost", "actions", "obs", "end_obs", "lx", "lu", "p_final")):
            raise ValueError(f"{what}: nominal must be None or the dict an earlier call returned")
        choice, index = self._new(M, dtype=torch.int32), self._new(K * M, dtype=torch.int32)
        cand_cost = self._new(N // M, M) if want_cand_cost else None
        self.ilqr_line_search_into(knot_obs, end_obs, actions, target, Q, R, cost=nominal["cost"], choice=choice, done=done, Q_final=Q_final,
                                   always=always, act_nom=nominal["actions"], obs_nom=nominal["obs"], end_nom=nominal["end_obs"],
                                   lx=nominal["lx"], lu=nominal["lu"], p_final=nominal["p_final"], index=index, cand_cost=cand_cost)
        return choice, index, cand_cost, nominal

    # -- iLQR line search that steers mu -----------------------------------------------------
    def ilqr_steer_into(self, knot_obs, end_obs, actions, target, Q, R, dv, alphas, *, cost, mu, status, choice, iters=None, done=None,
                        Q_final=None, rule=None, act_nom=None, obs_nom=None, end_nom=None, lx=None, lu=None, p_final=None, index=None,
                        cand_cost=None, **rule_kw):
        """Allocation-free steered line search of iLQR on tensors in the kernel's layouts (include/os2r_steer.h: os2rt_ilqr_steer;
        the arithmetic and its order are spelled out there): ilqr_line_search_into, every argument of which but `always` is
        taken as there, plus, per trajectory and in the same launch, an Armijo test on the predicted change, the update of mu, a
        convergence test and a freeze.  dv [K, 2, M] as ilqr_backward_into wrote it, alphas the candidates' step sizes (host
        values, one per candidate); mu [M] (the handle's dtype), status [M] int32 (0 active, 1 converged, 2 stalled) and iters [M]
        int32 (or None) are read and written.  The rule is a dict and / or keywords over gym_os2r_amd.steer.RULE_DEFAULTS: armijo,
        shrink, grow, mu_floor, mu_start, mu_max, tol.  Shapes, dtypes, device and contiguity are checked before the library is
        called (it takes addresses)."""
        from . import steer
        what = "ilqr_steer"
        n, D = 2 * self.nq, self.D
        q, r = self._lqr_cost(Q, R, what)
        qf = None if Q_final is None else self._lqr_cost(Q_final, R, f"{what}: Q_final")[0]
        the_rule = steer.rule(rule, **rule_kw)
        if not isinstance(target, torch.Tensor) or target.dim() != 2:
            raise ValueError(f"{what}: target must be a tensor of shape (M, {D})")
        if not isinstance(knot_obs, torch.Tensor) or knot_obs.dim() != 3:
            raise ValueError(f"{what}: knot_obs must be a tensor of shape (K, nalpha * M, {D})")
        M, K, N = int(target.shape[0]), int(knot_obs.shape[0]), int(knot_obs.shape[1])
        if M < 1 or K < 1 or N < M or N % M:
            raise ValueError(f"{what}: the {N} candidate lanes of knot_obs [{K} knots] are no multiple of the {M} trajectories of target")
        nal, L = N // M, K * M
        if not 1 <= nal <= 16:
            raise ValueError(f"{what}: between 1 and 16 candidates per trajectory, got {nal}")
        if K * N > 2 ** 31 - 1:
            raise ValueError(f"{what}: {K} knots of {N} candidate lanes exceed what an int32 index addresses")
        al = self._ilqr_scalars(0.0, alphas, True, what)[1]
        if len(al) != nal:
            raise ValueError(f"{what}: {len(al)} alphas for {nal} candidates per trajectory")
        if any(t is None for t in (end_obs, actions, dv, cost, mu, status, choice)):
            raise ValueError(f"{what}: end_obs, actions, dv, cost, mu, status and choice are required")
        for t, shape, name in ((knot_obs, (K, N, D), "knot_obs"), (end_obs, (N, D), "end_obs"), (actions, (K, N, 2), "actions"),
                               (target, (M, D), "target"), (dv, (K, 2, M), "dv"), (cost, (M,), "cost"), (mu, (M,), "mu"),
                               (act_nom, (K, M, 2), "act_nom"), (obs_nom, (K, M, D), "obs_nom"), (end_nom, (M, D), "end_nom"),
                               (lx, (n, L), "lx"), (lu, (2, L), "lu"), (p_final, (n, M), "p_final"), (cand_cost, (nal, M), "cand_cost")):
            self._out(t, shape, self.dtype, f"{what}: {name}")
        self._out(done, (K, N), torch.uint8, f"{what}: done")
        for t, shape, name in ((status, (M,), "status"), (iters, (M,), "iters"), (choice, (M,), "choice"), (index, (L,), "index")):
            self._out(t, shape, torch.int32, f"{what}: {name}")
        lib = steer.load()
        lay = self._layout()
        rc = lib.os2rt_ilqr_steer(C.byref(lay), K, M, nal, _ptr(knot_obs), _ptr(end_obs), _ptr(actions), _ptr(done), _ptr(target), q, r, qf,
                                  _ptr(dv), al, C.byref(the_rule), _ptr(cost), _ptr(act_nom), _ptr(obs_nom), _ptr(end_nom), _ptr(lx), _ptr(lu),
                                  _ptr(p_final), _ptr(mu), _ptr(status), _ptr(iters), _ptr(choice), _ptr(index), _ptr(cand_cost),
                                  self._stream())
        if rc != abi.OK:
            raise Os2rError(f"os2rt_ilqr_steer failed ({rc}): {lib.os2rt_last_error().decode()}")

    def ilqr_steer(self, knot_obs, end_obs, actions, target, Q, R, dv, alphas, *, nominal, done=None, Q_final=None, rule=None,
                   want_cand_cost: bool = True, **rule_kw):
        """The line search of iLQR for M trajectories that also steers every trajectory's regularisation, in one launch
        (include/os2r_steer.h: os2rt_ilqr_steer): ilqr_line_search on the nominal an earlier call returned, with, per trajectory,
        an Armijo test of the actual against the predicted change alpha dv[..., 0].sum(0) + alpha^2 dv[..., 1].sum(0) (rule
        member armijo; 0: none), mu halved after an accepted step and raised after an iteration without one (shrink, grow,
        mu_floor, mu_start, mu_max), a trajectory frozen once a step lowered its cost by no more than tol |cost| (status 1) or
        its mu would pass mu_max (status 2).  dv [K, M, 2] as ilqr_backward returned it (its permuted view of the kernel's layout
        is taken without a copy), alphas the step sizes ilqr_backward made the candidates' table for.  `nominal` is the dict
        ilqr_line_search returned; mu [M] (zeros), status [M] int32 (zeros: active) and iters [M] int32 (zeros) are added to it
        where missing and updated in place like the rest -- nominal["mu"] is what ilqr_backward(mu_dev=...) reads.  No host
        value is read: iterations can be launched back to back.
        -> (choice [M] int32: the accepted candidate or -1, index [K M] int32 for knots.copy_envs_from(cand_knots, index),
        cand_cost [nalpha, M] or None, nominal)."""
        what = "ilqr_steer"
        if not isinstance(target, torch.Tensor) or target.dim() != 2 or not isinstance(knot_obs, torch.Tensor) or knot_obs.dim() != 3:
            raise ValueError(f"{what}: target must be a tensor of shape (M, {self.D}) and knot_obs one of shape (K, nalpha * M, {self.D})")
        M, K, N = int(target.shape[0]), int(knot_obs.shape[0]), int(knot_obs.shape[1])
        if M < 1 or K < 1 or N < M or N % M:
            raise ValueError(f"{what}: the {N} candidate lanes of knot_obs [{K} knots] are no multiple of the {M} trajectories of target")
        if not isinstance(nominal, dict) or any(k not in nominal for k in ("cost", "actions", "obs", "end_obs", "lx", "lu", "p_final")):
            raise ValueError(f"{what}: nominal must be the dict ilqr_line_search (or an earlier call) returned")
        if not isinstance(dv, torch.Tensor) or tuple(dv.shape) != (K, M, 2) or dv.dtype != self.dtype or dv.device != self.device:
            raise ValueError(f"{what}: dv must be a {self.dtype} tensor of shape ({K}, {M}, 2) on {self.device}, as ilqr_backward returns it")
        dv_k = dv.permute(0, 2, 1).contiguous()             # no copy for what ilqr_backward returned
        for name, dtype in (("mu", self.dtype), ("status", torch.int32), ("iters", torch.int32)):
            if nominal.get(name) is None:
                nominal[name] = torch.zeros(M, dtype=dtype, device=self.device)
        choice, index = self._new(M, dtype=torch.int32), self._new(K * M, dtype=torch.int32)
        cand_cost = self._new(N // M, M) if want_cand_cost else None
        self.ilqr_steer_into(knot_obs, end_obs, actions, target, Q, R, dv_k, alphas, cost=nominal["cost"], mu=nominal["mu"],
                             status=nominal["status"], choice=choice, iters=nominal["iters"], done=done, Q_final=Q_final, rule=rule,
                             act_nom=nominal["actions"], obs_nom=nominal["obs"], end_nom=nominal["end_obs"], lx=nominal["lx"],
                             lu=nominal["lu"], p_final=nominal["p_final"], index=index, cand_cost=cand_cost, **rule_kw)
        return choice, index, cand_cost, nominal

    # -- MPPI update ------------------------------------------------------------------------
    def mppi_update_into(self, returns, actions, nominal_in, nominal_out, *, samples: int, temperature: float, shift: int = 1,
                         tail: str = "hold", applied=None, table=None, weights=None, ess=None, count=None):
        """Allocation-free MPPI update on tensors in the kernel's layouts (include/os2r_mppi.h: os2rm_mppi_update; the arithmetic
        and its order are spelled out there).  With S = samples, M robots, N = S M lanes (lane s M + m: sample s of robot m) and K
        knots: returns [N], actions [K, N, 2] and nominal_in [K, M, 2] are read; nominal_out [K, M, 2] (required, another tensor
        than nominal_in), applied [M, 2], table [K, 2, D+1, N] (only its bias entries [:, :, D, :] are written), weights [S, M],
        ess [M] and count [M] int32 are written, each of the last five or None.  temperature > 0 is the softmax temperature of
        the returns (beta = 1 / temperature), shift in 0..K, tail "hold" or "zero".  Shapes, dtypes, device and contiguity are
        checked before the library is called (it takes addresses)."""
        import math
        from . import mppi
        what = "mppi_update"
        if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
            raise ValueError(f"{what}: samples must be an integer >= 1, got {samples!r}")
        try:
            temp = float(temperature)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: temperature must be a number, got {type(temperature)}") from None
        if not math.isfinite(temp) or temp <= 0.0 or not math.isfinite(1.0 / temp):
            raise ValueError(f"{what}: temperature must be finite and > 0, got {temp}")
        if tail not in mppi.TAILS:
            raise ValueError(f"{what}: tail must be 'hold' or 'zero', got {tail!r}")
        if not isinstance(actions, torch.Tensor) or actions.dim() != 3:
            raise ValueError(f"{what}: actions must be a tensor of shape (K, samples * M, 2)")
        K, N, S = int(actions.shape[0]), int(actions.shape[1]), samples
        if K < 1 or N < S or N % S:
            raise ValueError(f"{what}: the {N} lanes of actions [{K} knots] are no multiple of samples = {S}")
        M = N // S
        if isinstance(shift, bool) or not isinstance(shift, int) or not 0 <= shift <= K:
            raise ValueError(f"{what}: shift must be an integer in 0..{K}, got {shift!r}")
        if returns is None or nominal_in is None or nominal_out is None:
            raise ValueError(f"{what}: returns, nominal_in and nominal_out are required")
        for t, shape, name in ((returns, (N,), "returns"), (actions, (K, N, 2), "actions"), (nominal_in, (K, M, 2), "nominal_in"),
                               (nominal_out, (K, M, 2), "nominal_out"), (applied, (M, 2), "applied"),
                               (table, (K, 2, self.D + 1, N), "table"), (weights, (S, M), "weights"), (ess, (M,), "ess")):
            self._out(t, shape, self.dtype, f"{what}: {name}")
        self._out(count, (M,), torch.int32, f"{what}: count")
        if nominal_out.data_ptr() == nominal_in.data_ptr():
            raise ValueError(f"{what}: nominal_out must be another tensor than nominal_in (every slot reads its source slot itself)")
        lib = mppi.load()
        lay = self._layout()
        rc = lib.os2rm_mppi_update(C.byref(lay), K, M, S, _ptr(returns), _ptr(actions), _ptr(nominal_in), 1.0 / temp, shift,
                                   mppi.TAILS[tail], _ptr(nominal_out), _ptr(applied), _ptr(table), _ptr(weights), _ptr(ess), _ptr(count),
                                   self._stream())
        if rc != abi.OK:
            raise Os2rError(f"os2rm_mppi_update failed ({rc}): {lib.os2rm_last_error().decode()}")

    def mppi_update(self, returns, actions, nominal, *, samples: int, temperature: float, shift: int = 1, tail: str = "hold",
                    table=None, want_weights: bool = False, want_ess: bool = False):
        """The MPPI update of M robots in one launch (include/os2r_mppi.h: os2rm_mppi_update): with S = samples and N = S M lanes,
        lane s M + m sample s of robot m -- a planner handle forked by copy_envs_from(real, arange(N) % M) --, returns [N] and
        actions [K, N, 2] are what the noisy rollout_schedule(first_episode=True, want_actions=True) returned and nominal
        [K, M, 2] the nominal its table held.  Every robot's lanes with a finite return are weighted by
        exp((return - max) / temperature); the new nominal is the weighted mean of their action sequences clipped to [-1, 1] (a
        robot without a valid lane keeps its nominal), moved `shift` slots towards the present with the last slot held
        (tail="hold") or zeros behind it (tail="zero").
        table: None (no table), True (this handle's own [N, K, 2, D+1] table, allocated as zeros at the first call and kept) or
        the table an earlier call or ilqr_backward(want_weights=True) returned -- a permuted view of the kernel's
        [K, 2, D+1, N] layout; only its bias entries table[:, :, :, D] are written, to the new nominal of the lane's robot: the
        weights of the next rollout_schedule, which then applies clip(nominal + sigma eps).
        The new nominal is written into one of two buffers the handle keeps for this shape, the one `nominal` is not: feed it
        back and the two alternate.
        -> (applied [M, 2]: slot 0 of the weighted mean, the action for real.step; nominal [K, M, 2]; table [N, K, 2, D+1] | None;
        weights [S, M] | None: the unnormalised weights; ess [M] | None: the effective sample size; count [M] int32: the valid
        lanes of every robot)."""
        what = "mppi_update"
        if not isinstance(actions, torch.Tensor) or actions.dim() != 3:
            raise ValueError(f"{what}: actions must be a tensor of shape (K, samples * M, 2)")
        if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
            raise ValueError(f"{what}: samples must be an integer >= 1, got {samples!r}")
        K, N, S = int(actions.shape[0]), int(actions.shape[1]), samples
        if K < 1 or N < S or N % S:
            raise ValueError(f"{what}: the {N} lanes of actions [{K} knots] are no multiple of samples = {S}")
        M, R = N // S, self.D + 1
        self._out(nominal, (K, M, 2), self.dtype, f"{what}: nominal")
        if nominal is None:
            raise ValueError(f"{what}: nominal is required")
        tab = None
        if table is True:
            tables = self.__dict__.setdefault("_mppi_tables", {})
            if (K, N) not in tables:
                tables[(K, N)] = torch.zeros(K, 2, R, N, dtype=self.dtype, device=self.device)
            tab = tables[(K, N)]
        elif table is not None and table is not False:
            if (not isinstance(table, torch.Tensor) or tuple(table.shape) != (N, K, 2, R) or table.dtype != self.dtype
                    or table.device != self.device or not table.permute(1, 2, 3, 0).is_contiguous()):
                raise ValueError(f"{what}: table must be None, True or a {self.dtype} tensor of shape ({N}, {K}, 2, {R}) on {self.device} "
                                 f"that is a permuted view of the kernel's [K, 2, D+1, N] layout, as an earlier call returned it")
            tab = table.permute(1, 2, 3, 0)
        pair = self.__dict__.setdefault("_mppi_nominals", {})
        if (K, M) not in pair:
            pair[(K, M)] = (self._new(K, M, 2), self._new(K, M, 2))
        out = pair[(K, M)][0] if nominal.data_ptr() != pair[(K, M)][0].data_ptr() else pair[(K, M)][1]
        applied, count = self._new(M, 2), self._new(M, dtype=torch.int32)
        weights = self._new(S, M) if want_weights else None
        ess = self._new(M) if want_ess else None
        self.mppi_update_into(returns, actions, nominal, out, samples=S, temperature=temperature, shift=shift, tail=tail,
                              applied=applied, table=tab, weights=weights, ess=ess, count=count)
        return applied, out, (None if tab is None else tab.permute(3, 0, 1, 2)), weights, ess, count

    # -- particle-filter update -------------------------------------------------------------
    def pf_update_into(self, obs, meas, prec, logw_out, index, *, particles: int, logw_in=None, u=None, resample_ratio: float = 0.5,
                       est=None, weights=None, ess=None, count=None, resampled=None):
        """Allocation-free particle-filter update on tensors in the kernel's layouts (include/os2r_pf.h: os2rp_pf_update; the
        arithmetic and its order are spelled out there).  With S = particles, M robots and N = S M lanes (lane s M + m: particle s
        of robot m): obs [N, D], meas [M, D], prec [D], logw_in [S, M] (None: zeros) and u [M] (None: 0.5) are read; logw_out
        [S, M] (required, another tensor than logw_in), index [N] int32 (required), est [M, D], weights [S, M], ess [M], count [M]
        int32 and resampled [M] int32 are written, each of the last five or None.  resample_ratio is finite and >= 0.  Shapes,
        dtypes, device and contiguity are checked before the library is called (it takes addresses)."""
        import math
        from . import pf
        what = "pf_update"
        if isinstance(particles, bool) or not isinstance(particles, int) or particles < 1:
            raise ValueError(f"{what}: particles must be an integer >= 1, got {particles!r}")
        try:
            ratio = float(resample_ratio)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: resample_ratio must be a number, got {type(resample_ratio)}") from None
        if isinstance(resample_ratio, bool) or not math.isfinite(ratio) or ratio < 0.0:
            raise ValueError(f"{what}: resample_ratio must be finite and >= 0, got {resample_ratio!r}")
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2:
            raise ValueError(f"{what}: obs must be a tensor of shape (particles * M, {self.D})")
        N, S = int(obs.shape[0]), particles
        if N < S or N % S:
            raise ValueError(f"{what}: the {N} lanes of obs are no multiple of particles = {S}")
        M = N // S
        if meas is None or prec is None or logw_out is None or index is None:
            raise ValueError(f"{what}: obs, meas, prec, logw_out and index are required")
        for t, shape, name in ((obs, (N, self.D), "obs"), (meas, (M, self.D), "meas"), (prec, (self.D,), "prec"), (logw_in, (S, M), "logw_in"),
                               (u, (M,), "u"), (logw_out, (S, M), "logw_out"), (est, (M, self.D), "est"), (weights, (S, M), "weights"),
                               (ess, (M,), "ess")):
            self._out(t, shape, self.dtype, f"{what}: {name}")
        for t, shape, name in ((index, (N,), "index"), (count, (M,), "count"), (resampled, (M,), "resampled")):
            self._out(t, shape, torch.int32, f"{what}: {name}")
        if logw_in is not None and logw_out.data_ptr() == logw_in.data_ptr():
            raise ValueError(f"{what}: logw_out must be another tensor than logw_in (the launch keeps the weights in it between its passes)")
        lib = pf.load()
        lay = self._layout()
        rc = lib.os2rp_pf_update(C.byref(lay), M, S, _ptr(obs), _ptr(meas), _ptr(prec), _ptr(logw_in), _ptr(u), ratio, _ptr(logw_out),
                                 _ptr(index), _ptr(est), _ptr(weights), _ptr(ess), _ptr(count), _ptr(resampled), self._stream())
        if rc != abi.OK:
            raise Os2rError(f"os2rp_pf_update failed ({rc}): {lib.os2rp_last_error().decode()}")

    def pf_update(self, obs, meas, prec, *, particles: int, logw=None, u=None, resample_ratio: float = 0.5, want_estimate: bool = True,
                  want_weights: bool = False):
        """The particle-filter update of M robots in one launch (include/os2r_pf.h: os2rp_pf_update): with S = particles and
        N = S M lanes, lane s M + m particle s of robot m -- a particle handle forked by copy_envs_from(real, arange(N) % M) --,
        obs [N, D] is every particle's observation as step, a one-step rollout or copy_envs_from returned it, meas [M, D] the
        measurement of every robot and prec [D] one inverse variance per observation entry (0 drops the entry).  Every particle's
        log-weight is logw [S, M] (None: zeros) minus half its precision-weighted squared distance from the measurement; a
        particle whose log-weight is not finite is invalid and has weight 0.  A robot resamples when its effective sample size
        falls below resample_ratio * S or when it holds an invalid particle: systematic resampling with the offset u [M] in
        [0, 1) (None: 0.5), after which its log-weights are 0.  A robot without a valid particle is lost: nothing moves, its
        log-weights are 0 and its estimate is the measurement.
        The new log-weights are written into one of two buffers the handle keeps for this shape, the one `logw` is not: feed
        them back and the two alternate.
        -> (logw [S, M]: normalised to a maximum of 0, -inf for an invalid particle; index [N] int32 for
        self.copy_envs_from(self, index): the ancestor of every lane, -1 (keep) in the lanes of a robot that did not resample;
        est [M, D] | None: the weighted mean observation; weights [S, M] | None: the unnormalised weights; ess [M]: the effective
        sample size; count [M] int32: the valid particles of every robot; resampled [M] int32: 1 where the robot resampled)."""
        what = "pf_update"
        if isinstance(particles, bool) or not isinstance(particles, int) or particles < 1:
            raise ValueError(f"{what}: particles must be an integer >= 1, got {particles!r}")
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2:
            raise ValueError(f"{what}: obs must be a tensor of shape (particles * M, {self.D})")
        N, S = int(obs.shape[0]), particles
        if N < S or N % S:
            raise ValueError(f"{what}: the {N} lanes of obs are no multiple of particles = {S}")
        M = N // S
        self._out(logw, (S, M), self.dtype, f"{what}: logw")
        pair = self.__dict__.setdefault("_pf_logw", {})
        if (S, M) not in pair:
            pair[(S, M)] = (self._new(S, M), self._new(S, M))
        out = pair[(S, M)][0] if logw is None or logw.data_ptr() != pair[(S, M)][0].data_ptr() else pair[(S, M)][1]
        index = self._new(N, dtype=torch.int32)
        est = self._new(M, self.D) if want_estimate else None
        weights = self._new(S, M) if want_weights else None
        ess, count, resampled = self._new(M), self._new(M, dtype=torch.int32), self._new(M, dtype=torch.int32)
        self.pf_update_into(obs, meas, prec, out, index, particles=S, logw_in=logw, u=u, resample_ratio=resample_ratio, est=est,
                            weights=weights, ess=ess, count=count, resampled=resampled)
        return out, index, est, weights, ess, count, resampled

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
