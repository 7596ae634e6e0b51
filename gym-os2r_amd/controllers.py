"""The controller calls of a HipSim: LQR gains, the iLQR backward pass (plain, with a mu per trajectory, or under box limits on the
actions), its line search with and without a steered mu, the MPPI
update, the cross-entropy update, the particle-filter update, the Kalman filter update, the two calls of the unscented Kalman filter (its sigma points and its update), the
score-function policy gradient, the two calls of the critic (GAE(lambda) and the linear value fit), the clipped-surrogate (PPO) gradient, the natural-gradient step, the two calls of evolution-strategy search (the perturbation and the ARS update), the three of running observation whitening (the statistics, the fold and the gradient back) and the two of system identification (the parameter lanes and the Levenberg-Marquardt update), each as an allocation-free ``*_into`` on tensors in the kernel's layout and an allocating
wrapper around it.  ``Controllers`` is the plain base class HipSim (gym_os2r_amd.sim) inherits them from; it uses the handle's
``_out``, ``_in``, ``_new``, ``_layout``, ``_stream`` and ``_check``.

Every check runs before a library is loaded or called.  What several methods check is written once, in the functions below;
the shape tables stay with their method.  A wrapper repeats a check of its ``*_into`` only where it has to run before the
wrapper permutes, copies or allocates.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import abi, box as box_lib, cem, cma, control, critic, ekf, es, mppi, norm, npg, pf, pg, ppo, search, steer, sysid, ukf
from ._lib import Os2rError, _ptr

NOMINAL_KEYS = ("cost", "actions", "obs", "end_obs", "lx", "lu", "p_final")


def _call(module, entry, last_error, *args):
    """Entry point `entry` of the companion library `module` loads; a status that is not OK raises Os2rError with the library's text."""
    lib = module.load()
    rc = getattr(lib, entry)(*args)
    if rc != abi.OK:
        raise Os2rError(f"{entry} failed ({rc}): {getattr(lib, last_error)().decode()}")


def _split(what, lanes, per, of, unit, ok=True):
    """The `lanes` lanes of `of`, `per` of them (the argument `unit`) to each trajectory or robot -> how many of those there are."""
    if not ok or lanes < per or lanes % per:
        raise ValueError(f"{what}: the {lanes} lanes of {of} are no multiple of {unit} = {per}")
    return lanes // per


def _count(what, name, v):
    """`v` is an integer >= 1 and no bool."""
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"{what}: {name} must be an integer >= 1, got {v!r}")
    return v


def _finite(what, name, v, ok, must, shown=None):
    """float(v), finite and ok(it) -- the error says "finite and `must`" and shows the float, or `shown`."""
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be a number, got {type(v)}") from None
    if not math.isfinite(x) or not ok(x):
        raise ValueError(f"{what}: {name} must be finite and {must}, got {x if shown is None else shown}")
    return x


def _not_negative(x):
    return x >= 0.0


def _invertible(x):
    return x > 0.0 and math.isfinite(1.0 / x)


def _shift(what, shift, K):
    """`shift` of a sampling planner's update with K knots: an integer in 0..K and no bool."""
    if isinstance(shift, bool) or not isinstance(shift, int) or not 0 <= shift <= K:
        raise ValueError(f"{what}: shift must be an integer in 0..{K}, got {shift!r}")
    return shift


def _nominal_dict(what, nominal, wanted):
    """`nominal` is a dict with every entry a line search keeps."""
    if not isinstance(nominal, dict) or any(k not in nominal for k in NOMINAL_KEYS):
        raise ValueError(f"{what}: nominal must be {wanted} returned")


class Controllers:
    """The controller methods of HipSim."""

    def _outs(self, what, rows):
        """self._out for every row (tensor, shape, dtype or None: the handle's, name), the errors naming the method `what`."""
        for t, shape, dtype, name in rows:
            self._out(t, shape, dtype or self.dtype, f"{what}: {name}")

    def _other_buffer(self, kept, shape, t):
        """Of the two buffers of `shape` the handle keeps in its dict `kept`, made at the first call: the one `t` (a tensor or None) is not."""
        pairs = self.__dict__.setdefault(kept, {})
        if shape not in pairs:
            pairs[shape] = (self._new(*shape), self._new(*shape))
        first, second = pairs[shape]
        return first if t is None or t.data_ptr() != first.data_ptr() else second

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

    def _riccati_lanes(self, what, A, K):
        """A [2nq, 2nq, L] of lqr_gains_into / ilqr_backward_into -> (L, M = L / K)."""
        n = 2 * self.nq
        if not isinstance(A, torch.Tensor) or A.dim() != 3:
            raise ValueError(f"{what}: A must be a tensor of shape ({n}, {n}, knots * M)")
        L = int(A.shape[2])
        return L, _split(what, L, K, "A", "knots")

    def _riccati_views(self, what, A, B, K):
        """A [L, 2nq, 2nq] and B [L, 2nq, 2] of lqr_gains / ilqr_backward -> (a, b, L, M = L / K), a and b in the kernel's layout."""
        n = 2 * self.nq
        for name, t, w in (("A", A, n), ("B", B, 2)):
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or tuple(t.shape[1:]) != (n, w):
                raise ValueError(f"{what}: {name} must be a tensor of shape (knots * M, {n}, {w}), got "
                                 f"{tuple(getattr(t, 'shape', ())) or type(t)}")
            if t.dtype != self.dtype or t.device != self.device:
                raise ValueError(f"{what}: {name} must be {self.dtype} on {self.device}, got {t.dtype} on {t.device}")
        L = int(A.shape[0])
        if int(B.shape[0]) != L:
            raise ValueError(f"{what}: A has {L} lanes, B {int(B.shape[0])}")
        M = _split(what, L, K, "A", "knots")
        return A.permute(1, 2, 0).contiguous(), B.permute(1, 2, 0).contiguous(), L, M     # no copy for what linearize() returned

    def lqr_gains_into(self, A, B, Q, R, *, knots: int = 1, sweeps: int = 1, P_final=None, gains_out=None, P_out=None, flags_out=None,
                       actions=None, obs=None, weights_out=None):
        """Allocation-free variant of lqr_gains() on tensors in the kernel's layout (include/os2r.h: os2r_lqr_gains), the
        trajectory index fastest: with K = knots, L = K M and n = 2nq, A [n, n, L], B [n, 2, L], P_final [n, n, M] or None (Q),
        gains_out [K, 2, n, M], P_out [n, n, M] (may be P_final), flags_out [K, M] uint8, weights_out [K, 2, D+1, M] with
        actions [L, 2] and obs [L, D]; each output may be None, not all of gains_out, P_out and weights_out.  Shapes, dtypes,
        device and contiguity are checked before the library is called (it takes addresses)."""
        what = "lqr_gains"
        n = 2 * self.nq
        K, sweeps = int(knots), int(sweeps)
        if K < 1 or sweeps < 1:
            raise ValueError(f"{what}: knots and sweeps must be >= 1, got {K} and {sweeps}")
        q, r = self._lqr_cost(Q, R)
        L, M = self._riccati_lanes(what, A, K)
        if gains_out is None and P_out is None and weights_out is None:
            raise ValueError(f"{what}: nothing asked for (gains, P and weights are all off)")
        if weights_out is not None and (actions is None or obs is None):
            raise ValueError(f"{what}: weights need actions and obs (the point each knot was linearised about)")
        if weights_out is None:
            actions = obs = None
        self._outs(what, ((A, (n, n, L), None, "A"), (B, (n, 2, L), None, "B"), (P_final, (n, n, M), None, "P_final"),
                          (gains_out, (K, 2, n, M), None, "gains_out"), (P_out, (n, n, M), None, "P_out"),
                          (flags_out, (K, M), torch.uint8, "flags_out"), (weights_out, (K, 2, self.D + 1, M), None, "weights_out"),
                          (actions, (L, 2), None, "actions"), (obs, (L, self.D), None, "obs")))
        if B is None:
            raise ValueError(f"{what}: B is required")
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
        what = "lqr_gains"
        n = 2 * self.nq
        K = int(knots)
        if K < 1 or int(sweeps) < 1:                  # (here too: the lanes are split by K below)
            raise ValueError(f"{what}: knots and sweeps must be >= 1, got {K} and {int(sweeps)}")
        if want_weights and (actions is None or obs is None):       # (here too: _in would make a tensor of None)
            raise ValueError(f"{what}: weights need actions and obs (the point each knot was linearised about)")
        a, b, L, M = self._riccati_views(what, A, B, K)
        pfin = None
        if P_final is not None:
            pfin = self._in(P_final, (M, n, n)).permute(1, 2, 0).contiguous()
        act = ob = None
        if want_weights:
            act, ob = self._in(actions, (L, 2)), self._in(obs, (L, self.D))
        gains = self._new(K, 2, n, M) if want_gains else None
        pout = self._new(n, n, M) if want_P else None
        flags = self._new(K, M, dtype=torch.uint8) if want_flags else None
        wts = self._new(K, 2, self.D + 1, M) if want_weights else None
        self.lqr_gains_into(a, b, Q, R, knots=K, sweeps=sweeps, P_final=pfin, gains_out=gains, P_out=pout, flags_out=flags, actions=act,
                            obs=ob, weights_out=wts)
        return (gains.permute(0, 3, 1, 2) if want_gains else None, pout.permute(2, 0, 1) if want_P else None, flags,
                wts.permute(3, 0, 1, 2) if want_weights else None)

    # -- iLQR backward pass -----------------------------------------------------------------
    def _ilqr_scalars(self, mu, alphas, want_weights, what="ilqr_backward"):
        """mu and alphas of ilqr_backward() (the alphas of ilqr_steer()) -> (float, ctypes double array or None), checked.
        `what`: the method the errors name."""
        mu = _finite(what, "mu", mu, _not_negative, ">= 0")
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
                           alphas=None, weights_out=None, mu_dev=None, box=None, clamp_out=None):
        """Allocation-free variant of ilqr_backward() on tensors in the kernel's layout (include/os2r_control.h:
        os2rc_ilqr_backward), the trajectory index fastest: with K = knots, L = K M and n = 2nq, A [n, n, L], B [n, 2, L],
        lx [n, L], lu [2, L], P_final [n, n, M], p_final [n, M] (each of the four None for its default), gains_out [K, 2, n, M],
        ff_out [K, 2, M], P_out [n, n, M] (may be P_final), p_out [n, M] (may be p_final), flags_out [K, M] uint8,
        dv_out [K, 2, M], weights_out [K, 2, D+1, len(alphas) M] with actions [L, 2], obs [L, D] and alphas; each output may be
        None, not all of them but flags_out.  mu_dev [M]: one mu per trajectory, read on the device (include/os2r_steer.h:
        os2rt_ilqr_backward_mu; mu itself must then be 0).  box: None, or True for (-1, 1), or (lo, hi), each a number or a pair of
        numbers, lo -inf or finite in [-1, 1], hi +inf or finite in [-1, 1]: the feed-forward step stays inside the box around the
        clamped nominal, the feedback rows of the clamped components are zero and the value recursion sees both
        (include/os2r_box.h: os2rb_ilqr_backward_box); actions [L, 2] is then required, and clamp_out [K, M] uint8 (or None) takes
        the knots' clamp bytes.  Shapes, dtypes, device and contiguity are checked before the library is called (it takes
        addresses)."""
        what = "ilqr_backward"
        n = 2 * self.nq
        K = int(knots)
        if K < 1:
            raise ValueError(f"{what}: knots must be >= 1, got {K}")
        q, r = self._lqr_cost(Q, R, what)
        L, M = self._riccati_lanes(what, A, K)
        if all(t is None for t in (gains_out, ff_out, P_out, p_out, dv_out, weights_out)):
            raise ValueError(f"{what}: nothing asked for (gains, ff, P, p, dv and weights are all off)")
        if weights_out is not None and (actions is None or obs is None or alphas is None):
            raise ValueError(f"{what}: weights need actions, obs (the point each knot was linearised about) and alphas")
        mu, al = self._ilqr_scalars(mu, alphas, weights_out is not None)
        if mu_dev is not None and mu != 0.0:
            raise ValueError(f"{what}: mu_dev and a nonzero mu ({mu}) are both given; the regularisation is one or the other")
        self._out(mu_dev, (M,), self.dtype, f"{what}: mu_dev")
        if box is None or box is False:
            box = None
            if clamp_out is not None:
                raise ValueError(f"{what}: clamp_out is written by the box-limited pass only (box=...)")
        else:
            lo, hi = box_lib.bounds(box, what)
            if actions is None:
                raise ValueError(f"{what}: box needs actions (the bounds are relative to the nominal actions)")
        if B is None:
            raise ValueError(f"{what}: B is required")
        nal = 0 if al is None else len(al)
        if weights_out is None:
            obs = None
            if box is None:
                actions = None
        self._outs(what, ((A, (n, n, L), None, "A"), (B, (n, 2, L), None, "B"), (lx, (n, L), None, "lx"), (lu, (2, L), None, "lu"),
                          (P_final, (n, n, M), None, "P_final"), (p_final, (n, M), None, "p_final"),
                          (gains_out, (K, 2, n, M), None, "gains_out"), (ff_out, (K, 2, M), None, "ff_out"), (P_out, (n, n, M), None, "P_out"),
                          (p_out, (n, M), None, "p_out"), (dv_out, (K, 2, M), None, "dv_out"), (flags_out, (K, M), torch.uint8, "flags_out"),
                          (weights_out, (K, 2, self.D + 1, nal * M), None, "weights_out"), (actions, (L, 2), None, "actions"),
                          (obs, (L, self.D), None, "obs"), (clamp_out, (K, M), torch.uint8, "clamp_out")))
        # the entry points differ in the regularisation: a host value, or one per trajectory read on the device
        head = (C.byref(self._layout()), K, M, _ptr(A), _ptr(B), _ptr(lx), _ptr(lu), q, r)
        tail = (_ptr(P_final), _ptr(p_final), _ptr(gains_out), _ptr(ff_out), _ptr(P_out), _ptr(p_out), _ptr(flags_out), _ptr(dv_out),
                _ptr(actions), _ptr(obs), al, nal, _ptr(weights_out), self._stream())
        if box is not None:        # ... and in the box: that entry point takes both forms of mu, and the clamp bytes
            _call(box_lib, "os2rb_ilqr_backward_box", "os2rb_last_error", *head, mu, _ptr(mu_dev), lo, hi, *tail[:8], _ptr(clamp_out),
                  *tail[8:])
        elif mu_dev is None:
            _call(control, "os2rc_ilqr_backward", "os2rc_last_error", *head, mu, *tail)
        else:
            _call(steer, "os2rt_ilqr_backward_mu", "os2rt_last_error", *head, _ptr(mu_dev), *tail)

    def ilqr_backward(self, A, B, Q, R, *, knots, lx=None, lu=None, mu=0.0, P_final=None, p_final=None, actions=None, obs=None,
                      alphas=None, want_gains=True, want_ff=True, want_P=False, want_p=False, want_flags=True, want_dv=True,
                      want_weights=False, mu_dev=None, box=None):
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
        non-finite entry runs as 0 with every knot of that trajectory refused (include/os2r_steer.h: os2rt_ilqr_backward_mu).
        box: True for (-1, 1), or (lo, hi), each a number or a pair of numbers: the control-limited pass
        (include/os2r_box.h: os2rb_ilqr_backward_box).  Per knot the feed-forward step is the exact minimum of the model over
        lo <= a_k + ff_k <= hi (a_k clamped to [-1, 1]), the gain rows of the clamped components are zero and the value
        recursion sees both; actions is then required even without want_weights, and the result gains a last member
        clamped [K, M] uint8: bit c set where component c is held at a bound, bit 2 + c where that is the upper one.  Without
        box nothing changes."""
        what = "ilqr_backward"
        n = 2 * self.nq
        K = int(knots)
        if K < 1:                                     # (here too: the lanes are split by K below)
            raise ValueError(f"{what}: knots must be >= 1, got {K}")
        if want_weights and (actions is None or obs is None or alphas is None):      # (here too: the table is sized by the alphas)
            raise ValueError(f"{what}: weights need actions, obs (the point each knot was linearised about) and alphas")
        al = self._ilqr_scalars(mu, alphas, want_weights)[1]
        boxed = box is not None and box is not False
        if boxed:                                     # (here too: before anything is permuted, copied or allocated)
            box_lib.bounds(box, what)
            if actions is None:
                raise ValueError(f"{what}: box needs actions (the bounds are relative to the nominal actions)")
        a, b, L, M = self._riccati_views(what, A, B, K)

        def given(t, shape, name, perm):
            if t is None:
                return None
            if (isinstance(t, torch.Tensor) and t.dtype == self.dtype and t.device == self.device and tuple(t.shape) == tuple(shape)
                    and t.permute(*perm).is_contiguous()):
                return t.permute(*perm)          # a permuted view of the kernel's layout (ilqr_line_search's *_view): no copy
            try:
                return self._in(t, shape).permute(*perm).contiguous()
            except ValueError as e:
                raise ValueError(f"{what}: {name}: {e}") from None
        gx, gu = given(lx, (L, n), "lx", (1, 0)), given(lu, (L, 2), "lu", (1, 0))
        pfin, vf = given(P_final, (M, n, n), "P_final", (1, 2, 0)), given(p_final, (M, n), "p_final", (1, 0))
        act = ob = None
        nal = 0
        if want_weights:
            nal = len(al)
            act, ob = given(actions, (L, 2), "actions", (0, 1)), given(obs, (L, self.D), "obs", (0, 1))
        elif boxed:
            act = given(actions, (L, 2), "actions", (0, 1))
        clamped = self._new(K, M, dtype=torch.uint8) if boxed else None
        gains = self._new(K, 2, n, M) if want_gains else None
        ff = self._new(K, 2, M) if want_ff else None
        pout = self._new(n, n, M) if want_P else None
        vout = self._new(n, M) if want_p else None
        flags = self._new(K, M, dtype=torch.uint8) if want_flags else None
        dv = self._new(K, 2, M) if want_dv else None
        wts = self._new(K, 2, self.D + 1, nal * M) if want_weights else None
        self.ilqr_backward_into(a, b, Q, R, knots=K, lx=gx, lu=gu, mu=mu, P_final=pfin, p_final=vf, gains_out=gains, ff_out=ff, P_out=pout,
                                p_out=vout, flags_out=flags, dv_out=dv, actions=act, obs=ob, alphas=alphas, weights_out=wts, mu_dev=mu_dev,
                                box=box if boxed else None, clamp_out=clamped)
        out = (gains.permute(0, 3, 1, 2) if want_gains else None, ff.permute(0, 2, 1) if want_ff else None,
               pout.permute(2, 0, 1) if want_P else None, vout.permute(1, 0) if want_p else None, flags,
               dv.permute(0, 2, 1) if want_dv else None, wts.permute(3, 0, 1, 2) if want_weights else None)
        return out + (clamped,) if boxed else out

    # -- iLQR line search, plain and steering mu ----------------------------------------------
    def _search_cost(self, what, Q, R, Q_final):
        """Q, R and Q_final (or None) of a line search -> three ctypes double arrays (qf None for None), checked as _lqr_cost checks."""
        q, r = self._lqr_cost(Q, R, what)
        return q, r, None if Q_final is None else self._lqr_cost(Q_final, R, f"{what}: Q_final")[0]

    def _search_geometry(self, what, target, knot_obs, one_refusal=False):
        """target [M, D] and knot_obs [K, nalpha M, D] of a line search -> (M, K, N = nalpha M, nalpha, L = K M), checked;
        `one_refusal`: the allocating forms' wording, one message for the ranks of both."""
        D = self.D
        no_target = not isinstance(target, torch.Tensor) or target.dim() != 2
        no_knots = not isinstance(knot_obs, torch.Tensor) or knot_obs.dim() != 3
        if one_refusal and (no_target or no_knots):
            raise ValueError(f"{what}: target must be a tensor of shape (M, {D}) and knot_obs one of shape (K, nalpha * M, {D})")
        if no_target:
            raise ValueError(f"{what}: target must be a tensor of shape (M, {D})")
        if no_knots:
            raise ValueError(f"{what}: knot_obs must be a tensor of shape (K, nalpha * M, {D})")
        M, K, N = int(target.shape[0]), int(knot_obs.shape[0]), int(knot_obs.shape[1])
        if M < 1 or K < 1 or N < M or N % M:
            raise ValueError(f"{what}: the {N} candidate lanes of knot_obs [{K} knots] are no multiple of the {M} trajectories of target")
        nal = N // M
        if not 1 <= nal <= 16:
            raise ValueError(f"{what}: between 1 and 16 candidates per trajectory, got {nal}")
        if K * N > 2 ** 31 - 1:
            raise ValueError(f"{what}: {K} knots of {N} candidate lanes exceed what an int32 index addresses")
        return M, K, N, nal, K * M

    def _search_rows(self, geometry, knot_obs, end_obs, actions, done, target, cost, act_nom, obs_nom, end_nom, lx, lu, p_final, choice,
                     index, cand_cost):
        """The shape table both line searches share, as a list: ilqr_steer_into appends its own rows."""
        M, K, N, nal, L = geometry
        n, D, u8, i32 = 2 * self.nq, self.D, torch.uint8, torch.int32
        return [(knot_obs, (K, N, D), None, "knot_obs"), (end_obs, (N, D), None, "end_obs"), (actions, (K, N, 2), None, "actions"),
                (target, (M, D), None, "target"), (cost, (M,), None, "cost"), (act_nom, (K, M, 2), None, "act_nom"),
                (obs_nom, (K, M, D), None, "obs_nom"), (end_nom, (M, D), None, "end_nom"), (lx, (n, L), None, "lx"), (lu, (2, L), None, "lu"),
                (p_final, (n, M), None, "p_final"), (cand_cost, (nal, M), None, "cand_cost"), (done, (K, N), u8, "done"),
                (choice, (M,), i32, "choice"), (index, (L,), i32, "index")]

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
        q, r, qf = self._search_cost(what, Q, R, Q_final)
        geometry = M, K, N, nal, L = self._search_geometry(what, target, knot_obs)
        if cost is None or choice is None:
            raise ValueError(f"{what}: cost and choice are required")
        self._outs(what, self._search_rows(geometry, knot_obs, end_obs, actions, done, target, cost, act_nom, obs_nom, end_nom, lx, lu,
                                           p_final, choice, index, cand_cost))
        if end_obs is None or actions is None:
            raise ValueError(f"{what}: end_obs and actions are required")
        _call(search, "os2rs_ilqr_line_search", "os2rs_last_error", C.byref(self._layout()), K, M, nal, search.ACCEPT_ALWAYS if always else 0,
              _ptr(knot_obs), _ptr(end_obs), _ptr(actions), _ptr(done), _ptr(target), q, r, qf, _ptr(cost), _ptr(act_nom), _ptr(obs_nom),
              _ptr(end_nom), _ptr(lx), _ptr(lu), _ptr(p_final), _ptr(choice), _ptr(index), _ptr(cand_cost), self._stream())

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
        M, K, N, nal, L = self._search_geometry(what, target, knot_obs, one_refusal=True)     # (here too: it sizes what is allocated)
        n = 2 * self.nq
        always = nominal is None
        if always:
            nominal = dict(cost=self._new(M), actions=self._new(K, M, 2), obs=self._new(K, M, self.D), end_obs=self._new(M, self.D),
                           lx=self._new(n, L), lu=self._new(2, L), p_final=self._new(n, M))
            for name in ("lx", "lu", "p_final"):
                nominal[name + "_view"] = nominal[name].permute(1, 0)
            for t in nominal.values():           # a trajectory none of whose candidates is acceptable keeps zeros, not garbage
                t.zero_()
        else:
            _nominal_dict(what, nominal, "None or the dict an earlier call")
        choice, index = self._new(M, dtype=torch.int32), self._new(L, dtype=torch.int32)
        cand_cost = self._new(nal, M) if want_cand_cost else None
        self.ilqr_line_search_into(knot_obs, end_obs, actions, target, Q, R, cost=nominal["cost"], choice=choice, done=done, Q_final=Q_final,
                                   always=always, act_nom=nominal["actions"], obs_nom=nominal["obs"], end_nom=nominal["end_obs"],
                                   lx=nominal["lx"], lu=nominal["lu"], p_final=nominal["p_final"], index=index, cand_cost=cand_cost)
        return choice, index, cand_cost, nominal

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
        what = "ilqr_steer"
        q, r, qf = self._search_cost(what, Q, R, Q_final)
        the_rule = steer.rule(rule, **rule_kw)
        geometry = M, K, N, nal, L = self._search_geometry(what, target, knot_obs)
        al = self._ilqr_scalars(0.0, alphas, True, what)[1]
        if len(al) != nal:
            raise ValueError(f"{what}: {len(al)} alphas for {nal} candidates per trajectory")
        if any(t is None for t in (end_obs, actions, dv, cost, mu, status, choice)):
            raise ValueError(f"{what}: end_obs, actions, dv, cost, mu, status and choice are required")
        rows = self._search_rows(geometry, knot_obs, end_obs, actions, done, target, cost, act_nom, obs_nom, end_nom, lx, lu, p_final, choice,
                                 index, cand_cost)
        self._outs(what, rows + [(dv, (K, 2, M), None, "dv"), (mu, (M,), None, "mu"), (status, (M,), torch.int32, "status"),
                                 (iters, (M,), torch.int32, "iters")])
        _call(steer, "os2rt_ilqr_steer", "os2rt_last_error", C.byref(self._layout()), K, M, nal, _ptr(knot_obs), _ptr(end_obs), _ptr(actions),
              _ptr(done), _ptr(target), q, r, qf, _ptr(dv), al, C.byref(the_rule), _ptr(cost), _ptr(act_nom), _ptr(obs_nom), _ptr(end_nom),
              _ptr(lx), _ptr(lu), _ptr(p_final), _ptr(mu), _ptr(status), _ptr(iters), _ptr(choice), _ptr(index), _ptr(cand_cost),
              self._stream())

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
        M, K, N, nal, L = self._search_geometry(what, target, knot_obs, one_refusal=True)     # (here too: it sizes what is allocated)
        _nominal_dict(what, nominal, "the dict ilqr_line_search (or an earlier call)")
        # (dv arrives as the [K, M, 2] view ilqr_backward returned, not in the layout ilqr_steer_into checks: its own refusal)
        if not isinstance(dv, torch.Tensor) or tuple(dv.shape) != (K, M, 2) or dv.dtype != self.dtype or dv.device != self.device:
            raise ValueError(f"{what}: dv must be a {self.dtype} tensor of shape ({K}, {M}, 2) on {self.device}, as ilqr_backward returns it")
        dv_k = dv.permute(0, 2, 1).contiguous()             # no copy for what ilqr_backward returned
        for name, dtype in (("mu", self.dtype), ("status", torch.int32), ("iters", torch.int32)):
            if nominal.get(name) is None:
                nominal[name] = torch.zeros(M, dtype=dtype, device=self.device)
        choice, index = self._new(M, dtype=torch.int32), self._new(L, dtype=torch.int32)
        cand_cost = self._new(nal, M) if want_cand_cost else None
        self.ilqr_steer_into(knot_obs, end_obs, actions, target, Q, R, dv_k, alphas, cost=nominal["cost"], mu=nominal["mu"],
                             status=nominal["status"], choice=choice, iters=nominal["iters"], done=done, Q_final=Q_final, rule=rule,
                             act_nom=nominal["actions"], obs_nom=nominal["obs"], end_nom=nominal["end_obs"], lx=nominal["lx"],
                             lu=nominal["lu"], p_final=nominal["p_final"], index=index, cand_cost=cand_cost, **rule_kw)
        return choice, index, cand_cost, nominal

    # -- MPPI update ------------------------------------------------------------------------
    def _mppi_lanes(self, what, actions, S):
        """actions [K, S M, 2] of an MPPI update with S samples per robot -> (K, N = S M, M), checked."""
        if not isinstance(actions, torch.Tensor) or actions.dim() != 3:
            raise ValueError(f"{what}: actions must be a tensor of shape (K, samples * M, 2)")
        K, N = int(actions.shape[0]), int(actions.shape[1])
        return K, N, _split(what, N, S, f"actions [{K} knots]", "samples", ok=K >= 1)

    def _planner_table(self, what, kept, table, K, N):
        """`table` of a sampling planner's update -> the table in the kernel's [K, 2, D+1, N] layout, or None: None or False (no
        table), True (this handle's own, allocated as zeros at the first call and kept in its dict `kept`) or the [N, K, 2, D+1]
        view an earlier call returned."""
        R = self.D + 1
        if table is True:
            tables = self.__dict__.setdefault(kept, {})
            if (K, N) not in tables:
                tables[(K, N)] = torch.zeros(K, 2, R, N, dtype=self.dtype, device=self.device)
            return tables[(K, N)]
        if table is None or table is False:
            return None
        if (not isinstance(table, torch.Tensor) or tuple(table.shape) != (N, K, 2, R) or table.dtype != self.dtype
                or table.device != self.device or not table.permute(1, 2, 3, 0).is_contiguous()):
            raise ValueError(f"{what}: table must be None, True or a {self.dtype} tensor of shape ({N}, {K}, 2, {R}) on {self.device} "
                             f"that is a permuted view of the kernel's [K, 2, D+1, N] layout, as an earlier call returned it")
        return table.permute(1, 2, 3, 0)

    def mppi_update_into(self, returns, actions, nominal_in, nominal_out, *, samples: int, temperature: float, shift: int = 1,
                         tail: str = "hold", applied=None, table=None, weights=None, ess=None, count=None):
        """Allocation-free MPPI update on tensors in the kernel's layouts (include/os2r_mppi.h: os2rm_mppi_update; the arithmetic
        and its order are spelled out there).  With S = samples, M robots, N = S M lanes (lane s M + m: sample s of robot m) and K
        knots: returns [N], actions [K, N, 2] and nominal_in [K, M, 2] are read; nominal_out [K, M, 2] (required, another tensor
        than nominal_in), applied [M, 2], table [K, 2, D+1, N] (only its bias entries [:, :, D, :] are written), weights [S, M],
        ess [M] and count [M] int32 are written, each of the last five or None.  temperature > 0 is the softmax temperature of
        the returns (beta = 1 / temperature), shift in 0..K, tail "hold" or "zero".  Shapes, dtypes, device and contiguity are
        checked before the library is called (it takes addresses)."""
        what = "mppi_update"
        S = _count(what, "samples", samples)
        temp = _finite(what, "temperature", temperature, _invertible, "> 0")
        if tail not in mppi.TAILS:
            raise ValueError(f"{what}: tail must be 'hold' or 'zero', got {tail!r}")
        K, N, M = self._mppi_lanes(what, actions, S)
        _shift(what, shift, K)
        if returns is None or nominal_in is None or nominal_out is None:
            raise ValueError(f"{what}: returns, nominal_in and nominal_out are required")
        self._outs(what, ((returns, (N,), None, "returns"), (actions, (K, N, 2), None, "actions"), (nominal_in, (K, M, 2), None, "nominal_in"),
                          (nominal_out, (K, M, 2), None, "nominal_out"), (applied, (M, 2), None, "applied"),
                          (table, (K, 2, self.D + 1, N), None, "table"), (weights, (S, M), None, "weights"), (ess, (M,), None, "ess"),
                          (count, (M,), torch.int32, "count")))
        if nominal_out.data_ptr() == nominal_in.data_ptr():
            raise ValueError(f"{what}: nominal_out must be another tensor than nominal_in (every slot reads its source slot itself)")
        _call(mppi, "os2rm_mppi_update", "os2rm_last_error", C.byref(self._layout()), K, M, S, _ptr(returns), _ptr(actions), _ptr(nominal_in),
              1.0 / temp, shift, mppi.TAILS[tail], _ptr(nominal_out), _ptr(applied), _ptr(table), _ptr(weights), _ptr(ess), _ptr(count),
              self._stream())

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
        S = _count(what, "samples", samples)
        K, N, M = self._mppi_lanes(what, actions, S)                      # (here too, both: they size what is allocated)
        self._out(nominal, (K, M, 2), self.dtype, f"{what}: nominal")
        if nominal is None:
            raise ValueError(f"{what}: nominal is required")
        tab = self._planner_table(what, "_mppi_tables", table, K, N)
        out = self._other_buffer("_mppi_nominals", (K, M, 2), nominal)
        applied, count = self._new(M, 2), self._new(M, dtype=torch.int32)
        weights = self._new(S, M) if want_weights else None
        ess = self._new(M) if want_ess else None
        self.mppi_update_into(returns, actions, nominal, out, samples=S, temperature=temperature, shift=shift, tail=tail,
                              applied=applied, table=tab, weights=weights, ess=ess, count=count)
        return applied, out, (None if tab is None else tab.permute(3, 0, 1, 2)), weights, ess, count

    # -- cross-entropy update ---------------------------------------------------------------
    def _cem_scalars(self, what, elites, S, gain, sigma_gain, sigma_min, sigma_max, tail):
        """The host values of a cross-entropy update -> (E, gain, sigma_gain, sigma_min, sigma_max), checked."""
        E = _count(what, "elites", elites)
        if E > S:
            raise ValueError(f"{what}: elites must be <= samples = {S}, got {E}")
        step = lambda x: 0.0 < x <= 1.0
        g, sg = _finite(what, "gain", gain, step, "in (0, 1]"), _finite(what, "sigma_gain", sigma_gain, step, "in (0, 1]")
        lo = _finite(what, "sigma_min", sigma_min, _not_negative, ">= 0")
        hi = _finite(what, "sigma_max", sigma_max, lambda x: x >= lo, f">= sigma_min = {lo}")
        if tail not in cem.TAILS:
            raise ValueError(f"{what}: tail must be 'hold' or 'zero', got {tail!r}")
        return E, g, sg, lo, hi

    def cem_update_into(self, returns, actions, nominal_in, sigma_in, nominal_out, var_out, sigma_out, *, samples: int, elites: int,
                        gain: float = 1.0, sigma_gain: float = 1.0, sigma_min: float = 0.0, sigma_max: float = 1.0, shift: int = 1,
                        tail: str = "hold", applied=None, table=None, lane_sigma=None, elite=None, threshold=None, count=None):
        """Allocation-free cross-entropy update on tensors in the kernel's layouts (include/os2r_cem.h: os2rx_cem_update; the
        arithmetic and its order are spelled out there).  With S = samples, E = elites, M robots, N = S M lanes (lane s M + m:
        sample s of robot m) and K knots: returns [N], actions [K, N, 2], nominal_in [K, M, 2] and sigma_in [2, M] are read;
        nominal_out [K, M, 2] (required, another tensor than nominal_in), var_out [K, M, 2] (required, the elite variance of every
        knot and the workspace of the pooling), sigma_out [2, M] (required; may be sigma_in), applied [M, 2], table
        [K, 2, D+1, N] (only its bias entries [:, :, D, :] are written), lane_sigma [2, N], elite [S, M] int32, threshold [M] and
        count [M] int32 are written, each of the last six or None.  gain and sigma_gain in (0, 1], 0 <= sigma_min <= sigma_max,
        shift in 0..K, tail "hold" or "zero".  Shapes, dtypes, device and contiguity are checked before the library is called (it
        takes addresses)."""
        what = "cem_update"
        S, i32 = _count(what, "samples", samples), torch.int32
        E, g, sg, lo, hi = self._cem_scalars(what, elites, S, gain, sigma_gain, sigma_min, sigma_max, tail)
        K, N, M = self._mppi_lanes(what, actions, S)
        _shift(what, shift, K)
        if any(t is None for t in (returns, nominal_in, sigma_in, nominal_out, var_out, sigma_out)):
            raise ValueError(f"{what}: returns, nominal_in, sigma_in, nominal_out, var_out and sigma_out are required")
        self._outs(what, ((returns, (N,), None, "returns"), (actions, (K, N, 2), None, "actions"), (nominal_in, (K, M, 2), None, "nominal_in"),
                          (sigma_in, (2, M), None, "sigma_in"), (nominal_out, (K, M, 2), None, "nominal_out"),
                          (var_out, (K, M, 2), None, "var_out"), (sigma_out, (2, M), None, "sigma_out"), (applied, (M, 2), None, "applied"),
                          (table, (K, 2, self.D + 1, N), None, "table"), (lane_sigma, (2, N), None, "lane_sigma"),
                          (elite, (S, M), i32, "elite"), (threshold, (M,), None, "threshold"), (count, (M,), i32, "count")))
        if nominal_out.data_ptr() == nominal_in.data_ptr():
            raise ValueError(f"{what}: nominal_out must be another tensor than nominal_in (a knot is written into another slot than its own)")
        if any(var_out.data_ptr() == t.data_ptr() for t in (returns, actions, nominal_in, sigma_in)):
            raise ValueError(f"{what}: var_out must be a tensor of its own (the pooling reads it after every knot has written it)")
        _call(cem, "os2rx_cem_update", "os2rx_last_error", C.byref(self._layout()), K, M, S, E, _ptr(returns), _ptr(actions), _ptr(nominal_in),
              _ptr(sigma_in), g, sg, lo, hi, shift, cem.TAILS[tail], _ptr(nominal_out), _ptr(var_out), _ptr(sigma_out), _ptr(applied),
              _ptr(table), _ptr(lane_sigma), _ptr(elite), _ptr(threshold), _ptr(count), self._stream())

    def cem_update(self, returns, actions, nominal, sigma, *, samples: int, elites: int, gain: float = 1.0, sigma_gain: float = 1.0,
                   sigma_min: float = 0.0, sigma_max: float = 1.0, shift: int = 1, tail: str = "hold", table=None,
                   want_elite: bool = False, want_variance: bool = True):
        """The cross-entropy update of M robots in one call (include/os2r_cem.h: os2rx_cem_update): with S = samples and N = S M
        lanes, lane s M + m sample s of robot m -- a planner handle forked by copy_envs_from(real, arange(N) % M) --, returns [N]
        and actions [K, N, 2] are what the noisy rollout_schedule(first_episode=True, want_actions=True) returned, nominal
        [K, M, 2] the nominal its table held and sigma [M, 2] the width it sampled with.  Of every robot's lanes with a finite
        return the best `elites` are kept (equal returns: the lower sample first); the nominal moves by `gain` towards the mean
        of their action sequences and is clipped to [-1, 1], the width moves by `sigma_gain` towards their standard deviation
        pooled over the knots and is clamped to [sigma_min, sigma_max]; a robot without a valid lane keeps both.  The nominal is
        moved `shift` slots towards the present with the last slot held (tail="hold") or zeros behind it (tail="zero"): shift=0
        between the iterations of one control step, shift=1 at its last.
        table: None, True or an earlier call's table, as mppi_update takes it; only its bias entries are written.  sigma as an
        earlier call returned it goes on without a copy.  The new nominal is written into one of two buffers the handle keeps
        for this shape, the one `nominal` is not: feed it back and the two alternate.
        -> (applied [M, 2]: knot 0 of the new mean, the action for real.step; nominal [K, M, 2]; table [N, K, 2, D+1] | None;
        sigma [M, 2]; lane_sigma [N, 2]: sigma of every lane's robot, what rollout_schedule(sigma=...) takes without a copy;
        var [K, M, 2] | None: the elite variance of every knot; elite [S, M] int32 | None: 1 for an elite lane; threshold [M]:
        the lowest elite return; count [M] int32: the valid lanes of every robot).  sigma and lane_sigma are transposed views of
        the [2, M] and [2, N] buffers the kernel wrote."""
        what = "cem_update"
        S = _count(what, "samples", samples)
        self._cem_scalars(what, elites, S, gain, sigma_gain, sigma_min, sigma_max, tail)    # (here too: before anything is allocated)
        K, N, M = self._mppi_lanes(what, actions, S)                      # (and these: they size what is allocated)
        self._out(nominal, (K, M, 2), self.dtype, f"{what}: nominal")
        if nominal is None or sigma is None:
            raise ValueError(f"{what}: nominal and sigma are required")
        sig_in = self._kernel_view(what, sigma, (M, 2), "sigma", (1, 0))
        tab = self._planner_table(what, "_cem_tables", table, K, N)
        out = self._other_buffer("_cem_nominals", (K, M, 2), nominal)
        applied, var, sig, lane = self._new(M, 2), self._new(K, M, 2), self._new(2, M), self._new(2, N)
        elite = self._new(S, M, dtype=torch.int32) if want_elite else None
        threshold, count = self._new(M), self._new(M, dtype=torch.int32)
        self.cem_update_into(returns, actions, nominal, sig_in, out, var, sig, samples=S, elites=elites, gain=gain, sigma_gain=sigma_gain,
                             sigma_min=sigma_min, sigma_max=sigma_max, shift=shift, tail=tail, applied=applied, table=tab, lane_sigma=lane,
                             elite=elite, threshold=threshold, count=count)
        return (applied, out, (None if tab is None else tab.permute(3, 0, 1, 2)), sig.t(), lane.t(), var if want_variance else None, elite,
                threshold, count)

    # -- particle-filter update -------------------------------------------------------------
    def _pf_lanes(self, what, obs, S):
        """obs [S M, D] of a particle-filter update with S particles per robot -> (N = S M, M), checked."""
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2:
            raise ValueError(f"{what}: obs must be a tensor of shape (particles * M, {self.D})")
        N = int(obs.shape[0])
        return N, _split(what, N, S, "obs", "particles")

    def pf_update_into(self, obs, meas, prec, logw_out, index, *, particles: int, logw_in=None, u=None, resample_ratio: float = 0.5,
                       est=None, weights=None, ess=None, count=None, resampled=None):
        """Allocation-free particle-filter update on tensors in the kernel's layouts (include/os2r_pf.h: os2rp_pf_update; the
        arithmetic and its order are spelled out there).  With S = particles, M robots and N = S M lanes (lane s M + m: particle s
        of robot m): obs [N, D], meas [M, D], prec [D], logw_in [S, M] (None: zeros) and u [M] (None: 0.5) are read; logw_out
        [S, M] (required, another tensor than logw_in), index [N] int32 (required), est [M, D], weights [S, M], ess [M], count [M]
        int32 and resampled [M] int32 are written, each of the last five or None.  resample_ratio is finite and >= 0.  Shapes,
        dtypes, device and contiguity are checked before the library is called (it takes addresses)."""
        what = "pf_update"
        S, D, i32 = _count(what, "particles", particles), self.D, torch.int32
        # (a bool is no ratio: refused in the words of a value that is not finite)
        ratio = _finite(what, "resample_ratio", math.nan if isinstance(resample_ratio, bool) else resample_ratio, _not_negative, ">= 0",
                        repr(resample_ratio))
        N, M = self._pf_lanes(what, obs, S)
        if meas is None or prec is None or logw_out is None or index is None:
            raise ValueError(f"{what}: obs, meas, prec, logw_out and index are required")
        self._outs(what, ((obs, (N, D), None, "obs"), (meas, (M, D), None, "meas"), (prec, (D,), None, "prec"), (logw_in, (S, M), None, "logw_in"),
                          (u, (M,), None, "u"), (logw_out, (S, M), None, "logw_out"), (est, (M, D), None, "est"),
                          (weights, (S, M), None, "weights"), (ess, (M,), None, "ess"), (index, (N,), i32, "index"), (count, (M,), i32, "count"),
                          (resampled, (M,), i32, "resampled")))
        if logw_in is not None and logw_out.data_ptr() == logw_in.data_ptr():
            raise ValueError(f"{what}: logw_out must be another tensor than logw_in (the launch keeps the weights in it between its passes)")
        _call(pf, "os2rp_pf_update", "os2rp_last_error", C.byref(self._layout()), M, S, _ptr(obs), _ptr(meas), _ptr(prec), _ptr(logw_in), _ptr(u),
              ratio, _ptr(logw_out), _ptr(index), _ptr(est), _ptr(weights), _ptr(ess), _ptr(count), _ptr(resampled), self._stream())

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
        S = _count(what, "particles", particles)
        N, M = self._pf_lanes(what, obs, S)                               # (here too, both: they size what is allocated)
        self._out(logw, (S, M), self.dtype, f"{what}: logw")              # (and logw here: its address picks the buffer)
        out = self._other_buffer("_pf_logw", (S, M), logw)
        index = self._new(N, dtype=torch.int32)
        est = self._new(M, self.D) if want_estimate else None
        weights = self._new(S, M) if want_weights else None
        ess, count, resampled = self._new(M), self._new(M, dtype=torch.int32), self._new(M, dtype=torch.int32)
        self.pf_update_into(obs, meas, prec, out, index, particles=S, logw_in=logw, u=u, resample_ratio=resample_ratio, est=est,
                            weights=weights, ess=ess, count=count, resampled=resampled)
        return out, index, est, weights, ess, count, resampled

    # -- Kalman filter update ---------------------------------------------------------------
    def _ekf_scalars(self, what, A, Q, gate):
        """A, Q and gate of a Kalman filter update -> (q as a ctypes double array or None, gate as a float), checked: A needs Q,
        which is checked as lqr_gains checks its Q; without A, Q is not read."""
        if A is not None and Q is None:
            raise ValueError(f"{what}: A needs Q (the process noise of the covariance prediction)")
        q = None if A is None else self._lqr_cost(Q, [[1.0, 0.0], [0.0, 1.0]], what)[0]
        # (a bool is no gate: refused in the words of a value that is not finite)
        return q, _finite(what, "gate", math.nan if isinstance(gate, bool) else gate, _not_negative, ">= 0", repr(gate))

    def ekf_update_into(self, x_pred, P_in, meas, prec, x_out, P_out, *, A=None, Q=None, gate: float = 0.0, nis=None, used=None,
                        refused=None, innov=None):
        """Allocation-free Kalman filter update on tensors in the kernel's layouts (include/os2r_ekf.h: os2re_ekf_update; the
        arithmetic and its order are spelled out there), the robot index fastest.  With M = x_pred.shape[1] robots (it need not
        be the handle's N) and n = 2nq: x_pred [n, M], P_in [n, n, M] (its upper triangle), A [n, n, M] (None: no covariance
        prediction), meas [M, D] and prec [D] are read; x_out [n, M] (required; may be x_pred) and P_out [n, n, M] (required; may be
        P_in), nis [M], used [M] int32, refused [M] int32 and innov [M, D] are written, each of the last four or None.  Q [n, n]
        (host values, finite, exactly symmetric; needed with A) is the process noise, gate finite and >= 0 (0: none).  Shapes,
        dtypes, device and contiguity are checked before the library is called (it takes addresses)."""
        what = "ekf_update"
        n, D, i32 = 2 * self.nq, self.D, torch.int32
        q, gate = self._ekf_scalars(what, A, Q, gate)
        if not isinstance(x_pred, torch.Tensor) or x_pred.dim() != 2 or int(x_pred.shape[1]) < 1:
            raise ValueError(f"{what}: x_pred must be a tensor of shape ({n}, M)")
        M = int(x_pred.shape[1])
        if P_in is None or meas is None or prec is None or x_out is None or P_out is None:
            raise ValueError(f"{what}: x_pred, P_in, meas, prec, x_out and P_out are required")
        self._outs(what, ((x_pred, (n, M), None, "x_pred"), (P_in, (n, n, M), None, "P_in"), (A, (n, n, M), None, "A"),
                          (meas, (M, D), None, "meas"), (prec, (D,), None, "prec"), (x_out, (n, M), None, "x_out"),
                          (P_out, (n, n, M), None, "P_out"), (nis, (M,), None, "nis"), (innov, (M, D), None, "innov"),
                          (used, (M,), i32, "used"), (refused, (M,), i32, "refused")))
        _call(ekf, "os2re_ekf_update", "os2re_last_error", C.byref(self._layout()), M, _ptr(x_pred), _ptr(P_in), _ptr(A), q, _ptr(meas),
              _ptr(prec), gate, _ptr(x_out), _ptr(P_out), _ptr(nis), _ptr(used), _ptr(refused), _ptr(innov), self._stream())

    def ekf_update(self, x_pred, P, meas, prec, *, A=None, Q=None, gate: float = 0.0, want_innov: bool = False):
        """The Kalman filter update of M robots in one launch (include/os2r_ekf.h: os2re_ekf_update): the covariance prediction
        P- = A P A' + Q, then the measurement update of state and covariance against meas [M, D], one raw observation slot after
        the other -- the slot d shows state column slot_col[d] with the variance 1 / prec[d]; an entry of meas that is not finite
        is a reading that did not arrive, an entry of prec that is not > 0 drops the slot.  The sequence gives the joint update
        of the textbook.  On an estimate handle, est.linearize(action) -> ekf_update -> est.set_state(x[:nq], x[nq:]) is one
        step of an extended Kalman filter for every environment.
        x_pred [2nq, M]: the predicted state, or the pair (next_q, next_qd) as linearize() returned it -- the two halves of one
        tensor, taken without a copy; A [M, 2nq, 2nq] as linearize() returned it (None: no prediction, P- = P) and P [M, 2nq, 2nq]
        as an earlier call returned it are permuted views of the kernel's layout and go on without a copy, anything else is
        converted and copied once; only the upper triangle of P is read.  Q [2nq, 2nq]: host values, finite, exactly symmetric
        (needed with A).  gate (0: none): a slot whose normalised innovation squared exceeds it is left out for that robot.
        The new covariance is written into one of two buffers the handle keeps for this shape, the one `P` is not in: feed it
        back and the two alternate.
        -> (x [2nq, M]: x[:nq] and x[nq:] are what set_state takes; P [M, 2nq, 2nq]; nis [M]: the normalised innovation squared
        of the applied slots, summed; used [M] int32: bit d set for each slot applied; refused [M] int32: bit d set for each slot
        whose innovation variance was not positive and finite; innov [M, D] | None: the innovation of every applied slot, 0
        elsewhere)."""
        what = "ekf_update"
        n, D = 2 * self.nq, self.D
        self._ekf_scalars(what, A, Q, gate)                                   # (here too: before anything is copied or allocated)
        if isinstance(x_pred, (tuple, list)) and len(x_pred) == 2 and all(isinstance(t, torch.Tensor) and t.dim() == 2 for t in x_pred):
            top, bottom = x_pred
            if (top.dtype == self.dtype and top.device == self.device and top.is_contiguous() and bottom.is_contiguous()
                    and tuple(top.shape) == tuple(bottom.shape) and int(top.shape[0]) == self.nq and bottom.dtype == top.dtype
                    and bottom.data_ptr() == top.data_ptr() + top.numel() * top.element_size()):
                x_pred = top.as_strided((n, int(top.shape[1])), (int(top.shape[1]), 1))     # linearize()'s own [2nq, N] tensor
            else:
                x_pred = torch.cat((top, bottom))
        if not isinstance(x_pred, torch.Tensor) or x_pred.dim() != 2 or int(x_pred.shape[1]) < 1:
            raise ValueError(f"{what}: x_pred must be a tensor of shape ({n}, M), or the pair (next_q, next_qd) of linearize()")
        M = int(x_pred.shape[1])

        def given(t, shape, name, perm):
            if t is None:
                return None
            if (isinstance(t, torch.Tensor) and t.dtype == self.dtype and t.device == self.device and tuple(t.shape) == tuple(shape)
                    and t.permute(*perm).is_contiguous()):
                return t.permute(*perm)          # a permuted view of the kernel's layout: no copy
            try:
                return self._in(t, shape).permute(*perm).contiguous()
            except (ValueError, TypeError, RuntimeError) as e:
                raise ValueError(f"{what}: {name}: {e}") from None
        if P is None:
            raise ValueError(f"{what}: P is required")
        p_in, a = given(P, (M, n, n), "P", (1, 2, 0)), given(A, (M, n, n), "A", (1, 2, 0))
        p_out = self._other_buffer("_ekf_covariances", (n, n, M), p_in)
        x_out, nis = self._new(n, M), self._new(M)
        used, refused = self._new(M, dtype=torch.int32), self._new(M, dtype=torch.int32)
        innov = self._new(M, D) if want_innov else None
        self.ekf_update_into(x_pred, p_in, meas, prec, x_out, p_out, A=a, Q=Q, gate=gate, nis=nis, used=used, refused=refused, innov=innov)
        return x_out, p_out.permute(2, 0, 1), nis, used, refused, innov

    # -- unscented Kalman filter: sigma points and update ---------------------------------------
    def _ukf_weights(self, what, alpha, beta, kappa):
        """gym_os2r_amd.ukf.weights for this handle's 2nq states -> (gamma, wm0, wc0, wi), its refusals naming the method `what`."""
        try:
            return ukf.weights(2 * self.nq, alpha, beta, kappa)
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None

    def _kernel_view(self, what, t, shape, name, perm):
        """`t` of `shape` as the kernel takes it, `perm` applied: a permuted view of the kernel's layout goes on without a copy,
        anything else is converted and copied once; None stays None."""
        if t is None:
            return None
        if (isinstance(t, torch.Tensor) and t.dtype == self.dtype and t.device == self.device and tuple(t.shape) == tuple(shape)
                and t.permute(*perm).is_contiguous()):
            return t.permute(*perm)
        try:
            return self._in(t, shape).permute(*perm).contiguous()
        except (ValueError, TypeError, RuntimeError) as e:
            raise ValueError(f"{what}: {name}: {e}") from None

    def ukf_points_into(self, x, P, points_out, *, failed=None, alpha: float = 1.0, beta: float = 2.0, kappa: float = 0.0):
        """Allocation-free sigma points on tensors in the kernel's layouts (include/os2r_ukf.h: os2ru_ukf_points; the arithmetic
        and its order are spelled out there), the robot index fastest.  With M = x.shape[1] robots (it need not be the handle's
        N), n = 2nq and S = 2n + 1: x [n, M] and P [n, n, M] (its upper triangle) are read; points_out [n, S M] (required; lane
        s M + m is point s of robot m) and failed [M] int32 (or None: 0, or j + 1 where the Cholesky factor failed at column j --
        all points of that robot are x) are written.  alpha, beta, kappa: gym_os2r_amd.ukf.weights.  Shapes, dtypes, device and
        contiguity are checked before the library is called (it takes addresses)."""
        what = "ukf_points"
        n = 2 * self.nq
        S = ukf.npoints(self.nq)
        gamma = self._ukf_weights(what, alpha, beta, kappa)[0]
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or int(x.shape[1]) < 1:
            raise ValueError(f"{what}: x must be a tensor of shape ({n}, M)")
        M = int(x.shape[1])
        if P is None or points_out is None:
            raise ValueError(f"{what}: x, P and points_out are required")
        self._outs(what, ((x, (n, M), None, "x"), (P, (n, n, M), None, "P"), (points_out, (n, S * M), None, "points_out"),
                          (failed, (M,), torch.int32, "failed")))
        _call(ukf, "os2ru_ukf_points", "os2ru_last_error", C.byref(self._layout()), M, _ptr(x), _ptr(P), gamma, _ptr(points_out), _ptr(failed),
              self._stream())

    def ukf_points(self, x, P, *, alpha: float = 1.0, beta: float = 2.0, kappa: float = 0.0, want_failed: bool = True):
        """The 2n + 1 sigma points of M robots in one launch (include/os2r_ukf.h: os2ru_ukf_points): a Cholesky factor L of every
        robot's P, then x, x + gamma L[:, j] and x - gamma L[:, j].  x [2nq, M]; P [M, 2nq, 2nq] -- what ukf_update returned
        is a permuted view of the kernel's layout and goes on without a copy, anything else is converted and copied once; only
        its upper triangle is read.  alpha, beta, kappa: gym_os2r_amd.ukf.weights (the defaults give gamma = sqrt(2nq)).
        -> (points [2nq, S M] with S = 4nq + 1, lane s M + m point s of robot m: points[:nq] and points[nq:] are what
        set_state takes on a sigma handle of S M lanes forked by copy_envs_from(real, arange(S M) % M); failed [M] int32 | None:
        0, or j + 1 where the factor met a pivot that is not positive and finite at column j -- that robot's points all equal x)."""
        what = "ukf_points"
        n = 2 * self.nq
        self._ukf_weights(what, alpha, beta, kappa)                           # (here too: before anything is copied or allocated)
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or int(x.shape[1]) < 1:
            raise ValueError(f"{what}: x must be a tensor of shape ({n}, M)")
        M = int(x.shape[1])
        if P is None:
            raise ValueError(f"{what}: P is required")
        p = self._kernel_view(what, P, (M, n, n), "P", (1, 2, 0))
        points = self._new(n, ukf.npoints(self.nq) * M)
        failed = self._new(M, dtype=torch.int32) if want_failed else None
        self.ukf_points_into(x, p, points, failed=failed, alpha=alpha, beta=beta, kappa=kappa)
        return points, failed

    def _ukf_state(self, what, state, meas):
        """state, the pair (q, qd) of get_state() on the sigma handle, and meas [M, D] of an unscented update -> (q, qd, M, lanes)."""
        S = ukf.npoints(self.nq)
        if not (isinstance(state, (tuple, list)) and len(state) == 2 and all(isinstance(t, torch.Tensor) and t.dim() == 2 for t in state)):
            raise ValueError(f"{what}: state must be the pair (q, qd) of get_state(), two tensors of shape ({self.nq}, {S} * M)")
        if not isinstance(meas, torch.Tensor) or meas.dim() != 2 or int(meas.shape[0]) < 1:
            raise ValueError(f"{what}: meas must be a tensor of shape (M, {self.D})")
        M, lanes = int(meas.shape[0]), int(state[0].shape[1])
        _split(what, lanes, S, f"state [{M} robots in meas]", "points", ok=lanes == S * M)
        return state[0], state[1], M, lanes

    def ukf_update_into(self, state, P_in, meas, prec, x_out, P_out, *, Q, done=None, gate: float = 0.0, alpha: float = 1.0,
                        beta: float = 2.0, kappa: float = 0.0, nis=None, used=None, refused=None, innov=None, lost=None, points_out=None,
                        failed=None):
        """Allocation-free unscented Kalman filter update on tensors in the kernel's layouts (include/os2r_ukf.h:
        os2ru_ukf_update; the arithmetic and its order are spelled out there), the robot index fastest.  With M = meas.shape[0]
        robots (it need not be the handle's N), n = 2nq and S = 2n + 1: state, the pair (q, qd) as get_state() returned it on the
        sigma handle after its step ([nq, S M] each, taken as they are), done [S M] uint8 (that step's flags, or None),
        P_in [n, n, M] (its upper triangle; used for lost robots only), meas [M, D] and prec [D] are read; x_out [n, M] (required),
        P_out [n, n, M] (required; may be P_in), nis [M], used [M] int32, refused [M] int32, innov [M, D], lost [M] int32,
        points_out [n, S M] (the sigma points of the result) and failed [M] int32 (only with points_out) are written, each of the
        last seven or None.  Q [n, n] (host values, finite, exactly symmetric) is the additive process noise, gate finite and
        >= 0 (0: none), alpha, beta, kappa: gym_os2r_amd.ukf.weights.  Shapes, dtypes, device and contiguity are checked before the
        library is called (it takes addresses)."""
        what = "ukf_update"
        n, D, i32 = 2 * self.nq, self.D, torch.int32
        nq, S = self.nq, ukf.npoints(self.nq)
        if Q is None:
            raise ValueError(f"{what}: Q is required (the additive process noise)")
        q_host, gate = self._ekf_scalars(what, True, Q, gate)
        gamma, wm0, wc0, wi = self._ukf_weights(what, alpha, beta, kappa)
        q, qd, M, lanes = self._ukf_state(what, state, meas)
        if P_in is None or prec is None or x_out is None or P_out is None:
            raise ValueError(f"{what}: state, P_in, meas, prec, x_out and P_out are required")
        if failed is not None and points_out is None:
            raise ValueError(f"{what}: failed needs points_out (it is the verdict on their Cholesky factor)")
        self._outs(what, ((q, (nq, lanes), None, "state[0]"), (qd, (nq, lanes), None, "state[1]"), (done, (lanes,), torch.uint8, "done"),
                          (P_in, (n, n, M), None, "P_in"), (meas, (M, D), None, "meas"), (prec, (D,), None, "prec"),
                          (x_out, (n, M), None, "x_out"), (P_out, (n, n, M), None, "P_out"), (nis, (M,), None, "nis"),
                          (innov, (M, D), None, "innov"), (used, (M,), i32, "used"), (refused, (M,), i32, "refused"), (lost, (M,), i32, "lost"),
                          (points_out, (n, lanes), None, "points_out"), (failed, (M,), i32, "failed")))
        _call(ukf, "os2ru_ukf_update", "os2ru_last_error", C.byref(self._layout()), M, _ptr(q), _ptr(qd), _ptr(done), _ptr(P_in), q_host, gamma,
              wm0, wc0, wi, _ptr(meas), _ptr(prec), gate, _ptr(x_out), _ptr(P_out), _ptr(nis), _ptr(used), _ptr(refused), _ptr(innov),
              _ptr(lost), _ptr(points_out), _ptr(failed), self._stream())

    def ukf_update(self, state, P, meas, prec, *, Q, done=None, gate: float = 0.0, alpha: float = 1.0, beta: float = 2.0, kappa: float = 0.0,
                   want_innov: bool = False, want_points: bool = True):
        """The unscented Kalman filter update of M robots in one launch (include/os2r_ukf.h: os2ru_ukf_update).  On a sigma
        handle of S M lanes (S = 4nq + 1, forked by copy_envs_from(real, arange(S M) % M)),
        sig.set_state(points[:nq], points[nq:]) -> sig.step(action tiled S times) -> sig.get_state() -> ukf_update is one filter
        step for every robot, and needs no Jacobian.  state: the pair (q, qd) get_state() returned, taken without a copy; done: the
        step's done flags [S M] uint8 (None: none).  The mean and covariance of every robot's propagated points are formed with the
        weights of gym_os2r_amd.ukf.weights(2nq, alpha, beta, kappa) and Q [2nq, 2nq] (host values, finite, exactly symmetric) is
        added; then the measurement update of ekf_update against meas [M, D] with prec [D] and gate.  A robot one of whose lanes
        is done or not finite is lost: its x is point 0 and its covariance the P it came with.  P [M, 2nq, 2nq] as an earlier call
        returned it is a permuted view of the kernel's layout and goes on without a copy, anything else is converted and copied
        once.  The new covariance is written into one of two buffers the handle keeps for this shape, the one `P` is not in: feed
        it back and the two alternate.
        -> (x [2nq, M]; P [M, 2nq, 2nq]; nis [M]; used [M] int32; refused [M] int32; innov [M, D] | None; lost [M] int32: 1 where
        the robot was lost; points [2nq, S M] | None: the sigma points of the new (x, P), what the next set_state takes;
        failed [M] int32 | None: as ukf_points returns it, with the points)."""
        what = "ukf_update"
        n, D, S = 2 * self.nq, self.D, ukf.npoints(self.nq)
        if Q is None:
            raise ValueError(f"{what}: Q is required (the additive process noise)")
        self._ekf_scalars(what, True, Q, gate)                                # (here too: before anything is copied or allocated)
        self._ukf_weights(what, alpha, beta, kappa)
        q, qd, M, lanes = self._ukf_state(what, state, meas)                  # (and M: it sizes what is allocated)
        if P is None:
            raise ValueError(f"{what}: P is required")
        p_in = self._kernel_view(what, P, (M, n, n), "P", (1, 2, 0))
        p_out = self._other_buffer("_ukf_covariances", (n, n, M), p_in)
        x_out, nis = self._new(n, M), self._new(M)
        used, refused, lost = (self._new(M, dtype=torch.int32) for _ in range(3))
        innov = self._new(M, D) if want_innov else None
        points = self._new(n, lanes) if want_points else None
        failed = self._new(M, dtype=torch.int32) if want_points else None
        self.ukf_update_into((q, qd), p_in, meas, prec, x_out, p_out, Q=Q, done=done, gate=gate, alpha=alpha, beta=beta, kappa=kappa, nis=nis,
                             used=used, refused=refused, innov=innov, lost=lost, points_out=points, failed=failed)
        return x_out, p_out.permute(2, 0, 1), nis, used, refused, innov, lost, points, failed

    # -- score-function policy gradient -----------------------------------------------------
    def _pg_lanes(self, what, obs, policies):
        """obs [K, S P, D] of a policy gradient with P = policies -> (K, N = S P, S, P), checked."""
        P = _count(what, "policies", policies)
        if not isinstance(obs, torch.Tensor) or obs.dim() != 3:
            raise ValueError(f"{what}: obs must be a tensor of shape (K, samples * policies, {self.D})")
        K, N = int(obs.shape[0]), int(obs.shape[1])
        if not 1 <= K <= 65535:
            raise ValueError(f"{what}: obs must hold 1..65535 steps, got {K}")
        S = _split(what, N, P, f"obs [{K} steps]", "policies")
        if N > 2 ** 31 - 1 or S * K > 2 ** 31 - 1:
            raise ValueError(f"{what}: {N} lanes, or {S} samples of {K} steps, exceed what an int32 holds")
        return K, N, S, P

    def _pg_weight(self, what, adv, rewards, done, gamma, baseline, rtg):
        """The two ways a policy gradient is given its weight -> gamma as a float, checked: adv or rewards, not both; rewards with
        done; baseline and the reward-to-go with rewards only."""
        if (adv is None) == (rewards is None):
            raise ValueError(f"{what}: the weight is adv (one number per lane) or rewards (with done), one or the other")
        if rewards is not None and done is None:
            raise ValueError(f"{what}: rewards need done (an episode's end cuts the reward-to-go)")
        if rewards is None and (baseline is not None or rtg):
            raise ValueError(f"{what}: baseline and the reward-to-go need rewards")
        return _finite(what, "gamma", math.nan if isinstance(gamma, bool) else gamma, lambda x: 0.0 <= x <= 1.0, "in [0, 1]", repr(gamma))

    def policy_gradient_into(self, obs, noise, sigma, grad, lane_grad, lane_count, *, policies: int = 1, obs0=None, actions=None,
                             tanh: bool = False, length=None, adv=None, rewards=None, done=None, gamma: float = 1.0, baseline=None,
                             lsig_grad=None, lane_lsig=None, steps=None, clipped=None, valid=None, rtg=None):
        """Allocation-free policy gradient on tensors in the kernel's layouts (include/os2r_pg.h: os2rg_policy_gradient; the
        arithmetic and its order are spelled out there).  With P = policies, S samples, N = S P lanes (lane s P + p: sample s of
        policy p) and K steps: obs [K, N, D], obs0 [N, D] (None: obs[k] is what step k's action saw), noise [K, N, 2], actions
        [K, N, 2] (required unless tanh), sigma [2] or [2, N], length [N] int32 (None: K) and the weight -- adv [N], or rewards
        [K, N] with done [K, N] uint8, gamma in [0, 1] and baseline [K, P] or None -- are read; grad [2, D+1, P], lane_grad
        [2, D+1, N] and lane_count [4, N] int32 (all three required), lsig_grad [2, P] with lane_lsig [2, N], steps [P] int32,
        clipped [2, P] int32, valid [P] int32 and rtg [K, N] (with rewards) are written, each of the last six or None.  Shapes,
        dtypes, device, contiguity, alignment and overlap are checked before the library is called (it takes addresses)."""
        what = "policy_gradient"
        K, N, S, P = self._pg_lanes(what, obs, policies)
        g = self._pg_weight(what, adv, rewards, done, gamma, baseline, rtg is not None)
        D, i32 = self.D, torch.int32
        if any(t is None for t in (noise, sigma, grad, lane_grad, lane_count)):
            raise ValueError(f"{what}: obs, noise, sigma, grad, lane_grad and lane_count are required")
        if not tanh and actions is None:
            raise ValueError(f"{what}: actions are required unless tanh (where the clip bound, a step adds nothing)")
        if (lsig_grad is None) != (lane_lsig is None):
            raise ValueError(f"{what}: lsig_grad and lane_lsig go together (the second launch reads the one to write the other)")
        if tanh:
            actions = None
        if rewards is None:
            done = None
        per_lane = isinstance(sigma, torch.Tensor) and sigma.dim() == 2
        inputs = ((obs, (K, N, D), None, "obs"), (obs0, (N, D), None, "obs0"), (noise, (K, N, 2), None, "noise"),
                  (actions, (K, N, 2), None, "actions"), (sigma, (2, N) if per_lane else (2,), None, "sigma"), (length, (N,), i32, "length"),
                  (adv, (N,), None, "adv"), (rewards, (K, N), None, "rewards"), (done, (K, N), torch.uint8, "done"),
                  (baseline, (K, P), None, "baseline"))
        outputs = ((grad, (2, D + 1, P), None, "grad"), (lane_grad, (2, D + 1, N), None, "lane_grad"), (lsig_grad, (2, P), None, "lsig_grad"),
                   (lane_lsig, (2, N), None, "lane_lsig"), (steps, (P,), i32, "steps"), (clipped, (2, P), i32, "clipped"),
                   (valid, (P,), i32, "valid"), (rtg, (K, N), None, "rtg"), (lane_count, (pg.LANE_COUNTS, N), i32, "lane_count"))
        self._outs(what, inputs + outputs)
        for t, name in ((noise, "noise"), (actions, "actions")):
            if t is not None and t.data_ptr() % (2 * t.element_size()):
                raise ValueError(f"{what}: {name} must be aligned to a pair of its elements")
        spans = [(name, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t, _, _, name in inputs + outputs if t is not None]
        first_output = sum(t is not None for t, _, _, _ in inputs)
        for o in range(first_output, len(spans)):         # every output against every input and every output before it
            name, lo, hi = spans[o]
            for other, lo2, hi2 in spans[:o]:
                if lo < hi2 and lo2 < hi:
                    raise ValueError(f"{what}: {name} overlaps {other} (an output shares no memory with an input or another output)")
        _call(pg, "os2rg_policy_gradient", "os2rg_last_error", C.byref(self._layout()), K, P, S,
              (pg.TANH if tanh else 0) | (pg.SIGMA_PER_LANE if per_lane else 0), _ptr(obs), _ptr(obs0), _ptr(noise), _ptr(actions), _ptr(sigma),
              _ptr(length), _ptr(adv), _ptr(rewards), _ptr(done), g, _ptr(baseline), _ptr(grad), _ptr(lane_grad), _ptr(lsig_grad),
              _ptr(lane_lsig), _ptr(steps), _ptr(clipped), _ptr(valid), _ptr(rtg), _ptr(lane_count), self._stream())

    def policy_gradient(self, obs, noise, sigma, *, policies: int = 1, obs0=None, actions=None, tanh: bool = False, length=None, adv=None,
                        rewards=None, done=None, gamma: float = 1.0, baseline=None, want_log_sigma: bool = False, want_lane: bool = False,
                        want_rtg: bool = False):
        """The score-function (REINFORCE) gradient of P = policies linear-Gaussian policies in one call (include/os2r_pg.h:
        os2rg_policy_gradient): with S samples and N = S P lanes, lane s P + p sample s of policy p -- the order
        copy_envs_from(real, arange(N) % P) forks in --, obs [K, N, D], actions [K, N, 2], noise [K, N, 2] and length [N] are what
        the noisy rollout_policy(first_episode=True, want_outputs=True, want_actions=True, want_noise=True) returned and sigma (a
        float, [2] or [N, 2]) what it sampled with; all are taken without a copy.  obs0 [N, D]: what reset() or the previous
        window's last step returned, the observation step 0 saw; None with obs the knot observations of a recorded rollout
        (want_knot_obs), which already are what every step saw.  Step k of a lane counts while k < length; its score is
        eps / sigma [x; 1] on the action components where sigma > 0 and -- unless tanh -- the clip did not bind.  The weight of
        a step is adv [N], one number per lane, or the discounted reward-to-go of rewards [K, N] cut at done [K, N] with gamma
        in [0, 1], minus baseline [K, P] where given.  A lane one of whose sums is not finite is left out of its policy's sums.
        -> (grad [P, 2, D+1]: the sum over the policy's valid lanes, a permuted view of the kernel's layout -- with P = N what
        rollout_policy takes as per-environment weights without a copy; steps [P] int32: the counted steps; clipped [P, 2]
        int32: how often the clip bound; valid [P] int32: the valid lanes; lsig_grad [P, 2] | None: the gradient with respect to
        log sigma; lane_grad [N, 2, D+1] | None: the per-lane sums; rtg [K, N] | None: the reward-to-go)."""
        what = "policy_gradient"
        K, N, S, P = self._pg_lanes(what, obs, policies)                    # (here too, all: they size what is allocated)
        self._pg_weight(what, adv, rewards, done, gamma, baseline, want_rtg)
        if isinstance(sigma, bool) or sigma is None:
            raise ValueError(f"{what}: sigma must be a float, a [2] tensor or an [{N}, 2] tensor, got {sigma!r}")
        if isinstance(sigma, (int, float)):
            sigma = torch.full((2,), float(sigma), dtype=self.dtype, device=self.device)
        elif isinstance(sigma, torch.Tensor) and sigma.dim() == 2:
            sigma = self._kernel_view(what, sigma, (N, 2), "sigma", (1, 0))  # the [2, N] an [N, 2] sigma is a view of goes on as it is
        D, i32 = self.D, torch.int32
        grad, lane, count = self._new(2, D + 1, P), self._new(2, D + 1, N), self._new(pg.LANE_COUNTS, N, dtype=i32)
        steps, clipped, valid = self._new(P, dtype=i32), self._new(2, P, dtype=i32), self._new(P, dtype=i32)
        lsig = self._new(2, P) if want_log_sigma else None
        lane_lsig = self._new(2, N) if want_log_sigma else None
        rtg = self._new(K, N) if want_rtg else None
        self.policy_gradient_into(obs, noise, sigma, grad, lane, count, policies=P, obs0=obs0, actions=actions, tanh=tanh, length=length,
                                  adv=adv, rewards=rewards, done=done, gamma=gamma, baseline=baseline, lsig_grad=lsig, lane_lsig=lane_lsig,
                                  steps=steps, clipped=clipped, valid=valid, rtg=rtg)
        return (grad.permute(2, 0, 1), steps, clipped.t(), valid, None if lsig is None else lsig.t(),
                lane.permute(2, 0, 1) if want_lane else None, rtg)

    # -- the critic: GAE(lambda) and the linear value fit -----------------------------------
    def _no_overlap(self, what, inputs, outputs):
        """No output of `outputs` shares memory with a row of `inputs` or with an output before it (rows as _outs takes them)."""
        spans = [(name, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t, _, _, name in inputs + outputs if t is not None]
        first_output = sum(t is not None for t, _, _, _ in inputs)
        for o in range(first_output, len(spans)):
            name, lo, hi = spans[o]
            for other, lo2, hi2 in spans[:o]:
                if lo < hi2 and lo2 < hi:
                    raise ValueError(f"{what}: {name} overlaps {other} (an output shares no memory with an input or another output)")

    def gae_into(self, obs, rewards, done, value_w, adv, values, *, obs0, policies: int = 1, term_obs=None, length=None,
                 gamma: float = 0.99, lam: float = 0.95, ret=None):
        """Allocation-free GAE(lambda) on tensors in the kernel's layouts (include/os2r_critic.h: os2rv_gae; the arithmetic and
        its order are spelled out there).  With P = policies, S samples, N = S P lanes (lane s P + p: sample s of policy p) and K
        steps: obs [K, N, D], obs0 [N, D] (required: what step 0 saw), term_obs [K, N, D] or None, rewards [K, N], done [K, N]
        uint8, length [N] int32 (None: K) and value_w [D+1, P] are read; adv [K, N] and values [K, N] (both required: the second
        launch reads values) and ret [K, N] (or None) are written.  gamma and lam in [0, 1].  Shapes, dtypes, device, contiguity
        and overlap are checked before the library is called (it takes addresses)."""
        what = "gae"
        K, N, S, P = self._pg_lanes(what, obs, policies)
        unit = lambda x: 0.0 <= x <= 1.0
        g = _finite(what, "gamma", math.nan if isinstance(gamma, bool) else gamma, unit, "in [0, 1]", repr(gamma))
        lm = _finite(what, "lam", math.nan if isinstance(lam, bool) else lam, unit, "in [0, 1]", repr(lam))
        if any(t is None for t in (obs0, rewards, done, value_w, adv, values)):
            raise ValueError(f"{what}: obs, obs0, rewards, done, value_w, adv and values are required")
        D = self.D
        inputs = ((obs, (K, N, D), None, "obs"), (obs0, (N, D), None, "obs0"), (term_obs, (K, N, D), None, "term_obs"),
                  (rewards, (K, N), None, "rewards"), (done, (K, N), torch.uint8, "done"), (length, (N,), torch.int32, "length"),
                  (value_w, (D + 1, P), None, "value_w"))
        outputs = ((adv, (K, N), None, "adv"), (ret, (K, N), None, "ret"), (values, (K, N), None, "values"))
        self._outs(what, inputs + outputs)
        self._no_overlap(what, inputs, outputs)
        _call(critic, "os2rv_gae", "os2rv_last_error", C.byref(self._layout()), K, P, S, _ptr(obs), _ptr(obs0), _ptr(term_obs), _ptr(rewards),
              _ptr(done), _ptr(length), _ptr(value_w), g, lm, _ptr(adv), _ptr(ret), _ptr(values), self._stream())

    def gae(self, obs, rewards, done, value_w, *, obs0, policies: int = 1, term_obs=None, length=None, gamma: float = 0.99,
            lam: float = 0.95, want_returns: bool = True, want_values: bool = False):
        """The generalised advantage estimate of every step of every lane under a linear value function per policy, in one call
        (include/os2r_critic.h: os2rv_gae): obs [K, N, D], rewards [K, N], done [K, N] uint8 and term_obs [K, N, D] are what
        rollout_policy(want_outputs=True) returned, all taken without a copy; obs0 [N, D] what reset() or the previous window's
        last step returned; value_w [P, D+1] the weights of V_p(x) = w_p . [x; 1] as value_fit returns them (a permuted view of
        the kernel's [D+1, P] goes on without a copy).  A done step (bit 0) or a guarded one (bit 2) ends its episode with value
        0 behind it, a TimeLimit truncation (bit 1 alone) with the value of term_obs (0 without term_obs); the window counts
        whole, across auto-resets, or up to length [N] int32 where given.
        -> (adv [K, N]; ret [K, N] | None: adv + values, the target of value_fit; values [K, N] | None), 0 where k >= length.
        policy_gradient(rewards=adv, done=done, gamma=0.0) weights every step with its advantage."""
        what = "gae"
        K, N, S, P = self._pg_lanes(what, obs, policies)                    # (here too: they size what is allocated)
        w = self._kernel_view(what, value_w, (P, self.D + 1), "value_w", (1, 0))
        adv, values = self._new(K, N), self._new(K, N)
        ret = self._new(K, N) if want_returns else None
        self.gae_into(obs, rewards, done, w, adv, values, obs0=obs0, policies=P, term_obs=term_obs, length=length, gamma=gamma, lam=lam,
                      ret=ret)
        return adv, ret, values if want_values else None

    def value_fit_into(self, obs, target, w, lane_mom, mom, lane_count, *, obs0, policies: int = 1, length=None, prev=None,
                       ridge: float = 0.0, failed=None, steps=None, valid=None):
        """Allocation-free ridge least-squares fit of the value weights on tensors in the kernel's layouts (include/os2r_critic.h:
        os2rv_value_fit; the arithmetic and its order are spelled out there).  With P = policies, N = S P lanes, K steps and
        E = gym_os2r_amd.critic.moments(D): obs [K, N, D], obs0 [N, D] (required), target [K, N], length [N] int32 (None: K) and
        prev [D+1, P] (None: the ridge pulls towards 0) are read; w [D+1, P], lane_mom [E, N], mom [E, P] and lane_count [2, N]
        int32 (all four required: each launch reads what the one before it wrote) and failed, steps, valid [P] int32 (each or
        None) are written.  ridge >= 0.  Shapes, dtypes, device, contiguity and overlap are checked before the library is called
        (it takes addresses)."""
        what = "value_fit"
        K, N, S, P = self._pg_lanes(what, obs, policies)
        r = _finite(what, "ridge", math.nan if isinstance(ridge, bool) else ridge, _not_negative, ">= 0", repr(ridge))
        if any(t is None for t in (obs0, target, w, lane_mom, mom, lane_count)):
            raise ValueError(f"{what}: obs, obs0, target, w, lane_mom, mom and lane_count are required")
        D, i32 = self.D, torch.int32
        E = critic.moments(D)
        inputs = ((obs, (K, N, D), None, "obs"), (obs0, (N, D), None, "obs0"), (target, (K, N), None, "target"),
                  (length, (N,), i32, "length"), (prev, (D + 1, P), None, "prev"))
        outputs = ((w, (D + 1, P), None, "w"), (lane_mom, (E, N), None, "lane_mom"), (mom, (E, P), None, "mom"),
                   (lane_count, (critic.LANE_COUNTS, N), i32, "lane_count"), (failed, (P,), i32, "failed"), (steps, (P,), i32, "steps"),
                   (valid, (P,), i32, "valid"))
        self._outs(what, inputs + outputs)
        self._no_overlap(what, inputs, outputs)
        _call(critic, "os2rv_value_fit", "os2rv_last_error", C.byref(self._layout()), K, P, S, _ptr(obs), _ptr(obs0), _ptr(target),
              _ptr(length), _ptr(prev), r, _ptr(w), _ptr(lane_mom), _ptr(mom), _ptr(lane_count), _ptr(failed), _ptr(steps), _ptr(valid),
              self._stream())

    def value_fit(self, obs, target, *, obs0, policies: int = 1, length=None, prev=None, ridge: float = 0.0):
        """The ridge least-squares refit of P = policies linear value functions on the batch in one call (include/os2r_critic.h:
        os2rv_value_fit): w_p minimises sum (w . [x_k; 1] - target[k][l])^2 + ridge |w - prev_p|^2 over the counted steps of the
        policy's valid lanes, by the normal equations and a Cholesky factor.  obs [K, N, D] and obs0 [N, D] as in gae(), target
        [K, N] the ret of gae() or the rtg of policy_gradient(), prev [P, D+1] the weights an earlier call returned (None: 0).
        A lane one of whose moment sums is not finite is left out.
        -> (w [P, D+1]: a permuted view of the kernel's layout, what gae() and the next value_fit(prev=...) take without a copy
        -- where the factor failed, prev (or 0); failed [P] int32: 0, or j + 1 where the factor failed at column j; steps [P]
        int32: the counted steps; valid [P] int32: the valid lanes)."""
        what = "value_fit"
        K, N, S, P = self._pg_lanes(what, obs, policies)                    # (here too: they size what is allocated)
        D, i32 = self.D, torch.int32
        pv = self._kernel_view(what, prev, (P, D + 1), "prev", (1, 0))
        E = critic.moments(D)
        w, lane_mom, mom, count = self._new(D + 1, P), self._new(E, N), self._new(E, P), self._new(critic.LANE_COUNTS, N, dtype=i32)
        failed, steps, valid = (self._new(P, dtype=i32) for _ in range(3))
        self.value_fit_into(obs, target, w, lane_mom, mom, count, obs0=obs0, policies=P, length=length, prev=pv, ridge=ridge, failed=failed,
                            steps=steps, valid=valid)
        return w.t(), failed, steps, valid

    # -- the clipped-surrogate (PPO) gradient -----------------------------------------------
    def ppo_gradient_into(self, obs, noise, sigma, weights, weights_old, adv, grad, lane_grad, lane_stat, lane_count, *, policies: int = 1,
                          clip: float = 0.2, obs0=None, actions=None, tanh: bool = False, length=None, sigma_new=None, lsig_grad=None,
                          lane_lsig=None, stat=None, steps=None, clipped=None, gated=None, valid=None, ratio=None):
        """Allocation-free clipped-surrogate gradient on tensors in the kernel's layouts (include/os2r_ppo.h: os2ro_ppo_gradient;
        the arithmetic and its order are spelled out there).  With P = policies, S samples, N = S P lanes (lane s P + p: sample s
        of policy p) and K steps: obs [K, N, D], obs0 [N, D] (None: obs[k] is what step k's action saw), noise [K, N, 2], actions
        [K, N, 2] (required unless tanh), sigma [2] or [2, N] (the width the batch was sampled with), sigma_new [2, P] (None: the
        same width), weights and weights_old [2, D+1, P] (evaluated, and sampled with), length [N] int32 (None: K) and adv [K, N]
        are read, clip in (0, 1); grad [2, D+1, P], lane_grad [2, D+1, N], lane_stat [3, N] and lane_count [5, N] int32 (all four
        required), lsig_grad [2, P] with lane_lsig [2, N], stat [3, P], steps [P] int32, clipped [2, P] int32, gated [P] int32,
        valid [P] int32 and ratio [K, N] are written, each of the last eight or None.  Shapes, dtypes, device, contiguity,
        alignment and overlap are checked before the library is called (it takes addresses)."""
        what = "ppo_gradient"
        K, N, S, P = self._pg_lanes(what, obs, policies)
        c = _finite(what, "clip", math.nan if isinstance(clip, bool) else clip, lambda x: 0.0 < x < 1.0, "in (0, 1)", repr(clip))
        D, i32 = self.D, torch.int32
        if any(t is None for t in (noise, sigma, weights, weights_old, adv, grad, lane_grad, lane_stat, lane_count)):
            raise ValueError(f"{what}: obs, noise, sigma, weights, weights_old, adv, grad, lane_grad, lane_stat and lane_count are required")
        if not tanh and actions is None:
            raise ValueError(f"{what}: actions are required unless tanh (where the clip bound, a step's component is left out)")
        if (lsig_grad is None) != (lane_lsig is None):
            raise ValueError(f"{what}: lsig_grad and lane_lsig go together (the second launch reads the one to write the other)")
        if tanh:
            actions = None
        per_lane = isinstance(sigma, torch.Tensor) and sigma.dim() == 2
        inputs = ((obs, (K, N, D), None, "obs"), (obs0, (N, D), None, "obs0"), (noise, (K, N, 2), None, "noise"),
                  (actions, (K, N, 2), None, "actions"), (sigma, (2, N) if per_lane else (2,), None, "sigma"),
                  (sigma_new, (2, P), None, "sigma_new"), (weights, (2, D + 1, P), None, "weights"),
                  (weights_old, (2, D + 1, P), None, "weights_old"), (length, (N,), i32, "length"), (adv, (K, N), None, "adv"))
        outputs = ((grad, (2, D + 1, P), None, "grad"), (lane_grad, (2, D + 1, N), None, "lane_grad"), (lsig_grad, (2, P), None, "lsig_grad"),
                   (lane_lsig, (2, N), None, "lane_lsig"), (stat, (ppo.STATS, P), None, "stat"), (lane_stat, (ppo.STATS, N), None, "lane_stat"),
                   (steps, (P,), i32, "steps"), (clipped, (2, P), i32, "clipped"), (gated, (P,), i32, "gated"), (valid, (P,), i32, "valid"),
                   (ratio, (K, N), None, "ratio"), (lane_count, (ppo.LANE_COUNTS, N), i32, "lane_count"))
        self._outs(what, inputs + outputs)
        for t, name in ((noise, "noise"), (actions, "actions")):
            if t is not None and t.data_ptr() % (2 * t.element_size()):
                raise ValueError(f"{what}: {name} must be aligned to a pair of its elements")
        self._no_overlap(what, inputs, outputs)
        _call(ppo, "os2ro_ppo_gradient", "os2ro_last_error", C.byref(self._layout()), K, P, S,
              (ppo.TANH if tanh else 0) | (ppo.SIGMA_PER_LANE if per_lane else 0), _ptr(obs), _ptr(obs0), _ptr(noise), _ptr(actions), _ptr(sigma),
              _ptr(sigma_new), _ptr(weights), _ptr(weights_old), _ptr(length), _ptr(adv), c, _ptr(grad), _ptr(lane_grad), _ptr(lsig_grad),
              _ptr(lane_lsig), _ptr(stat), _ptr(lane_stat), _ptr(steps), _ptr(clipped), _ptr(gated), _ptr(valid), _ptr(ratio), _ptr(lane_count),
              self._stream())

    def ppo_gradient(self, obs, noise, sigma, weights, weights_old, adv, *, policies: int = 1, clip: float = 0.2, obs0=None, actions=None,
                     tanh: bool = False, length=None, sigma_new=None, want_log_sigma: bool = False, want_lane: bool = False,
                     want_ratio: bool = False):
        """The gradient of PPO's clipped surrogate sum min(rho psi, clamp(rho, 1 - clip, 1 + clip) psi) of P = policies
        linear-Gaussian policies in one call (include/os2r_ppo.h: os2ro_ppo_gradient), evaluated at `weights` on a batch that was
        sampled with `weights_old`: obs, noise, actions, length, obs0, sigma (a float, [2] or [N, 2]) and tanh are those of
        policy_gradient, all taken without a copy; adv [K, N] is the weight psi of every step as gae() returned it (normalised
        or not).  weights and weights_old are [P, 2, D+1] -- a permuted view of the kernel's [2, D+1, P], as this call's grad
        is, goes on without a copy --, sigma_new [P, 2] the width of the policy being evaluated (None: the width of the batch).
        rho is the likelihood ratio of the pre-squash sample over the components on which the action clip did not bind; a
        step adds its gradient unless (psi > 0 and rho > 1 + clip) or (psi < 0 and rho < 1 - clip).  With weights equal to
        weights_old and sigma_new None every rho is 1 and the call returns the bits of policy_gradient(rewards=adv, gamma=0.0).
        A lane one of whose sums is not finite is left out of its policy's sums.
        -> (grad [P, 2, D+1]: a permuted view of the kernel's layout; stats [P, 3]: the sums of the surrogate itself, of rho - 1
        (dev) and of log rho before the widths' factor (logr) -- where the widths are unchanged (dev - logr) / steps is the k3
        estimate of the KL divergence KL(old || new), mean((rho - 1) - log rho) over the counted steps, and -logr / steps the
        k1 estimate; steps [P] int32: the counted steps; clipped [P, 2] int32: how often the action clip bound; gated [P] int32:
        the steps whose gradient the ratio's clip took out; valid [P] int32: the valid lanes; lsig_grad [P, 2] | None: the
        gradient with respect to the log of the evaluated width; lane_grad [N, 2, D+1] | None: the per-lane sums; ratio [K, N] |
        None: rho of every counted step, 0 behind length)."""
        what = "ppo_gradient"
        K, N, S, P = self._pg_lanes(what, obs, policies)                    # (here too: they size what is allocated)
        if isinstance(sigma, bool) or sigma is None:
            raise ValueError(f"{what}: sigma must be a float, a [2] tensor or an [{N}, 2] tensor, got {sigma!r}")
        if isinstance(sigma, (int, float)):
            sigma = torch.full((2,), float(sigma), dtype=self.dtype, device=self.device)
        elif isinstance(sigma, torch.Tensor) and sigma.dim() == 2:
            sigma = self._kernel_view(what, sigma, (N, 2), "sigma", (1, 0))  # the [2, N] an [N, 2] sigma is a view of goes on as it is
        D, i32 = self.D, torch.int32
        if weights is None or weights_old is None:
            raise ValueError(f"{what}: weights and weights_old are required, each [{P}, 2, {D + 1}]")
        w = self._kernel_view(what, weights, (P, 2, D + 1), "weights", (1, 2, 0))
        w_old = self._kernel_view(what, weights_old, (P, 2, D + 1), "weights_old", (1, 2, 0))
        s_new = self._kernel_view(what, sigma_new, (P, 2), "sigma_new", (1, 0))
        grad, lane, count = self._new(2, D + 1, P), self._new(2, D + 1, N), self._new(ppo.LANE_COUNTS, N, dtype=i32)
        stat, lane_stat = self._new(ppo.STATS, P), self._new(ppo.STATS, N)
        steps, clipped, gated, valid = self._new(P, dtype=i32), self._new(2, P, dtype=i32), self._new(P, dtype=i32), self._new(P, dtype=i32)
        lsig = self._new(2, P) if want_log_sigma else None
        lane_lsig = self._new(2, N) if want_log_sigma else None
        ratio = self._new(K, N) if want_ratio else None
        self.ppo_gradient_into(obs, noise, sigma, w, w_old, adv, grad, lane, lane_stat, count, policies=P, clip=clip, obs0=obs0,
                               actions=actions, tanh=tanh, length=length, sigma_new=s_new, lsig_grad=lsig, lane_lsig=lane_lsig, stat=stat,
                               steps=steps, clipped=clipped, gated=gated, valid=valid, ratio=ratio)
        return (grad.permute(2, 0, 1), stat.t(), steps, clipped.t(), gated, valid, None if lsig is None else lsig.t(),
                lane.permute(2, 0, 1) if want_lane else None, ratio)

    # -- the natural-gradient step ------------------------------------------------------------
    def natural_step_into(self, obs, sigma, grad, step, lane_mom, mom, lane_count, *, policies: int = 1, obs0=None, actions=None,
                          tanh: bool = False, length=None, lsig_grad=None, damping: float = 1e-3, kl: float = 0.01, dir=None,
                          lsig_step=None, beta=None, quad=None, failed=None, steps=None, open=None, valid=None):
        """Allocation-free natural-gradient step on tensors in the kernel's layouts (include/os2r_npg.h: os2rn_natural_step; the
        arithmetic and its order are spelled out there).  With P = policies, S samples, N = S P lanes (lane s P + p: sample s of
        policy p), K steps and E = gym_os2r_amd.npg.moments(D): obs [K, N, D], obs0 [N, D] (None: obs[k] is what step k's action
        saw), actions [K, N, 2] (required unless tanh), sigma [2] or [2, N], length [N] int32 (None: K), grad [2, D+1, P] and
        lsig_grad [2, P] (or None) are read, damping >= 0 and kl >= 0; step [2, D+1, P], lane_mom [E, N], mom [E, P] and lane_count
        [4, N] int32 (all four required: each launch reads what the one before it wrote), lsig_step [2, P] (exactly with
        lsig_grad), dir [2, D+1, P], beta [P], quad [P], failed [3, P] int32, steps [P] int32, open [2, P] int32 and valid [P] int32
        are written, each of the last seven or None (without steps or open the solve adds those integers up itself, a lane
        after the other: give both where S is large).  Shapes, dtypes, device, contiguity, alignment and overlap are checked
        before the library is called (it takes addresses)."""
        what = "natural_step"
        K, N, S, P = self._pg_lanes(what, obs, policies)
        damp = _finite(what, "damping", math.nan if isinstance(damping, bool) else damping, _not_negative, ">= 0", repr(damping))
        bound = _finite(what, "kl", math.nan if isinstance(kl, bool) else kl, _not_negative, ">= 0", repr(kl))
        D, i32 = self.D, torch.int32
        if any(t is None for t in (sigma, grad, step, lane_mom, mom, lane_count)):
            raise ValueError(f"{what}: obs, sigma, grad, step, lane_mom, mom and lane_count are required")
        if not tanh and actions is None:
            raise ValueError(f"{what}: actions are required unless tanh (where the clip bound, a step's component adds no curvature)")
        if (lsig_grad is None) != (lsig_step is None):
            raise ValueError(f"{what}: lsig_grad and lsig_step go together (the step of the widths is that of their gradient)")
        if tanh:
            actions = None
        per_lane = isinstance(sigma, torch.Tensor) and sigma.dim() == 2
        E = npg.moments(D)
        inputs = ((obs, (K, N, D), None, "obs"), (obs0, (N, D), None, "obs0"), (actions, (K, N, 2), None, "actions"),
                  (sigma, (2, N) if per_lane else (2,), None, "sigma"), (length, (N,), i32, "length"), (grad, (2, D + 1, P), None, "grad"),
                  (lsig_grad, (2, P), None, "lsig_grad"))
        outputs = ((step, (2, D + 1, P), None, "step"), (dir, (2, D + 1, P), None, "dir"), (lsig_step, (2, P), None, "lsig_step"),
                   (beta, (P,), None, "beta"), (quad, (P,), None, "quad"), (failed, (3, P), i32, "failed"), (steps, (P,), i32, "steps"),
                   (open, (2, P), i32, "open"), (valid, (P,), i32, "valid"), (lane_mom, (E, N), None, "lane_mom"), (mom, (E, P), None, "mom"),
                   (lane_count, (npg.LANE_COUNTS, N), i32, "lane_count"))
        self._outs(what, inputs + outputs)
        if actions is not None and actions.data_ptr() % (2 * actions.element_size()):
            raise ValueError(f"{what}: actions must be aligned to a pair of its elements")
        self._no_overlap(what, inputs, outputs)
        _call(npg, "os2rn_natural_step", "os2rn_last_error", C.byref(self._layout()), K, P, S,
              (npg.TANH if tanh else 0) | (npg.SIGMA_PER_LANE if per_lane else 0), _ptr(obs), _ptr(obs0), _ptr(actions), _ptr(sigma),
              _ptr(length), _ptr(grad), _ptr(lsig_grad), damp, bound, _ptr(step), _ptr(dir), _ptr(lsig_step), _ptr(beta), _ptr(quad),
              _ptr(failed), _ptr(steps), _ptr(open), _ptr(valid), _ptr(lane_mom), _ptr(mom), _ptr(lane_count), self._stream())

    def natural_step(self, obs, sigma, grad, *, policies: int = 1, obs0=None, actions=None, tanh: bool = False, length=None, lsig_grad=None,
                     damping: float = 1e-3, kl: float = 0.01, want_dir: bool = False, want_counts: bool = True):
        """The natural-gradient step of P = policies linear-Gaussian policies in one call (include/os2r_npg.h:
        os2rn_natural_step): obs, actions, length, obs0, sigma (a float, [2] or [N, 2]) and tanh are those of policy_gradient,
        all taken without a copy; grad [P, 2, D+1] is what policy_gradient or ppo_gradient returned (a permuted view of the
        kernel's [2, D+1, P] goes on without a copy), lsig_grad [P, 2] their gradient of log sigma (None: the widths stay).
        Per action component j the Fisher matrix of the mean weights is the mean over the counted steps of the policy's valid
        lanes of [x; 1][x; 1]' / sigma_j^2 on the steps where the component was open (sigma_j > 0 and, unless tanh, the clip did
        not bind); d_j solves (F_j + damping I) d_j = grad_j / steps by a Cholesky factor, the widths have the Fisher entry
        2 open_j / steps.  With the widths unchanged the mean KL divergence of a step Delta is exactly 1/2 Delta' F Delta, so
        step = sqrt(2 kl / (g . d)) d has the divergence kl (up to the damping): a step size in nats, the same for every policy.
        kl = 0: step = d, the plain natural gradient.  A lane one of whose moment sums is not finite is left out.
        -> (step [P, 2, D+1]: a permuted view of the kernel's layout, weights + step is what rollout_policy takes next;
        lsig_step [P, 2] | None: the step of log sigma; beta [P]: the factor on d; quad [P]: g . d; failed [P, 3] int32: per
        component 0 or the column + 1 at which its factor failed (d_j = 0), and 1 where g . d was not finite and positive
        (step = 0); steps [P] int32 | None: the counted steps; open [P, 2] int32 | None: the open steps of each component; valid
        [P] int32 | None: the valid lanes -- the three None without want_counts; dir [P, 2, D+1] | None: d itself)."""
        what = "natural_step"
        K, N, S, P = self._pg_lanes(what, obs, policies)                    # (here too: they size what is allocated)
        if isinstance(sigma, bool) or sigma is None:
            raise ValueError(f"{what}: sigma must be a float, a [2] tensor or an [{N}, 2] tensor, got {sigma!r}")
        if isinstance(sigma, (int, float)):
            sigma = torch.full((2,), float(sigma), dtype=self.dtype, device=self.device)
        elif isinstance(sigma, torch.Tensor) and sigma.dim() == 2:
            sigma = self._kernel_view(what, sigma, (N, 2), "sigma", (1, 0))  # the [2, N] an [N, 2] sigma is a view of goes on as it is
        D, i32 = self.D, torch.int32
        if grad is None:
            raise ValueError(f"{what}: grad is required, [{P}, 2, {D + 1}]")
        g = self._kernel_view(what, grad, (P, 2, D + 1), "grad", (1, 2, 0))
        g_ls = self._kernel_view(what, lsig_grad, (P, 2), "lsig_grad", (1, 0))
        E = npg.moments(D)
        step, lane_mom, mom, count = self._new(2, D + 1, P), self._new(E, N), self._new(E, P), self._new(npg.LANE_COUNTS, N, dtype=i32)
        beta, quad, failed = self._new(P), self._new(P), self._new(3, P, dtype=i32)
        # the integer totals are always asked of the sum launch: the solve reads them
        steps, opened, valid = self._new(P, dtype=i32), self._new(2, P, dtype=i32), self._new(P, dtype=i32)
        direction = self._new(2, D + 1, P) if want_dir else None
        ls_step = self._new(2, P) if g_ls is not None else None
        self.natural_step_into(obs, sigma, g, step, lane_mom, mom, count, policies=P, obs0=obs0, actions=actions, tanh=tanh, length=length,
                               lsig_grad=g_ls, damping=damping, kl=kl, dir=direction, lsig_step=ls_step, beta=beta, quad=quad, failed=failed,
                               steps=steps, open=opened, valid=valid)
        return (step.permute(2, 0, 1), None if ls_step is None else ls_step.t(), beta, quad, failed.t(),
                steps if want_counts else None, opened.t() if want_counts else None, valid if want_counts else None,
                None if direction is None else direction.permute(2, 0, 1))

    # -- evolution strategies: antithetic perturbations and the ARS V1-t update -------------
    def _es_shape(self, what, theta, directions, generation, seed, pop_offset):
        """theta [M, 2, D+1] and the integers both calls share -> (M, S, N = 2 S M, seed, pop_offset, generation)."""
        S = _count(what, "directions", directions)
        if S > es.MAX_DIRECTIONS:
            raise ValueError(f"{what}: directions must be below 2^27, got {S}")
        if not isinstance(theta, torch.Tensor) or theta.dim() != 3 or theta.shape[0] < 1:
            raise ValueError(f"{what}: theta must be a tensor [M, 2, {self.D + 1}] with M >= 1, got {tuple(getattr(theta, 'shape', ()))}")
        M = int(theta.shape[0])
        if 2 * S * M > 2 ** 31 - 1:
            raise ValueError(f"{what}: 2 x directions x populations = {2 * S * M} exceeds 2^31 - 1")
        words = []
        for name, v in (("generation", generation), ("pop_offset", pop_offset)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 32:
                raise ValueError(f"{what}: {name} must be an integer in 0..2^32 - 1, got {v!r}")
            words.append(v)
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64):
            raise ValueError(f"{what}: seed must be None (the handle's) or an integer in 0..2^64 - 1, got {seed!r}")
        return M, S, 2 * S * M, seed, words[1], words[0]

    def _es_aligned(self, what, rows):
        for t, name in rows:
            if t is not None and t.data_ptr() % (2 * t.element_size()):
                raise ValueError(f"{what}: {name} must be aligned to a pair of its elements")

    def es_perturb_into(self, theta, weights, *, directions: int, nu: float, generation: int, seed=None, pop_offset: int = 0, delta=None):
        """Allocation-free antithetic perturbation of M policies along S = directions directions each, in one launch
        (include/os2r_es.h: os2ra_es_perturb; the arithmetic is spelled out there).  theta [M, 2, D+1] is read; weights [N, 2, D+1]
        with N = 2 S M lanes and delta [S M, 2, D+1] (or None) are written: lane (h S + s) M + m is theta_m + nu delta[m, s] for
        h = 0 and theta_m - nu delta[m, s] for h = 1, what rollout_policy takes as per-environment weights; row s M + m of delta
        is delta[m, s].  The directions are a pure function of (seed, pop_offset + m, s, generation) under the stepper's counter
        RNG (stream 6), drawn in double and rounded once to the handle's dtype; seed None is the handle's seed, generation and
        pop_offset are 32-bit words.  nu >= 0.  Shapes, dtypes, device, contiguity, alignment and overlap are checked before the
        library is called (it takes addresses)."""
        what = "es_perturb"
        M, S, N, seed, off, gen = self._es_shape(what, theta, directions, generation, seed, pop_offset)
        scale = _finite(what, "nu", math.nan if isinstance(nu, bool) else nu, _not_negative, ">= 0", repr(nu))
        if weights is None:
            raise ValueError(f"{what}: theta and weights are required")
        D = self.D
        inputs = ((theta, (M, 2, D + 1), None, "theta"),)
        outputs = ((weights, (N, 2, D + 1), None, "weights"), (delta, (S * M, 2, D + 1), None, "delta"))
        self._outs(what, inputs + outputs)
        self._es_aligned(what, ((theta, "theta"), (weights, "weights"), (delta, "delta")))
        self._no_overlap(what, inputs, outputs)
        _call(es, "os2ra_es_perturb", "os2ra_last_error", C.byref(self._layout()), M, S, 0, int(self.cfg.seed) if seed is None else seed, off,
              gen, _ptr(theta), scale, _ptr(weights), _ptr(delta), self._stream())

    def es_perturb(self, theta, directions: int, nu: float, generation: int, seed=None, pop_offset: int = 0, want_delta: bool = False):
        """The 2 S M perturbed policies of one generation of evolution-strategy search, in one launch (include/os2r_es.h:
        os2ra_es_perturb): theta [M, 2, D+1] holds M policies (populations) as rollout_policy takes one, S = directions.
        -> (weights [N, 2, D+1], N = 2 S M: lane (h S + s) M + m is theta_m + nu delta[m, s] (h = 0) or theta_m - nu delta[m, s]
        (h = 1) -- rollout_policy(K, weights, first_episode=True) on a handle of N environments returns what es_update takes,
        and copy_envs_from(real, arange(N) % M) lines the environments up without a gather; delta [S M, 2, D+1] | None: the
        directions, row s M + m, for tests and for callers who want them -- es_update does not read them, it regenerates them
        from (seed, pop_offset + m, s, generation)).  Populations that differ in pop_offset only draw different directions; a
        shard of populations with pop_offset = a draws what populations a, a + 1, ... of one call would."""
        what = "es_perturb"
        M, S, N, _, _, _ = self._es_shape(what, theta, directions, generation, seed, pop_offset)   # (here too: they size what is allocated)
        weights = self._new(N, 2, self.D + 1)
        delta = self._new(S * M, 2, self.D + 1) if want_delta else None
        self.es_perturb_into(theta, weights, directions=S, nu=nu, generation=generation, seed=seed, pop_offset=pop_offset, delta=delta)
        return weights, delta

    def es_update_into(self, returns, theta, theta_new, sigma_r, count, used, kept, *, directions: int, generation: int, step_size: float,
                       top: int = 0, sigma_floor: float = 1e-8, seed=None, pop_offset: int = 0, grad=None, score=None):
        """Allocation-free ARS V1-t update of M policies from the returns of their 2 S lanes (include/os2r_es.h: os2ra_es_update;
        the arithmetic and its order are spelled out there).  returns [N] (N = 2 S M, the lanes of es_perturb) and theta
        [M, 2, D+1] are read; theta_new [M, 2, D+1], sigma_r [M], count [M] int32, used [M] int32 and kept [S M] int32 (all
        required: kept is the scratch the sums read where top selects) and grad [M, 2, D+1] (or None) are written; score [S M]
        in the handle's dtype is scratch, required where 0 < top < directions and not touched otherwise.  step_size and
        sigma_floor >= 0, top >= 0.  generation, seed and pop_offset are those of the es_perturb call whose weights were rolled
        out.  An output may not overlap an input: the caller swaps theta and theta_new.  Shapes, dtypes, device, contiguity,
        alignment and overlap are checked before the library is called (it takes addresses)."""
        what = "es_update"
        M, S, N, seed, off, gen = self._es_shape(what, theta, directions, generation, seed, pop_offset)
        if isinstance(top, bool) or not isinstance(top, int) or top < 0:
            raise ValueError(f"{what}: top must be an integer >= 0 (0: every direction), got {top!r}")
        step = _finite(what, "step_size", math.nan if isinstance(step_size, bool) else step_size, _not_negative, ">= 0", repr(step_size))
        floor = _finite(what, "sigma_floor", math.nan if isinstance(sigma_floor, bool) else sigma_floor, _not_negative, ">= 0",
                        repr(sigma_floor))
        if any(t is None for t in (returns, theta_new, sigma_r, count, used, kept)):
            raise ValueError(f"{what}: returns, theta, theta_new, sigma_r, count, used and kept are required")
        select = 0 < top < S
        if select and score is None:
            raise ValueError(f"{what}: score [{S * M}] is required where 0 < top < directions (the rank launch reads it)")
        D, i32 = self.D, torch.int32
        inputs = ((returns, (N,), None, "returns"), (theta, (M, 2, D + 1), None, "theta"))
        outputs = ((theta_new, (M, 2, D + 1), None, "theta_new"), (sigma_r, (M,), None, "sigma_r"), (count, (M,), i32, "count"),
                   (used, (M,), i32, "used"), (grad, (M, 2, D + 1), None, "grad"), (kept, (S * M,), i32, "kept"),
                   (score if select else None, (S * M,), None, "score"))
        self._outs(what, inputs + outputs)
        self._es_aligned(what, ((theta, "theta"), (theta_new, "theta_new"), (grad, "grad")))
        self._no_overlap(what, inputs, outputs)
        _call(es, "os2ra_es_update", "os2ra_last_error", C.byref(self._layout()), M, S, min(top, 2 ** 31 - 1), 0,
              int(self.cfg.seed) if seed is None else seed, off, gen, _ptr(returns), _ptr(theta), step, floor, _ptr(theta_new), _ptr(sigma_r),
              _ptr(count), _ptr(used), _ptr(grad), _ptr(kept), _ptr(score) if select else None, self._stream())

    def es_update(self, returns, theta, directions: int, generation: int, step_size: float, top: int = 0, sigma_floor: float = 1e-8,
                  seed=None, pop_offset: int = 0, want_grad: bool = False, want_kept: bool = False):
        """The update of augmented random search (ARS V1-t, Mania et al. 2018) of M policies in one call (include/os2r_es.h:
        os2ra_es_update): returns [N] is what rollout_policy(K, weights, first_episode=True) returned for the weights of
        es_perturb(theta, directions, nu, generation, ...), as it lies on the device; generation, seed and pop_offset are that
        call's.  Per population: a direction is valid where both of its returns are finite; the b' = min(top or S, valid) valid
        directions of the largest max(r+, r-) are kept (equal scores: the lower s first); sigma_R is the standard deviation
        (ddof 0) of the 2 b' kept returns, at least sigma_floor; theta_new = theta + step_size / (b' sigma_R) sum (r+ - r-) delta
        over the kept directions, the directions regenerated from the counter RNG, not read.  A population without a valid
        direction keeps theta and reports sigma_R = 0.
        -> (theta_new [M, 2, D+1]; sigma_r [M]; count [M] int32: the valid directions; used [M] int32: b'; grad [M, 2, D+1] |
        None: the step without step_size, for the caller's own optimiser; kept [S M] int32 | None: 1 where direction s of
        population m, at s M + m, was kept)."""
        what = "es_update"
        M, S, N, _, _, _ = self._es_shape(what, theta, directions, generation, seed, pop_offset)   # (here too: they size what is allocated)
        D, i32 = self.D, torch.int32
        theta_new, sigma_r = self._new(M, 2, D + 1), self._new(M)
        count, used, kept = self._new(M, dtype=i32), self._new(M, dtype=i32), self._new(S * M, dtype=i32)
        grad = self._new(M, 2, D + 1) if want_grad else None
        select = isinstance(top, int) and 0 < top < S
        score = self._new(S * M) if select else None
        self.es_update_into(returns, theta, theta_new, sigma_r, count, used, kept, directions=S, generation=generation, step_size=step_size,
                            top=top, sigma_floor=sigma_floor, seed=seed, pop_offset=pop_offset, grad=grad, score=score)
        return theta_new, sigma_r, count, used, grad, kept if want_kept else None

    # -- CMA-ES: factors and correlated samples, and the update of mean, step size, covariance and paths ------
    def _cma_state(self, what, state, name="state"):
        """state = (mean [M, 2, D+1], sigma [M], cov [M, E, E], p_sigma [M, E], p_c [M, E]) -> (its five tensors, M), the shapes
        checked against the mean's."""
        E = 2 * (self.D + 1)
        if not isinstance(state, (tuple, list)) or len(state) != 5 or not isinstance(state[0], torch.Tensor) or state[0].dim() != 3 \
                or state[0].shape[0] < 1:
            raise ValueError(f"{what}: {name} must be (mean [M, 2, {self.D + 1}], sigma [M], cov [M, {E}, {E}], p_sigma [M, {E}], "
                             f"p_c [M, {E}]) with M >= 1, got {type(state)}")
        M = int(state[0].shape[0])
        shapes = ((M, 2, self.D + 1), (M,), (M, E, E), (M, E), (M, E))
        rows = tuple((t, shape, None, f"{name}: {n}") for t, shape, n in zip(state, shapes, ("mean", "sigma", "cov", "p_sigma", "p_c")))
        if any(t is None for t in state):
            raise ValueError(f"{what}: {name}: mean, sigma, cov, p_sigma and p_c are all required")
        self._outs(what, rows)
        return rows, M

    def _cma_shape(self, what, M, samples, generation, seed, pop_offset):
        """The integers both calls share -> (S, N = S M, seed, pop_offset, generation)."""
        S = _count(what, "samples", samples)
        if S < 2 or S > cma.MAX_SAMPLES:
            raise ValueError(f"{what}: samples must be in 2..2^27 - 1, got {S}")
        if S * M > 2 ** 31 - 1:
            raise ValueError(f"{what}: samples x populations = {S * M} exceeds 2^31 - 1")
        words = []
        for name, v in (("generation", generation), ("pop_offset", pop_offset)):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 32:
                raise ValueError(f"{what}: {name} must be an integer in 0..2^32 - 1, got {v!r}")
            words.append(v)
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64):
            raise ValueError(f"{what}: seed must be None (the handle's) or an integer in 0..2^64 - 1, got {seed!r}")
        return S, S * M, seed, words[1], words[0]

    def cma_init(self, theta, sigma0):
        """The CMA-ES state of M populations that start at theta [M, 2, D+1] with the step size sigma0 (a float > 0, or a tensor
        [M]): -> (mean, sigma [M], cov [M, E, E] = I, p_sigma [M, E] = 0, p_c [M, E] = 0), new tensors in the handle's dtype."""
        what = "cma_init"
        if not isinstance(theta, torch.Tensor) or theta.dim() != 3 or theta.shape[0] < 1 or tuple(theta.shape[1:]) != (2, self.D + 1):
            raise ValueError(f"{what}: theta must be a tensor [M, 2, {self.D + 1}] with M >= 1, got {tuple(getattr(theta, 'shape', ()))}")
        M, E = int(theta.shape[0]), 2 * (self.D + 1)
        if isinstance(sigma0, torch.Tensor):
            sigma = self._in(sigma0, (M,)).clone()
        else:
            sigma = torch.full((M,), _finite(what, "sigma0", math.nan if isinstance(sigma0, bool) else sigma0, _invertible, "> 0", repr(sigma0)),
                               dtype=self.dtype, device=self.device)
        cov = torch.eye(E, dtype=self.dtype, device=self.device).repeat(M, 1, 1)
        zero = lambda: torch.zeros(M, E, dtype=self.dtype, device=self.device)
        return self._in(theta, (M, 2, self.D + 1)).clone(), sigma, cov, zero(), zero()

    def cma_sample_into(self, state, factor, failed, weights, *, samples: int, generation: int, seed=None, pop_offset: int = 0, z=None):
        """Allocation-free factors and samples of one CMA-ES generation of M populations, S = samples each (include/os2r_cma.h:
        os2rk_cma_sample; the arithmetic is spelled out there).  Of state = (mean [M, 2, D+1], sigma [M], cov [M, E, E], p_sigma,
        p_c) mean, sigma and the lower triangle of cov are read; factor [M, E, E], failed [M] int32, weights [N, 2, D+1] with
        N = S M lanes and z [N, 2, D+1] (or None) are written: lane s M + m is mean_m + sigma_m A_m z[m, s], what rollout_policy
        takes as per-environment weights, or mean_m where the factor of C_m failed (failed[m] = the column + 1) or sigma_m is
        not finite and positive (failed[m] = E + 1).  The normals are a pure function of (seed, pop_offset + m, s, generation)
        under the stepper's counter RNG (stream 7); seed None is the handle's seed.  Shapes, dtypes, device, contiguity,
        alignment and overlap are checked before the library is called (it takes addresses)."""
        what = "cma_sample"
        rows, M = self._cma_state(what, state)
        S, N, seed, off, gen = self._cma_shape(what, M, samples, generation, seed, pop_offset)
        if any(t is None for t in (factor, failed, weights)):
            raise ValueError(f"{what}: factor, failed and weights are required")
        D, E = self.D, 2 * (self.D + 1)
        inputs = rows[:3]
        outputs = ((factor, (M, E, E), None, "factor"), (failed, (M,), torch.int32, "failed"), (weights, (N, 2, D + 1), None, "weights"),
                   (z, (N, 2, D + 1), None, "z"))
        self._outs(what, outputs)
        self._es_aligned(what, ((state[0], "state: mean"), (weights, "weights"), (z, "z")))
        self._no_overlap(what, inputs, outputs)
        _call(cma, "os2rk_cma_sample", "os2rk_last_error", C.byref(self._layout()), M, S, 0, int(self.cfg.seed) if seed is None else seed, off,
              gen, _ptr(state[0]), _ptr(state[1]), _ptr(state[2]), _ptr(factor), _ptr(failed), _ptr(weights), _ptr(z), self._stream())

    def cma_sample(self, state, samples: int, generation: int, seed=None, pop_offset: int = 0, want_z: bool = False):
        """The S M sampled policies of one CMA-ES generation, in two launches (include/os2r_cma.h: os2rk_cma_sample): state is
        what cma_init or cma_update returned, S = samples.
        -> (weights [N, 2, D+1], N = S M: lane s M + m is sample s of population m -- rollout_policy(K, weights,
        first_episode=True) on a handle of N environments returns what cma_update takes, and copy_envs_from(real,
        arange(N) % M) lines the environments up without a gather; factor [M, E, E]: the lower Cholesky factor of every
        covariance, which cma_update reads; failed [M] int32: 0, or why population m was not sampled; z [N, 2, D+1] | None: the
        normals, row s M + m, for tests -- cma_update regenerates them)."""
        what = "cma_sample"
        _, M = self._cma_state(what, state)
        S, N, _, _, _ = self._cma_shape(what, M, samples, generation, seed, pop_offset)      # (here too: they size what is allocated)
        E = 2 * (self.D + 1)
        weights, factor, failed = self._new(N, 2, self.D + 1), self._new(M, E, E), self._new(M, dtype=torch.int32)
        z = self._new(N, 2, self.D + 1) if want_z else None
        self.cma_sample_into(state, factor, failed, weights, samples=S, generation=generation, seed=seed, pop_offset=pop_offset, z=z)
        return weights, factor, failed, z

    def cma_update_into(self, returns, state, factor, failed, state_new, count, status, rank, *, samples: int, generation: int, rankw,
                        constants, seed=None, pop_offset: int = 0, yw=None, ps_norm=None, growth=None):
        """Allocation-free CMA-ES update of M populations from the returns of their S lanes, larger is better
        (include/os2r_cma.h: os2rk_cma_update; the arithmetic and its order are spelled out there).  returns [N] (N = S M, the
        lanes of cma_sample), state, factor [M, E, E] and failed [M] int32 (as cma_sample wrote them) and rankw [mu] (the
        recombination weights, in the handle's dtype on its device) are read; constants is a cma.Os2rkCmaConstants
        (cma.constants() has Hansen's defaults).  state_new (five tensors as state), count [M] int32, status [M] int32 and rank
        [N] int32 (all required: rank is the scratch the sums read) and yw [M, 2, D+1], ps_norm [M], growth [M] (each or None)
        are written.  generation, seed and pop_offset are those of the cma_sample call whose weights were rolled out.  An output
        may not overlap an input or another output: the caller swaps two states.  Shapes, dtypes, device, contiguity,
        alignment and overlap are checked before the library is called (it takes addresses)."""
        what = "cma_update"
        rows, M = self._cma_state(what, state)
        S, N, seed, off, gen = self._cma_shape(what, M, samples, generation, seed, pop_offset)
        if not isinstance(rankw, torch.Tensor) or rankw.dim() != 1 or not 1 <= rankw.shape[0] <= S:
            raise ValueError(f"{what}: rankw must be a tensor [mu] with 1 <= mu <= samples = {S}, got {tuple(getattr(rankw, 'shape', ()))}")
        mu = int(rankw.shape[0])
        if not isinstance(constants, cma.Os2rkCmaConstants):
            raise ValueError(f"{what}: constants must be a cma.Os2rkCmaConstants (cma.constants() makes one), got {type(constants)}")
        for name in cma.CONSTANT_NAMES:
            if not math.isfinite(getattr(constants, name)):
                raise ValueError(f"{what}: constants.{name} must be finite, got {getattr(constants, name)}")
        if any(t is None for t in (returns, factor, failed, count, status, rank)):
            raise ValueError(f"{what}: returns, factor, failed, count, status and rank are required")
        out_rows, M_new = self._cma_state(what, state_new, "state_new")
        if M_new != M:
            raise ValueError(f"{what}: state_new holds {M_new} populations, state {M}")
        D, E, i32 = self.D, 2 * (self.D + 1), torch.int32
        inputs = ((returns, (N,), None, "returns"), (rankw, (mu,), None, "rankw")) + rows + \
                 ((factor, (M, E, E), None, "factor"), (failed, (M,), i32, "failed"))
        outputs = out_rows + ((count, (M,), i32, "count"), (status, (M,), i32, "status"), (rank, (N,), i32, "rank"),
                              (yw, (M, 2, D + 1), None, "yw"), (ps_norm, (M,), None, "ps_norm"), (growth, (M,), None, "growth"))
        self._outs(what, inputs + outputs)
        self._es_aligned(what, ((state[0], "state: mean"), (state_new[0], "state_new: mean"), (yw, "yw")))
        self._no_overlap(what, inputs, outputs)
        _call(cma, "os2rk_cma_update", "os2rk_last_error", C.byref(self._layout()), M, S, mu, 0, int(self.cfg.seed) if seed is None else seed,
              off, gen, _ptr(returns), _ptr(rankw), *[_ptr(t) for t in state], _ptr(factor), _ptr(failed), C.byref(constants),
              *[_ptr(t) for t in state_new], _ptr(count), _ptr(status), _ptr(rank), _ptr(yw), _ptr(ps_norm), _ptr(growth), self._stream())

    def cma_update(self, returns, state, factor, failed, samples: int, generation: int, parents=None, age=None, sigma_min: float = 1e-8,
                   sigma_max: float = 1.0, seed=None, pop_offset: int = 0, want_yw: bool = False, want_norm: bool = False,
                   want_growth: bool = False):
        """The update of Cholesky-CMA-ES (Hansen and Ostermeier 2001; Suttorp, Hansen and Igel 2009) of M populations in one call
        (include/os2r_cma.h: os2rk_cma_update), with Hansen's default constants (cma.constants): returns [N] is what
        rollout_policy(K, weights, first_episode=True) returned for the weights of cma_sample(state, samples, generation, ...),
        as it lies on the device; factor and failed are that call's, and so are generation, seed and pop_offset.  Per
        population: a lane is valid where its return is finite; the mu = parents (None: S // 2) valid lanes of the largest
        return are the parents (equal returns: the lower s first), weighted by rank; the mean moves by sigma times their weighted
        step, the step-size path by their weighted normals -- regenerated from the counter RNG, not read --, the covariance by
        the rank-one term of its path and the rank-mu term of the parents' steps, and sigma by the length of its path.  age is the
        number of updates the state has seen (None: generation); it enters the stall test of the path only.  A population
        whose factor failed (status 2) or that has fewer than mu valid lanes (status 1) keeps its state.
        -> (state_new: five new tensors as state; count [M] int32: the valid lanes; status [M] int32; rank [N] int32: the rank
        of every lane among those of its population; yw [M, 2, D+1] | None: the weighted step; ps_norm [M] | None: the length of
        the new step-size path; growth [M] | None: the factor on sigma before its clamp to [sigma_min, sigma_max])."""
        what = "cma_update"
        _, M = self._cma_state(what, state)
        S, N, _, _, gen = self._cma_shape(what, M, samples, generation, seed, pop_offset)      # (here too: they size what is allocated)
        if parents is not None and (isinstance(parents, bool) or not isinstance(parents, int) or not 1 <= parents <= S):
            raise ValueError(f"{what}: parents must be None (samples // 2) or an integer in 1..{S}, got {parents!r}")
        if age is not None and (isinstance(age, bool) or not isinstance(age, int) or age < 0):
            raise ValueError(f"{what}: age must be None (the generation) or an integer >= 0, got {age!r}")
        lo = _finite(what, "sigma_min", math.nan if isinstance(sigma_min, bool) else sigma_min, _not_negative, ">= 0", repr(sigma_min))
        hi = _finite(what, "sigma_max", math.nan if isinstance(sigma_max, bool) else sigma_max, lambda x: x >= lo, ">= sigma_min", repr(sigma_max))
        D, E, i32 = self.D, 2 * (self.D + 1), torch.int32
        rankw, constants = cma.constants(E, S, parents, gen if age is None else age, lo, hi)
        made = self.__dict__.setdefault("_cma_rankw", {})
        if (S, len(rankw)) not in made:                                                      # the weights on the device, once per shape
            made[(S, len(rankw))] = torch.tensor(rankw, dtype=torch.float64).to(self.dtype).to(self.device)
        state_new = (self._new(M, 2, D + 1), self._new(M), self._new(M, E, E), self._new(M, E), self._new(M, E))
        count, status, rank = self._new(M, dtype=i32), self._new(M, dtype=i32), self._new(N, dtype=i32)
        yw = self._new(M, 2, D + 1) if want_yw else None
        ps_norm = self._new(M) if want_norm else None
        growth = self._new(M) if want_growth else None
        self.cma_update_into(returns, state, factor, failed, state_new, count, status, rank, samples=S, generation=generation,
                             rankw=made[(S, len(rankw))], constants=constants, seed=seed, pop_offset=pop_offset, yw=yw, ps_norm=ps_norm,
                             growth=growth)
        return state_new, count, status, rank, yw, ps_norm, growth

    # -- running observation whitening: the statistics, the fold and the gradient back ---------
    def _norm_state(self, what, state, P=None, required=True):
        """state = (count [P] int64, mean [P, D], m2 [P, D]) of a whitening call -> (count, mean, m2, P), checked; None (an empty
        state, where the call takes one) -> (None, None, None, P)."""
        if state is None and not required:
            return None, None, None, P
        if not isinstance(state, (tuple, list)) or len(state) != 3 or not isinstance(state[0], torch.Tensor):
            raise ValueError(f"{what}: state must be (count [P] int64, mean [P, {self.D}], m2 [P, {self.D}])"
                             f"{'' if required else ' or None'}, got {type(state)}")
        count, mean, m2 = state
        if P is None:
            P = int(count.shape[0]) if count.dim() == 1 else 0
            if P < 1:
                raise ValueError(f"{what}: state: count must be an int64 tensor [P] with P >= 1, got {tuple(count.shape)}")
        self._outs(what, ((count, (P,), torch.int64, "state: count"), (mean, (P, self.D), None, "state: mean"),
                          (m2, (P, self.D), None, "state: m2")))
        if mean is None or m2 is None:
            raise ValueError(f"{what}: state: count, mean and m2 go together")
        return count, mean, m2, P

    def obs_stats_into(self, obs, count, mean, m2, lane_sum, lane_count, *, policies: int = 1, obs0=None, length=None, state=None,
                       steps=None, valid=None):
        """Allocation-free merge of one batch of observations into the running mean and deviation of P = policies policies, on
        tensors in the kernel's layouts (include/os2r_norm.h: os2rz_obs_stats; the arithmetic and its order are spelled out
        there).  With S samples, N = S P lanes (lane s P + p: sample s of policy p) and K steps: obs [K, N, D], obs0 [N, D]
        (None: obs[k] is what step k's action saw), length [N] int32 (None: K) and state = (count [P] int64, mean [P, D],
        m2 [P, D]) (None: empty) are read; count [P] int64, mean [P, D], m2 [P, D], lane_sum [2 D, N] and lane_count [2, N] int32
        (all five required: the second launch reads what the first wrote into the last two) and steps, valid [P] int32 (each or
        None) are written.  An output may not overlap an input: the caller swaps two states.  Shapes, dtypes, device, contiguity
        and overlap are checked before the library is called (it takes addresses)."""
        what = "obs_stats"
        K, N, S, P = self._pg_lanes(what, obs, policies)
        c_in, m_in, q_in, _ = self._norm_state(what, state, P, required=False)
        if any(t is None for t in (count, mean, m2, lane_sum, lane_count)):
            raise ValueError(f"{what}: obs, count, mean, m2, lane_sum and lane_count are required")
        D, i32, i64 = self.D, torch.int32, torch.int64
        inputs = ((obs, (K, N, D), None, "obs"), (obs0, (N, D), None, "obs0"), (length, (N,), i32, "length"),
                  (c_in, (P,), i64, "state: count"), (m_in, (P, D), None, "state: mean"), (q_in, (P, D), None, "state: m2"))
        outputs = ((count, (P,), i64, "count"), (mean, (P, D), None, "mean"), (m2, (P, D), None, "m2"), (steps, (P,), i32, "steps"),
                   (valid, (P,), i32, "valid"), (lane_sum, (2 * D, N), None, "lane_sum"), (lane_count, (norm.LANE_COUNTS, N), i32, "lane_count"))
        self._outs(what, inputs + outputs)
        self._no_overlap(what, inputs, outputs)
        _call(norm, "os2rz_obs_stats", "os2rz_last_error", C.byref(self._layout()), K, P, S, 0, _ptr(obs), _ptr(obs0), _ptr(length),
              _ptr(c_in), _ptr(m_in), _ptr(q_in), _ptr(count), _ptr(mean), _ptr(m2), _ptr(steps), _ptr(valid), _ptr(lane_sum),
              _ptr(lane_count), self._stream())

    def obs_stats(self, obs, *, policies: int = 1, obs0=None, length=None, state=None):
        """The running mean and deviation of every observation component of P = policies policies after one more batch, in one
        call (include/os2r_norm.h: os2rz_obs_stats): obs [K, N, D] and length [N] int32 are what
        rollout_policy(want_outputs=True) returned, obs0 [N, D] what reset() or the previous window's last step returned (None:
        obs[k] is what step k saw), all taken without a copy; lane s P + p is sample s of policy p.  state is None (nothing seen
        yet) or the (count [P] int64, mean [P, D], m2 [P, D]) an earlier call returned: m2 is the sum of squared deviations, so
        the variance is m2 / count.  The batch's sums are taken about the running mean (or, for an empty state, about the first
        observation), which keeps float32 exact where a component's mean is large beside its deviation, and merged by Chan's
        formula.  A lane one of whose sums is not finite is left out; a policy without a counted step keeps its state.
        -> (state: new tensors, the one given is left as it is; steps [P] int32: the counted steps of the batch; valid [P]
        int32: the valid lanes).  norm_fold(theta, state) gives the weights rollout_policy takes for a policy theta on whitened
        observations, norm_unfold(grad, state) takes a gradient back."""
        what = "obs_stats"
        K, N, S, P = self._pg_lanes(what, obs, policies)                    # (here too: they size what is allocated)
        D, i32 = self.D, torch.int32
        count, mean, m2 = self._new(P, dtype=torch.int64), self._new(P, D), self._new(P, D)
        steps, valid = self._new(P, dtype=i32), self._new(P, dtype=i32)
        self.obs_stats_into(obs, count, mean, m2, self._new(2 * D, N), self._new(norm.LANE_COUNTS, N, dtype=i32), policies=P, obs0=obs0,
                            length=length, state=state, steps=steps, valid=valid)
        return (count, mean, m2), steps, valid

    def _norm_sets(self, what, t, name, Q=None):
        """theta, weights or a gradient of the allocating whitening calls, [Q, rows, D+1] or [Q, D+1] (one row: value weights) ->
        (the tensor as the kernel takes it, policy_fastest, the function that gives a kernel tensor the caller's shape back).  A
        permuted view of the kernel's [rows, D+1, Q] (what policy_gradient and value_fit return) goes on without a copy."""
        n = self.D + 1
        if not isinstance(t, torch.Tensor) or t.dim() not in (2, 3) or t.shape[-1] != n or t.shape[0] < 1 or (t.dim() == 3 and t.shape[1] not in (1, 2)):
            raise ValueError(f"{what}: {name} must be a tensor [Q, 2, {n}], [Q, 1, {n}] or [Q, {n}] with Q >= 1, got "
                             f"{tuple(getattr(t, 'shape', ())) or type(t)}")
        if t.dtype != self.dtype or t.device != self.device:
            raise ValueError(f"{what}: {name} must be {self.dtype} on {self.device}, got {t.dtype} on {t.device}")
        if Q is not None and int(t.shape[0]) != Q:
            raise ValueError(f"{what}: {name} must hold {Q} sets, got {int(t.shape[0])}")
        flat = t.dim() == 2
        full = t.unsqueeze(1) if flat else t                              # [Q, rows, D+1]
        if not full.is_contiguous() and full.permute(1, 2, 0).is_contiguous():
            back = (lambda k: k.permute(2, 0, 1).squeeze(1)) if flat else (lambda k: k.permute(2, 0, 1))
            return full.permute(1, 2, 0), True, back
        return full.contiguous(), False, ((lambda k: k.squeeze(1)) if flat else (lambda k: k))

    def _norm_call(self, what, entry, source, state, out, std_floor, lanes, policy_fastest, names):
        """What norm_fold_into and norm_unfold_into share: the checks of the state, the scale and the two arrays, and the call."""
        count, mean, m2, P = self._norm_state(what, state)
        floor = _finite(what, "std_floor", math.nan if isinstance(std_floor, bool) else std_floor, lambda x: x > 0.0, "> 0", repr(std_floor))
        if self.dtype == torch.float32 and float(torch.tensor(floor, dtype=torch.float32)) == 0.0:
            raise ValueError(f"{what}: std_floor must be finite and > 0 in float32, got {std_floor!r}")
        Q = P
        if lanes is not None:
            Q = _count(what, "lanes", lanes)
            _split(what, Q, P, "lanes", "policies")
            if Q > 2 ** 31 - 1:
                raise ValueError(f"{what}: {Q} lanes exceed what an int32 holds")
        if source is None or out is None:
            raise ValueError(f"{what}: {names[0]} and {names[1]} are required")
        n = self.D + 1
        fastest = bool(policy_fastest)
        if not isinstance(source, torch.Tensor) or source.dim() != 3 or source.shape[0 if fastest else 1] not in (1, 2):
            raise ValueError(f"{what}: {names[0]} must be a tensor [{Q}, rows, {n}], or [rows, {n}, {Q}] with policy_fastest, rows 1 or 2, "
                             f"got {tuple(getattr(source, 'shape', ())) or type(source)}")
        rows = int(source.shape[0 if fastest else 1])
        shape = (rows, n, Q) if fastest else (Q, rows, n)
        inputs = ((count, (P,), torch.int64, "state: count"), (mean, (P, self.D), None, "state: mean"), (m2, (P, self.D), None, "state: m2"),
                  (source, shape, None, names[0]))
        outputs = ((out, shape, None, names[1]),)
        self._outs(what, inputs + outputs)
        self._no_overlap(what, inputs, outputs)
        flags = (norm.POLICY_FASTEST if fastest else 0) | (norm.PER_LANE if lanes is not None else 0)
        head = (C.byref(self._layout()), P) + ((Q,) if entry == "os2rz_fold" else ()) + (rows, flags)
        _call(norm, entry, "os2rz_last_error", *head, _ptr(count), _ptr(mean), _ptr(m2), floor, _ptr(source), _ptr(out), self._stream())

    def norm_fold_into(self, theta, state, weights, *, std_floor: float = 1e-6, lanes=None, policy_fastest: bool = False):
        """Allocation-free fold of policies given on whitened observations into weights on raw ones, in one launch, on tensors in
        the kernel's layouts (include/os2r_norm.h: os2rz_fold; the arithmetic is spelled out there).  state = (count [P] int64,
        mean [P, D], m2 [P, D]) as obs_stats returns it and theta are read, weights is written; both are [Q, rows, D+1] or, with
        policy_fastest, [rows, D+1, Q], rows 2 for a policy or 1 for value weights.  Q = P, set p under the statistics of policy
        p; with lanes = N (a multiple of P) Q = N, set l under those of policy l mod P -- what es_perturb writes and what the
        per-environment rollout_policy reads.  std_floor > 0 bounds the deviation from below.  A policy with count < 2 is copied
        through.  Shapes, dtypes, device, contiguity and overlap are checked before the library is called (it takes addresses)."""
        self._norm_call("norm_fold", "os2rz_fold", theta, state, weights, std_floor, lanes, policy_fastest, ("theta", "weights"))

    def norm_fold(self, theta, state, *, std_floor: float = 1e-6, lanes=None):
        """The weights W, b with W . x + b = theta . [(x - mean) / std; 1], in one launch (include/os2r_norm.h: os2rz_fold): theta
        [P, 2, D+1] holds P policies on whitened observations (or [P, D+1]: value weights, one row), state is what obs_stats
        returned, std = max(sqrt(m2 / count), std_floor).  With lanes = N theta is [N, 2, D+1], one set per lane as es_perturb
        returns it, lane l under the statistics of policy l mod P.  A permuted view of the kernel's [rows, D+1, Q] layout (a
        gradient-shaped tensor, or value_fit's weights) is taken without a copy and the result has the same layout, so it goes
        into rollout_policy or gae as it is.  A policy that has seen fewer than two observations is returned unchanged.
        -> weights, shaped like theta."""
        what = "norm_fold"
        _, _, _, P = self._norm_state(what, state)
        Q = P if lanes is None else _count(what, "lanes", lanes)
        source, fastest, back = self._norm_sets(what, theta, "theta", Q)
        out = torch.empty_like(source)
        self.norm_fold_into(source, state, out, std_floor=std_floor, lanes=lanes, policy_fastest=fastest)
        return back(out)

    def norm_unfold_into(self, grad, state, grad_theta, *, std_floor: float = 1e-6, policy_fastest: bool = False):
        """Allocation-free chain rule back through norm_fold, in one launch, on tensors in the kernel's layouts
        (include/os2r_norm.h: os2rz_unfold): grad, the gradient with respect to the folded weights, is read and grad_theta, the
        gradient with respect to theta, is written; both are [P, rows, D+1] or, with policy_fastest, [rows, D+1, P] -- the layout
        policy_gradient_into and ppo_gradient_into write.  state and std_floor are those of the fold.  Shapes, dtypes, device,
        contiguity and overlap are checked before the library is called (it takes addresses)."""
        self._norm_call("norm_unfold", "os2rz_unfold", grad, state, grad_theta, std_floor, None, policy_fastest, ("grad", "grad_theta"))

    def norm_unfold(self, grad, state, *, std_floor: float = 1e-6):
        """The gradient with respect to theta of a function of the weights norm_fold(theta, state) gave, from its gradient with
        respect to those weights, in one launch (include/os2r_norm.h: os2rz_unfold): grad [P, 2, D+1] as policy_gradient or
        ppo_gradient return it (their permuted view of the kernel's layout is taken without a copy), or [P, D+1].
        gtheta[j, d] = (g[j, d] - g[j, D] mean_d) / std_d, gtheta[j, D] = g[j, D].  A step (natural_step's) is not a gradient
        and is not mapped: the natural gradient is invariant under the reparametrisation.
        -> grad_theta, shaped like grad."""
        what = "norm_unfold"
        _, _, _, P = self._norm_state(what, state)
        source, fastest, back = self._norm_sets(what, grad, "grad", P)
        out = torch.empty_like(source)
        self.norm_unfold_into(source, state, out, std_floor=std_floor, policy_fastest=fastest)
        return back(out)

    # -- system identification: the parameter lanes, and the Gauss-Newton / Levenberg-Marquardt update -------
    def _sysid_steps(self, what, sel, h, lo, hi):
        """The identified parameters: sel, P pairs (field, index) or None (where the call does not read them), and the steps and
        bounds h, lo, hi, P numbers each -> (P, sel as int32 [2 P] or None, h, lo, hi as double [P]), checked."""
        def numbers(name, v):
            try:
                items = list(v.tolist() if hasattr(v, "tolist") else v)
                out = [float(x) for x in items]
            except (TypeError, ValueError):
                raise ValueError(f"{what}: {name} must be a sequence of numbers, got {type(v)}") from None
            if any(isinstance(x, bool) for x in items):
                raise ValueError(f"{what}: {name} must be a sequence of numbers, got a bool")
            return out

        def rounded(x):
            """x as the library rounds it: once, to the handle's dtype."""
            return x if self.dtype == torch.float64 else float(torch.tensor(x, dtype=torch.float64).to(torch.float32))
        h, lo, hi = numbers("h", h), numbers("lo", lo), numbers("hi", hi)
        P = len(h)
        if not 1 <= P <= sysid.MAX_PARAMS or len(lo) != P or len(hi) != P:
            raise ValueError(f"{what}: h, lo and hi must hold one entry for each of 1..{sysid.MAX_PARAMS} parameters, got {P}, {len(lo)} and {len(hi)}")
        for p in range(P):
            if not math.isfinite(h[p]) or not h[p] > 0.0 or not math.isfinite(rounded(h[p])) or not rounded(h[p]) > 0.0:
                raise ValueError(f"{what}: h[{p}] must be finite and > 0 in the handle's dtype, got {h[p]}")
            if math.isnan(lo[p]) or math.isnan(hi[p]) or lo[p] > hi[p]:
                raise ValueError(f"{what}: lo[{p}] <= hi[{p}] must hold (infinite bounds are allowed), got {lo[p]} and {hi[p]}")
        pairs = None
        if sel is not None:
            try:
                flat = [(f, i) for f, i in sel]
            except (TypeError, ValueError):
                raise ValueError(f"{what}: sel must be a sequence of (field, index) pairs, got {sel!r}") from None
            if len(flat) != P:
                raise ValueError(f"{what}: sel names {len(flat)} parameters, h holds {P}")
            seen = set()
            for f, i in flat:
                if any(isinstance(x, bool) or not isinstance(x, int) for x in (f, i)) or f not in sysid.FIELDS \
                        or not 0 <= i < (1 if f == abi.PARAM_GRAVITY else self.nq):
                    raise ValueError(f"{what}: sel: ({f!r}, {i!r}) is no entry of a parameter field of a chain of {self.nq} dofs")
                if (f, i) in seen:
                    raise ValueError(f"{what}: sel names ({f}, {i}) twice")
                seen.add((f, i))
            pairs = (C.c_int32 * (2 * P))(*[x for pair in flat for x in pair])
        dbl = C.c_double * P
        return P, pairs, dbl(*h), dbl(*lo), dbl(*hi)

    def _sysid_sets(self, what, theta, P):
        """theta [T, P] -> T."""
        if not isinstance(theta, torch.Tensor) or theta.dim() != 2 or not 1 <= theta.shape[0] <= sysid.MAX_SETS or theta.shape[1] != P:
            raise ValueError(f"{what}: theta must be a tensor [T, {P}] with T in 1..2^26 - 1, got {tuple(getattr(theta, 'shape', ()))}")
        return int(theta.shape[0])

    def _sysid_state(self, what, state, T, P, name="state"):
        """state = (theta_best [T, P], cost_best [T], hess [T, P, P], grad [T, P], lam [T], status [T] int32, iters [T] int32)
        -> its rows as _outs takes them, checked."""
        if not isinstance(state, (tuple, list)) or len(state) != 7 or any(t is None for t in state):
            raise ValueError(f"{what}: {name} must be (theta_best [T, P], cost_best [T], hess [T, P, P], grad [T, P], lam [T], status [T] int32, "
                             f"iters [T] int32), got {type(state)}")
        shapes = ((T, P), (T,), (T, P, P), (T, P), (T,), (T,), (T,))
        dtypes = (None,) * 5 + (torch.int32,) * 2
        rows = tuple((t, shape, dtype, f"{name}: {n}") for t, shape, dtype, n in zip(state, shapes, dtypes, sysid.STATE))
        self._outs(what, rows)
        return rows

    def sysid_init(self, theta0, lam0: float = 1e-3):
        """The state of T parameter sets that start at theta0 [T, P] with the damping lam0 (a float > 0): -> (theta_best = theta0,
        cost_best [T] = +inf, hess [T, P, P] = 0, grad [T, P] = 0, lam [T] = lam0, status [T] int32 = 0, iters [T] int32 = 0), new
        tensors in the handle's dtype.  The first point sysid_perturb takes is theta0 itself."""
        what = "sysid_init"
        if not isinstance(theta0, torch.Tensor) or theta0.dim() != 2 or theta0.shape[0] < 1 or not 1 <= theta0.shape[1] <= sysid.MAX_PARAMS:
            raise ValueError(f"{what}: theta0 must be a tensor [T, P] with T >= 1 and P in 1..{sysid.MAX_PARAMS}, got "
                             f"{tuple(getattr(theta0, 'shape', ()))}")
        T, P = int(theta0.shape[0]), int(theta0.shape[1])
        lam = _finite(what, "lam0", math.nan if isinstance(lam0, bool) else lam0, _invertible, "> 0", repr(lam0))
        new = lambda shape, value, dtype=None: torch.full(shape, value, dtype=dtype or self.dtype, device=self.device)
        return (self._in(theta0, (T, P)).clone(), new((T,), math.inf), new((T, P, P), 0.0), new((T, P), 0.0), new((T,), lam),
                new((T,), 0, torch.int32), new((T,), 0, torch.int32))

    def sysid_perturb_into(self, theta, base, params, *, sel, h, lo, hi):
        """Allocation-free parameter lanes of one identification step (include/os2r_sysid.h: os2ri_perturb; one launch).  theta
        [T, P] (the point of every set) and base [4 nq + 1, M] (the packed parameters of the M segments, sysid.pack; segment m
        belongs to set m mod T) are read; params [4 nq + 1, N], N = (2 P + 1) M, is written: lane s M + m gets base[:, m] with the
        identified entries sel[p] = (field, index) at theta (s = 0 and every lane not their own), at min(theta + h, hi)
        (s = 1 + p) or at max(theta - h, lo) (s = 1 + P + p).  sysid.field_view(params, nq, f) is what set_params(f, ...) takes,
        without a copy.  Shapes, dtypes, device, contiguity and overlap are checked before the library is called."""
        what = "sysid_perturb"
        P, pairs, hs, los, his = self._sysid_steps(what, sel, h, lo, hi)
        if sel is None:
            raise ValueError(f"{what}: sel is required")
        T = self._sysid_sets(what, theta, P)
        F = sysid.rows(self.nq)
        if not isinstance(base, torch.Tensor) or base.dim() != 2 or base.shape[1] < 1 or base.shape[1] % T:
            raise ValueError(f"{what}: base must be a tensor [{F}, M] with M a multiple of the {T} sets, got {tuple(getattr(base, 'shape', ()))}")
        M = int(base.shape[1])
        if (2 * P + 1) * M > 2 ** 31 - 1 or F * (2 * P + 1) * M > 2 ** 32 - 1:
            raise ValueError(f"{what}: (2 P + 1) M = {(2 * P + 1) * M} lanes exceed 2^31 - 1, or their {F} rows 2^32 - 1 entries")
        if params is None:
            raise ValueError(f"{what}: params is required")
        inputs = ((theta, (T, P), None, "theta"), (base, (F, M), None, "base"))
        outputs = ((params, (F, (2 * P + 1) * M), None, "params"),)
        self._outs(what, inputs + outputs)
        self._no_overlap(what, inputs, outputs)
        _call(sysid, "os2ri_perturb", "os2ri_last_error", C.byref(self._layout()), P, T, M, pairs, hs, los, his, _ptr(theta), _ptr(base),
              _ptr(params), self._stream())

    def sysid_perturb(self, theta, base, *, sel, h, lo, hi):
        """The parameter lanes of one identification step in one launch (include/os2r_sysid.h: os2ri_perturb): theta [T, P] is what
        sysid_init started at or sysid_update returned as theta_next, base [4 nq + 1, M] the packed parameters of the segments.
        -> params [4 nq + 1, (2 P + 1) M]; the loop goes on with set_params(f, sysid.field_view(params, nq, f)) for the five
        fields, set_state, rollout(K, actions) and sysid_update."""
        what = "sysid_perturb"
        P, _, _, _, _ = self._sysid_steps(what, sel, h, lo, hi)
        self._sysid_sets(what, theta, P)
        if not isinstance(base, torch.Tensor) or base.dim() != 2 or base.shape[1] < 1 or (2 * P + 1) * base.shape[1] > 2 ** 31 - 1:
            raise ValueError(f"{what}: base must be a tensor [{sysid.rows(self.nq)}, M], got {tuple(getattr(base, 'shape', ()))}")
        params = self._new(sysid.rows(self.nq), (2 * P + 1) * int(base.shape[1]))
        self.sysid_perturb_into(theta, base, params, sel=sel, h=h, lo=lo, hi=hi)
        return params

    def sysid_update_into(self, obs, meas, prec, theta, state, state_new, theta_next, sums, counts, *, h, lo, hi, constants, done=None,
                          cost=None, valid=None, accepted=None, failed=None, delta=None):
        """Allocation-free Levenberg-Marquardt update of T parameter sets from the rollout of their lanes (include/os2r_sysid.h:
        os2ri_update; three stream-ordered launches, no host synchronisation; the arithmetic and its order are spelled out
        there).  obs [K, N, D] (the rollout of the lanes of sysid_perturb), meas [K, M, D] (the logged observations; a reading
        that is not finite is skipped), prec [D] (a slot whose weight is not finite and > 0 is dropped), theta [T, P] and h, lo,
        hi (those of the sysid_perturb call that made the lanes), done [K, N] uint8 (or None) and state are read; constants is a
        sysid.Os2riConstants (sysid.constants()).  state_new (seven tensors as state) and theta_next [T, P] (the point the next
        sysid_perturb takes) are written, and cost [T], valid [T] int32, accepted [T] uint8, failed [T] int32 and delta [T, P]
        (each or None); sums [E (M + T)] with E = P (P + 1) / 2 + P + 1 and counts [M + T] int32 are the call's scratch.  A segment
        counts iff none of its lanes was done in the K steps and all its sums are finite.  A point is accepted iff it costs less
        than the best so far; a rejected one raises lam by the factor grow, an accepted one lowers it; either way the next
        point is the best one plus the damped Gauss-Newton step of the system stored with it, clamped to [lo, hi].  A set
        whose status is not 0 (1: converged, 2: lam passed lam_max) passes through.  An output may not overlap an input or
        another output: the caller swaps two states."""
        what = "sysid_update"
        P, _, hs, los, his = self._sysid_steps(what, None, h, lo, hi)
        T = self._sysid_sets(what, theta, P)
        if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or not isinstance(meas, torch.Tensor) or meas.dim() != 3 or meas.shape[1] < 1 \
                or meas.shape[1] % T or obs.shape[0] < 1:
            raise ValueError(f"{what}: obs must be a tensor [K, N, {self.D}] and meas a tensor [K, M, {self.D}] with M a multiple of the {T} sets, "
                             f"got {tuple(getattr(obs, 'shape', ()))} and {tuple(getattr(meas, 'shape', ()))}")
        K, M = int(obs.shape[0]), int(meas.shape[1])
        N, E, D, i32 = (2 * P + 1) * M, P * (P + 1) // 2 + P + 1, self.D, torch.int32
        if N > 2 ** 31 - 1:
            raise ValueError(f"{what}: (2 P + 1) M = {N} lanes exceed 2^31 - 1")
        if not isinstance(constants, sysid.Os2riConstants):
            raise ValueError(f"{what}: constants must be a sysid.Os2riConstants (sysid.constants() makes one), got {type(constants)}")
        for name in sysid.CONSTANT_NAMES:
            if not math.isfinite(getattr(constants, name)):
                raise ValueError(f"{what}: constants.{name} must be finite, got {getattr(constants, name)}")
        if constants.lam_min < 0.0 or not constants.diag_floor > 0.0:
            raise ValueError(f"{what}: constants.lam_min must be >= 0 and constants.diag_floor > 0, got {constants.lam_min} and {constants.diag_floor}")
        if any(t is None for t in (prec, theta_next, sums, counts)):
            raise ValueError(f"{what}: prec, theta_next, sums and counts are required")
        rows = self._sysid_state(what, state, T, P)
        out_rows = self._sysid_state(what, state_new, T, P, "state_new")
        inputs = ((obs, (K, N, D), None, "obs"), (meas, (K, M, D), None, "meas"), (done, (K, N), torch.uint8, "done"), (prec, (D,), None, "prec"),
                  (theta, (T, P), None, "theta")) + rows
        outputs = out_rows + ((theta_next, (T, P), None, "theta_next"), (cost, (T,), None, "cost"), (valid, (T,), i32, "valid"),
                              (accepted, (T,), torch.uint8, "accepted"), (failed, (T,), i32, "failed"), (delta, (T, P), None, "delta"),
                              (sums, (E * (M + T),), None, "sums"), (counts, (M + T,), i32, "counts"))
        self._outs(what, inputs + outputs)
        self._no_overlap(what, inputs, outputs)
        _call(sysid, "os2ri_update", "os2ri_last_error", C.byref(self._layout()), P, T, M, K, hs, los, his, C.byref(constants), _ptr(obs), _ptr(meas),
              _ptr(done), _ptr(prec), _ptr(theta), *[_ptr(t) for t in state], *[_ptr(t) for t in state_new], _ptr(theta_next), _ptr(cost),
              _ptr(valid), _ptr(accepted), _ptr(failed), _ptr(delta), _ptr(sums), _ptr(counts), self._stream())

    def sysid_update(self, obs, meas, prec, theta, state, *, h, lo, hi, constants=None, done=None, want_info: bool = True):
        """One Levenberg-Marquardt step of T parameter sets (include/os2r_sysid.h: os2ri_update): obs [K, N, D] and done [K, N] are
        what rollout(K, actions) returned for the lanes of sysid_perturb(theta, ...), as they lie on the device; meas [K, M, D]
        the logged observations of the M segments, prec [D] the weights of the observation slots, state what sysid_init or the
        last sysid_update returned; h, lo and hi are those of the sysid_perturb call; constants None is sysid.constants().
        -> (state_new: seven new tensors as state; theta_next [T, P]: the point of the next sysid_perturb; info | None: (cost [T],
        valid [T] int32: the segments that counted, accepted [T] uint8, failed [T] int32: 0 or the column + 1 at which the
        factor of the damped system failed, delta [T, P]: the step))."""
        what = "sysid_update"
        P, _, _, _, _ = self._sysid_steps(what, None, h, lo, hi)
        T = self._sysid_sets(what, theta, P)
        if not isinstance(meas, torch.Tensor) or meas.dim() != 3 or meas.shape[1] < 1:
            raise ValueError(f"{what}: meas must be a tensor [K, M, {self.D}], got {tuple(getattr(meas, 'shape', ()))}")
        M, E, i32 = int(meas.shape[1]), P * (P + 1) // 2 + P + 1, torch.int32
        state_new = (self._new(T, P), self._new(T), self._new(T, P, P), self._new(T, P), self._new(T), self._new(T, dtype=i32),
                     self._new(T, dtype=i32))
        theta_next, sums, counts = self._new(T, P), self._new(E * (M + T)), self._new(M + T, dtype=i32)
        info = (self._new(T), self._new(T, dtype=i32), self._new(T, dtype=torch.uint8), self._new(T, dtype=i32), self._new(T, P)) if want_info \
            else (None,) * 5
        self.sysid_update_into(obs, meas, prec, theta, state, state_new, theta_next, sums, counts, h=h, lo=lo, hi=hi,
                               constants=sysid.constants() if constants is None else constants, done=done, cost=info[0], valid=info[1],
                               accepted=info[2], failed=info[3], delta=info[4])
        return state_new, theta_next, info if want_info else None
