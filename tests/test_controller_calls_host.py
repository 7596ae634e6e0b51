"""The controller methods of HipSim (lqr_gains, ilqr_backward, ilqr_line_search, ilqr_steer, mppi_update, pf_update and
their *_into forms) held in place without a device: what each call passes to C, position by position, and the exception of
every call that is valid but for one argument.

(a) A recorder stands where each library would be.  The order of the 16 to 29 positional arguments of every entry point is
written out below by hand, read off the prototypes in include/os2r*.h; each recorded address, integer and float is mapped back
to the Python argument it must be.

(b) tests/golden/controller_errors.json holds, for every case of `_cases`, the exception type and the full message as recorded on
the commit its first key names.  That commit's controller section holds 83 `raise ValueError` sites (and gym_os2r_amd.steer.rule
four, HipSim._out and HipSim._in one each, reached from it); the table has 502 cases, run in both dtypes.  A case that
reaches a library (its load() or the recorder) instead of raising fails.  To record again after a message was changed on
purpose: `PYTHONPATH=. python tests/test_controller_calls_host.py`.
"""
import ctypes as C
import inspect
import json
import os

import pytest
import torch

from gym_os2r_amd import abi, control, mppi, pf, search, steer
from gym_os2r_amd.sim import HipSim

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "controller_errors.json")
RECORDED_ON = "recorded on"                       # the first key of the recording: the commit whose messages it holds

NQ, D, K, M = 3, 4, 3, 4
n, L, R1 = 2 * NQ, K * M, D + 1
NAL = S = 2                                       # candidates, samples and particles per robot
N = NAL * M
DTYPES = (torch.float64, torch.float32)
LOADERS = {"control": control, "search": search, "steer": steer, "mppi": mppi, "pf": pf}

# the positional arguments of every entry point, by the name of the Python argument (or value) that must stand there
ORDER = {
    "os2r_lqr_gains": ["handle", "K", "M", "sweeps", "A", "B", "q", "r", "P_final", "gains_out", "P_out", "flags_out", "actions", "obs",
                       "weights_out", "stream"],
    "os2rc_ilqr_backward": ["layout", "K", "M", "A", "B", "lx", "lu", "q", "r", "mu", "P_final", "p_final", "gains_out", "ff_out", "P_out",
                            "p_out", "flags_out", "dv_out", "actions", "obs", "alphas", "nal", "weights_out", "stream"],
    "os2rt_ilqr_backward_mu": ["layout", "K", "M", "A", "B", "lx", "lu", "q", "r", "mu_dev", "P_final", "p_final", "gains_out", "ff_out",
                               "P_out", "p_out", "flags_out", "dv_out", "actions", "obs", "alphas", "nal", "weights_out", "stream"],
    "os2rs_ilqr_line_search": ["layout", "K", "M", "nal", "flags", "knot_obs", "end_obs", "actions", "done", "target", "q", "r", "qf", "cost",
                               "act_nom", "obs_nom", "end_nom", "lx", "lu", "p_final", "choice", "index", "cand_cost", "stream"],
    "os2rt_ilqr_steer": ["layout", "K", "M", "nal", "knot_obs", "end_obs", "actions", "done", "target", "q", "r", "qf", "dv", "alphas", "rule",
                         "cost", "act_nom", "obs_nom", "end_nom", "lx", "lu", "p_final", "mu", "status", "iters", "choice", "index",
                         "cand_cost", "stream"],
    "os2rm_mppi_update": ["layout", "K", "M", "S", "returns", "actions", "nominal_in", "beta", "shift", "tail", "nominal_out", "applied",
                          "table", "weights", "ess", "count", "stream"],
    "os2rp_pf_update": ["layout", "M", "S", "obs", "meas", "prec", "logw_in", "u", "resample_ratio", "logw_out", "index", "est", "weights",
                        "ess", "count", "resampled", "stream"],
}
TABLES = {"os2r_lqr_gains": None, "os2rc_ilqr_backward": control, "os2rt_ilqr_backward_mu": steer, "os2rs_ilqr_line_search": search,
          "os2rt_ilqr_steer": steer, "os2rm_mppi_update": mppi, "os2rp_pf_update": pf}


class Recorder:
    """Stands where a library would be: every attribute is a function that keeps its positional arguments and returns OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return abi.OK
        return call


STREAM = C.c_void_p(0)


def _sim(dtype, monkeypatch, rec):
    """_bare() of tests/test_ilqr_steer_host.py with `rec` where each library would be; -> (handle, the loads reached)."""
    s = HipSim.__new__(HipSim)
    s.N, s.nq, s.D, s.dtype, s.device = N, NQ, D, dtype, torch.device("cpu")
    s._h, s._lib = C.c_void_p(0x1234), rec
    s._control_layout = control.layout(abi.F64 if dtype == torch.float64 else abi.F32, NQ, 0, [0, 1, 2, 3])
    s._stream = lambda: STREAM
    reached = []
    for name, module in LOADERS.items():
        monkeypatch.setattr(module, "load", lambda name=name: (reached.append(name), rec)[1])
    return s, reached


QV = (torch.arange(36.0, dtype=torch.float64).reshape(n, n) + torch.arange(36.0, dtype=torch.float64).reshape(n, n).T
      + 40.0 * torch.eye(n, dtype=torch.float64))
RV = [[0.5, 0.125], [0.125, 0.75]]
QF = 2.0 * QV
ALPHAS = (1.0, 0.5)
RULE = dict(armijo=1e-4, tol=1e-3)


def _valid(dt, method):
    """Keyword arguments of a call of `method` that is valid, every optional argument given and each tensor distinct."""
    z = lambda *shape, dtype=dt: torch.zeros(*shape, dtype=dtype)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)
    nominal = lambda: dict(cost=z(M), actions=z(K, M, 2), obs=z(K, M, D), end_obs=z(M, D), lx=z(n, L), lu=z(2, L), p_final=z(n, M))
    rollout = lambda: dict(knot_obs=z(K, N, D), end_obs=z(N, D), actions=z(K, N, 2), target=z(M, D), Q=QV, R=RV, done=u8(K, N), Q_final=QF)
    nom_into = lambda: dict(act_nom=z(K, M, 2), obs_nom=z(K, M, D), end_nom=z(M, D), lx=z(n, L), lu=z(2, L), p_final=z(n, M), index=i32(L),
                            cand_cost=z(NAL, M))
    return {
        "lqr_gains_into": lambda: dict(
            A=z(n, n, L), B=z(n, 2, L), Q=QV, R=RV, knots=K, sweeps=2, P_final=z(n, n, M), gains_out=z(K, 2, n, M), P_out=z(n, n, M),
            flags_out=u8(K, M), actions=z(L, 2), obs=z(L, D), weights_out=z(K, 2, R1, M)),
        "lqr_gains": lambda: dict(
            A=z(n, n, L).permute(2, 0, 1), B=z(n, 2, L).permute(2, 0, 1), Q=QV, R=RV, knots=K, sweeps=2, P_final=z(M, n, n), actions=z(L, 2),
            obs=z(L, D), want_gains=True, want_P=True, want_flags=True, want_weights=True),
        "ilqr_backward_into": lambda: dict(
            A=z(n, n, L), B=z(n, 2, L), Q=QV, R=RV, knots=K, lx=z(n, L), lu=z(2, L), mu=0.25, P_final=z(n, n, M), p_final=z(n, M),
            gains_out=z(K, 2, n, M), ff_out=z(K, 2, M), P_out=z(n, n, M), p_out=z(n, M), flags_out=u8(K, M), dv_out=z(K, 2, M),
            actions=z(L, 2), obs=z(L, D), alphas=ALPHAS, weights_out=z(K, 2, R1, NAL * M), mu_dev=None),
        "ilqr_backward": lambda: dict(
            A=z(n, n, L).permute(2, 0, 1), B=z(n, 2, L).permute(2, 0, 1), Q=QV, R=RV, knots=K, lx=z(n, L).permute(1, 0),
            lu=z(2, L).permute(1, 0), mu=0.25, P_final=z(n, n, M).permute(2, 0, 1), p_final=z(n, M).permute(1, 0), actions=z(L, 2),
            obs=z(L, D), alphas=ALPHAS, want_gains=True, want_ff=True, want_P=True, want_p=True, want_flags=True, want_dv=True,
            want_weights=True, mu_dev=None),
        "ilqr_line_search_into": lambda: dict(rollout(), cost=z(M), choice=i32(M), always=True, **nom_into()),
        "ilqr_line_search": lambda: dict(rollout(), nominal=nominal(), want_cand_cost=True),
        "ilqr_steer_into": lambda: dict(rollout(), dv=z(K, 2, M), alphas=ALPHAS, cost=z(M), mu=z(M), status=i32(M), choice=i32(M),
                                        iters=i32(M), rule=dict(RULE), shrink=0.25, **nom_into()),
        "ilqr_steer": lambda: dict(rollout(), dv=z(K, 2, M).permute(0, 2, 1), alphas=ALPHAS, nominal=nominal(), rule=dict(RULE),
                                   want_cand_cost=True, shrink=0.25),
        "mppi_update_into": lambda: dict(
            returns=z(N), actions=z(K, N, 2), nominal_in=z(K, M, 2), nominal_out=z(K, M, 2), samples=S, temperature=0.5, shift=2,
            tail="zero", applied=z(M, 2), table=z(K, 2, R1, N), weights=z(S, M), ess=z(M), count=i32(M)),
        "mppi_update": lambda: dict(
            returns=z(N), actions=z(K, N, 2), nominal=z(K, M, 2), samples=S, temperature=0.5, shift=2, tail="zero",
            table=z(K, 2, R1, N).permute(3, 0, 1, 2), want_weights=True, want_ess=True),
        "pf_update_into": lambda: dict(
            obs=z(N, D), meas=z(M, D), prec=z(D), logw_out=z(S, M), index=i32(N), particles=S, logw_in=z(S, M), u=z(M),
            resample_ratio=0.75, est=z(M, D), weights=z(S, M), ess=z(M), count=i32(M), resampled=i32(M)),
        "pf_update": lambda: dict(
            obs=z(N, D), meas=z(M, D), prec=z(D), particles=S, logw=z(S, M), u=z(M), resample_ratio=0.75, want_estimate=True,
            want_weights=True),
    }[method]()


# ---------------------------------------------------------------------------------------
# (a) what reaches C
# ---------------------------------------------------------------------------------------
def _decode(a):
    """A recorded argument as a plain value: the address of a pointer (None: null), the list of a ctypes array, the object
    behind a byref(); anything else as it is."""
    if isinstance(a, C.c_void_p):
        return a.value
    if isinstance(a, C.Array):
        return list(a)
    return getattr(a, "_obj", a)


def _held(rec, s, entry, kw, **special):
    """The newest recorded call is `entry`, as long as its row of ENTRY_POINTS, and holds in every position what ORDER names:
    the address of that tensor of `kw` (null where it is None) or the value of `special`."""
    name, args = rec.calls[-1]
    assert name == entry
    table = _lib_table(entry)
    assert len(args) == len(table[entry]) == len(ORDER[entry])
    special = dict(special, K=K, M=M, q=QV.reshape(-1).tolist(), r=[v for row in RV for v in row])
    for i, (what, got) in enumerate(zip(ORDER[entry], args)):
        where = f"{entry}, argument {i} ({what})"
        if what == "stream":
            assert got is STREAM, where
        elif what == "handle":
            assert got is s._h, where
        elif what == "layout":
            assert _decode(got) is s._control_layout, where
        elif what == "rule":
            rule = _decode(got)
            assert {k: getattr(rule, k) for k in steer.RULE_DEFAULTS} == special["rule"], where
        elif what in special:
            assert _decode(got) == special[what] and type(_decode(got)) is type(special[what]), where
        else:
            assert _decode(got) == (None if kw[what] is None else kw[what].data_ptr()), where


def _lib_table(entry):
    from gym_os2r_amd import _lib
    return _lib.ENTRY_POINTS if TABLES[entry] is None else TABLES[entry].ENTRY_POINTS


def _distinct(kw):
    ptrs = [v.data_ptr() for v in kw.values() if isinstance(v, torch.Tensor)]
    assert len(set(ptrs)) == len(ptrs)


def _without(kw, *names):
    return dict(kw, **{k: None for k in names})


@pytest.mark.parametrize("dt", DTYPES, ids=str)
def test_the_order_of_what_every_into_call_passes_to_c(dt, monkeypatch):
    rec = Recorder()
    s, reached = _sim(dt, monkeypatch, rec)
    qf, al = QF.reshape(-1).tolist(), list(ALPHAS)
    rule = {k: getattr(steer.rule(RULE, shrink=0.25), k) for k in steer.RULE_DEFAULTS}

    kw = _valid(dt, "lqr_gains_into")
    _distinct(kw)
    s.lqr_gains_into(**kw)
    _held(rec, s, "os2r_lqr_gains", kw, sweeps=2)
    kw = _without(kw, "P_final", "P_out", "flags_out", "weights_out")
    s.lqr_gains_into(**kw)                         # actions and obs are given: without weights_out they do not reach the library
    _held(rec, s, "os2r_lqr_gains", _without(kw, "actions", "obs"), sweeps=2)
    assert reached == []

    kw = _valid(dt, "ilqr_backward_into")
    _distinct(kw)
    s.ilqr_backward_into(**kw)
    _held(rec, s, "os2rc_ilqr_backward", kw, mu=0.25, alphas=al, nal=NAL)
    kw_mu = dict(kw, mu=0.0, mu_dev=torch.zeros(M, dtype=dt))
    s.ilqr_backward_into(**kw_mu)
    _held(rec, s, "os2rt_ilqr_backward_mu", kw_mu, alphas=al, nal=NAL)
    optional = ("lx", "lu", "P_final", "p_final", "ff_out", "P_out", "p_out", "flags_out", "dv_out", "weights_out")
    s.ilqr_backward_into(**_without(kw, *optional))
    _held(rec, s, "os2rc_ilqr_backward", _without(kw, "actions", "obs", *optional), mu=0.25, alphas=None, nal=0)
    s.ilqr_backward_into(**_without(kw_mu, *optional))
    _held(rec, s, "os2rt_ilqr_backward_mu", _without(kw_mu, "actions", "obs", *optional), alphas=None, nal=0)
    assert reached == ["control", "steer", "control", "steer"]

    kw = _valid(dt, "ilqr_line_search_into")
    _distinct(kw)
    s.ilqr_line_search_into(**kw)
    _held(rec, s, "os2rs_ilqr_line_search", kw, nal=NAL, flags=search.ACCEPT_ALWAYS, qf=qf)
    kw = _without(kw, "done", "Q_final", "act_nom", "obs_nom", "end_nom", "lx", "lu", "p_final", "index", "cand_cost")
    del kw["always"]
    s.ilqr_line_search_into(**kw)
    _held(rec, s, "os2rs_ilqr_line_search", kw, nal=NAL, flags=0, qf=None)

    kw = _valid(dt, "ilqr_steer_into")
    _distinct(kw)
    s.ilqr_steer_into(**kw)
    _held(rec, s, "os2rt_ilqr_steer", kw, nal=NAL, qf=qf, alphas=al, rule=rule)
    kw = _without(kw, "iters", "done", "Q_final", "rule", "act_nom", "obs_nom", "end_nom", "lx", "lu", "p_final", "index", "cand_cost")
    del kw["shrink"]
    s.ilqr_steer_into(**kw)
    _held(rec, s, "os2rt_ilqr_steer", kw, nal=NAL, qf=None, alphas=al, rule=steer.RULE_DEFAULTS)

    kw = _valid(dt, "mppi_update_into")
    _distinct(kw)
    s.mppi_update_into(**kw)
    _held(rec, s, "os2rm_mppi_update", kw, S=S, beta=1.0 / 0.5, shift=2, tail=mppi.TAILS["zero"])
    kw = _without(kw, "applied", "table", "weights", "ess", "count")
    del kw["shift"], kw["tail"]
    s.mppi_update_into(**kw)
    _held(rec, s, "os2rm_mppi_update", kw, S=S, beta=1.0 / 0.5, shift=1, tail=mppi.TAILS["hold"])

    kw = _valid(dt, "pf_update_into")
    _distinct(kw)
    s.pf_update_into(**kw)
    _held(rec, s, "os2rp_pf_update", kw, S=S, resample_ratio=0.75)
    kw = _without(kw, "logw_in", "u", "est", "weights", "ess", "count", "resampled")
    del kw["resample_ratio"]
    s.pf_update_into(**kw)
    _held(rec, s, "os2rp_pf_update", kw, S=S, resample_ratio=0.5)
    assert reached[4:] == ["search", "search", "steer", "steer", "mppi", "mppi", "pf", "pf"] and len(rec.calls) == 14


def _spy(monkeypatch, method):
    """Keep the keyword form of every call of HipSim.<method>, then make it; -> the list of them."""
    seen, real = [], getattr(HipSim, method)

    def spy(self, *args, **kw):
        bound = inspect.signature(real).bind(self, *args, **kw)
        bound.apply_defaults()
        seen.append({k: v for k, v in bound.arguments.items() if k != "self"})
        seen[-1].update(seen[-1].pop("rule_kw", {}))
        return real(self, *args, **kw)
    monkeypatch.setattr(HipSim, method, spy)
    return seen


def _kernel_layout(kw, dt, shapes):
    """Every tensor of the *_into call `kw` is contiguous, and has the shape and dtype of `shapes` (dtype None: the handle's)."""
    tensors = {k for k, v in kw.items() if isinstance(v, torch.Tensor) and k not in ("Q", "Q_final")}
    assert tensors == set(shapes)
    for name, (shape, dtype) in shapes.items():
        t = kw[name]
        assert tuple(t.shape) == shape and t.dtype == (dtype or dt) and t.is_contiguous(), name


def _views(got, dt, shapes):
    assert len(got) == len(shapes)
    for t, (shape, dtype) in zip(got, shapes):
        assert tuple(t.shape) == shape and t.dtype == (dtype or dt)


@pytest.mark.parametrize("dt", DTYPES, ids=str)
def test_what_the_allocating_wrappers_hand_to_their_into_form(dt, monkeypatch):
    rec = Recorder()
    s, _ = _sim(dt, monkeypatch, rec)
    qf, al, u8, i32 = QF.reshape(-1).tolist(), list(ALPHAS), torch.uint8, torch.int32
    same = lambda a, b: a.data_ptr() == b.data_ptr()

    seen = _spy(monkeypatch, "lqr_gains_into")
    kw = _valid(dt, "lqr_gains")
    got = s.lqr_gains(**kw)
    _kernel_layout(seen[0], dt, dict(A=((n, n, L), None), B=((n, 2, L), None), P_final=((n, n, M), None), gains_out=((K, 2, n, M), None),
                                     P_out=((n, n, M), None), flags_out=((K, M), u8), actions=((L, 2), None), obs=((L, D), None),
                                     weights_out=((K, 2, R1, M), None)))
    _held(rec, s, "os2r_lqr_gains", seen[0], sweeps=2)
    _views(got, dt, [((K, M, 2, n), None), ((M, n, n), None), ((K, M), u8), ((M, K, 2, R1), None)])
    # what linearize() returned goes on without a copy, and so do actions and obs
    assert same(seen[0]["A"], kw["A"]) and same(seen[0]["B"], kw["B"]) and same(seen[0]["actions"], kw["actions"]) and same(seen[0]["obs"], kw["obs"])
    assert s.lqr_gains(**dict(kw, want_gains=False, want_flags=False, want_weights=False))[::2] == (None, None)

    seen = _spy(monkeypatch, "ilqr_backward_into")
    kw = _valid(dt, "ilqr_backward")
    got = s.ilqr_backward(**kw)
    shapes = dict(A=((n, n, L), None), B=((n, 2, L), None), lx=((n, L), None), lu=((2, L), None), P_final=((n, n, M), None),
                  p_final=((n, M), None), gains_out=((K, 2, n, M), None), ff_out=((K, 2, M), None), P_out=((n, n, M), None),
                  p_out=((n, M), None), flags_out=((K, M), u8), dv_out=((K, 2, M), None), actions=((L, 2), None), obs=((L, D), None),
                  weights_out=((K, 2, R1, NAL * M), None))
    _kernel_layout(seen[0], dt, shapes)
    _held(rec, s, "os2rc_ilqr_backward", seen[0], mu=0.25, alphas=al, nal=NAL)
    _views(got, dt, [((K, M, 2, n), None), ((K, M, 2), None), ((M, n, n), None), ((M, n), None), ((K, M), u8), ((K, M, 2), None),
                     ((NAL * M, K, 2, R1), None)])
    # linearize()'s A and B and ilqr_line_search's *_view go on without a copy
    assert all(same(seen[0][k], kw[k]) for k in ("A", "B", "lx", "lu", "P_final", "p_final", "actions", "obs"))
    mu_dev = torch.zeros(M, dtype=dt)
    s.ilqr_backward(**dict(kw, mu=0.0, mu_dev=mu_dev))
    _kernel_layout(seen[1], dt, dict(shapes, mu_dev=((M,), None)))
    _held(rec, s, "os2rt_ilqr_backward_mu", seen[1], alphas=al, nal=NAL)
    assert seen[1]["mu_dev"] is mu_dev
    dv_view = got[5]

    seen = _spy(monkeypatch, "ilqr_line_search_into")
    kw = _valid(dt, "ilqr_line_search")
    del kw["nominal"]
    choice, index, cand_cost, nominal = s.ilqr_line_search(**kw)
    shapes = dict(knot_obs=((K, N, D), None), end_obs=((N, D), None), actions=((K, N, 2), None), target=((M, D), None), done=((K, N), u8),
                  cost=((M,), None), choice=((M,), i32),
                  act_nom=((K, M, 2), None), obs_nom=((K, M, D), None), end_nom=((M, D), None), lx=((n, L), None), lu=((2, L), None),
                  p_final=((n, M), None), index=((L,), i32), cand_cost=((NAL, M), None))
    _kernel_layout(seen[0], dt, shapes)
    assert seen[0]["always"] is True
    _held(rec, s, "os2rs_ilqr_line_search", seen[0], nal=NAL, flags=search.ACCEPT_ALWAYS, qf=qf)
    _views((choice, index, cand_cost), dt, [((M,), i32), ((L,), i32), ((NAL, M), None)])
    assert set(nominal) == {"cost", "actions", "obs", "end_obs", "lx", "lu", "p_final", "lx_view", "lu_view", "p_final_view"}
    _views([nominal[k] for k in ("lx_view", "lu_view", "p_final_view")], dt, [((L, n), None), ((L, 2), None), ((M, n), None)])
    assert all(same(nominal[k + "_view"], nominal[k]) for k in ("lx", "lu", "p_final")) and not any(t.any() for t in nominal.values())
    assert all(same(seen[0][k], kw[k]) for k in ("knot_obs", "end_obs", "actions", "target", "done"))
    again = s.ilqr_line_search(**dict(kw, nominal=nominal, want_cand_cost=False))
    assert again[2] is None and again[3] is nominal and seen[1]["always"] is False
    assert all(seen[1][a] is nominal[b] for a, b in (("cost", "cost"), ("act_nom", "actions"), ("obs_nom", "obs"), ("end_nom", "end_obs"),
                                                     ("lx", "lx"), ("lu", "lu"), ("p_final", "p_final")))
    _held(rec, s, "os2rs_ilqr_line_search", seen[1], nal=NAL, flags=0, qf=qf)

    seen = _spy(monkeypatch, "ilqr_steer_into")
    kw = dict(_valid(dt, "ilqr_steer"), nominal=nominal, dv=dv_view)
    choice, index, cand_cost, back = s.ilqr_steer(**kw)
    _kernel_layout(seen[0], dt, dict(shapes, dv=((K, 2, M), None), mu=((M,), None), status=((M,), i32), iters=((M,), i32)))
    _held(rec, s, "os2rt_ilqr_steer", seen[0], nal=NAL, qf=qf, alphas=al,
          rule={k: getattr(steer.rule(RULE, shrink=0.25), k) for k in steer.RULE_DEFAULTS})
    _views((choice, index, cand_cost), dt, [((M,), i32), ((L,), i32), ((NAL, M), None)])
    # the dv ilqr_backward returned goes on without a copy; mu, status and iters are added to the nominal as zeros and kept
    assert back is nominal and same(seen[0]["dv"], dv_view) and not any(nominal[k].any() for k in ("mu", "status", "iters"))
    assert all(seen[0][k] is nominal[k] for k in ("cost", "mu", "status", "iters"))
    mu = nominal["mu"]
    s.ilqr_steer(**kw)
    assert nominal["mu"] is mu and seen[1]["mu"] is mu

    seen = _spy(monkeypatch, "mppi_update_into")
    kw = _valid(dt, "mppi_update")
    applied, nom1, table, weights, ess, count = s.mppi_update(**kw)
    _kernel_layout(seen[0], dt, dict(returns=((N,), None), actions=((K, N, 2), None), nominal_in=((K, M, 2), None),
                                     nominal_out=((K, M, 2), None), applied=((M, 2), None), table=((K, 2, R1, N), None),
                                     weights=((S, M), None), ess=((M,), None), count=((M,), i32)))
    _held(rec, s, "os2rm_mppi_update", seen[0], S=S, beta=2.0, shift=2, tail=mppi.TAILS["zero"])
    _views((applied, nom1, table, weights, ess, count), dt, [((M, 2), None), ((K, M, 2), None), ((N, K, 2, R1), None), ((S, M), None),
                                                             ((M,), None), ((M,), i32)])
    assert same(seen[0]["table"], kw["table"]) and table.data_ptr() == kw["table"].data_ptr() and seen[0]["nominal_in"] is kw["nominal"]
    # the new nominal fed back: the two kept buffers alternate
    nom2 = s.mppi_update(**dict(kw, nominal=nom1, table=True, want_weights=False, want_ess=False))[1]
    out = s.mppi_update(**dict(kw, nominal=nom2, table=True))
    assert not same(nom1, nom2) and same(out[1], nom1) and seen[2]["nominal_in"] is nom2 and seen[2]["nominal_out"] is nom1
    assert tuple(out[2].shape) == (N, K, 2, R1) and same(seen[1]["table"], seen[2]["table"]) and seen[1]["table"].is_contiguous()
    assert s.mppi_update(**dict(kw, table=None, want_weights=False, want_ess=False))[2:5] == (None, None, None)

    seen = _spy(monkeypatch, "pf_update_into")
    kw = _valid(dt, "pf_update")
    logw1, index, est, weights, ess, count, resampled = got = s.pf_update(**kw)
    _kernel_layout(seen[0], dt, dict(obs=((N, D), None), meas=((M, D), None), prec=((D,), None), logw_out=((S, M), None), index=((N,), i32),
                                     logw_in=((S, M), None), u=((M,), None), est=((M, D), None), weights=((S, M), None), ess=((M,), None),
                                     count=((M,), i32), resampled=((M,), i32)))
    _held(rec, s, "os2rp_pf_update", seen[0], S=S, resample_ratio=0.75)
    _views(got, dt, [((S, M), None), ((N,), i32), ((M, D), None), ((S, M), None), ((M,), None), ((M,), i32), ((M,), i32)])
    assert all(seen[0][a] is kw[b] for a, b in (("obs", "obs"), ("meas", "meas"), ("prec", "prec"), ("logw_in", "logw"), ("u", "u")))
    logw2 = s.pf_update(**dict(kw, logw=logw1, want_estimate=False))[0]
    out = s.pf_update(**dict(kw, logw=logw2))
    assert not same(logw1, logw2) and same(out[0], logw1) and seen[2]["logw_in"] is logw2 and seen[2]["logw_out"] is logw1
    first = s.pf_update(**dict(kw, logw=None, u=None))
    assert same(first[0], logw1) and seen[3]["logw_in"] is None and seen[3]["u"] is None and seen[1]["est"] is None


# ---------------------------------------------------------------------------------------
# (b) calls that are valid but for one argument
# ---------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
# the arguments whose last axis counts the lanes: theirs is made wrong along the first
FIRST_AXIS = {("lqr_gains_into", "A"), ("lqr_gains_into", "B"), ("ilqr_backward_into", "A"), ("ilqr_backward_into", "B")}


def _bumped(t, axis=-1):
    shape = list(t.shape)
    shape[axis] += 1
    return torch.zeros(shape, dtype=t.dtype)


def _other(t):
    return t.to({torch.float64: torch.float32, torch.float32: torch.float64}.get(t.dtype, torch.int64))


def _strided(t):
    return _bumped(torch.cat([t, t], -1)).narrow(-1, 0, 2 * t.shape[-1])[..., ::2]


def _cases(dt):
    """-> {case name: (method, keyword arguments)}: every call valid but for what its name says."""
    out = {}

    def add(method, label, **changes):
        """`changes` replace arguments; one named nominal__x replaces entry x of the nominal dict."""
        kw = _valid(dt, method)
        for k, v in changes.items():
            if k.startswith("nominal__"):
                kw["nominal"][k[9:]] = v
            else:
                kw[k] = v
        assert f"{method}: {label}" not in out
        out[f"{method}: {label}"] = (method, kw)

    def tensors(method):
        kw = _valid(dt, method)
        named = [(k, v) for k, v in kw.items() if isinstance(v, torch.Tensor) and k not in ("Q", "Q_final")]
        named += [("nominal__" + k, v) for k, v in (kw.get("nominal") if isinstance(kw.get("nominal"), dict) else {}).items()]
        for k, v in named:                       # one row of a shape table each
            add(method, f"{k} one too long", **{k: _bumped(v, 0 if (method, k) in FIRST_AXIS else -1)})
            if not v.dtype.is_floating_point:
                add(method, f"{k} of another dtype", **{k: _other(v)})
        if method in ("lqr_gains", "ilqr_backward"):      # these two convert and copy what is no view of the kernel's layout
            return
        k, v = [(k, v) for k, v in named if v.dtype.is_floating_point][-1]
        add(method, f"{k} of another dtype", **{k: _other(v)})
        add(method, f"{k} not contiguous", **{k: _strided(v)})
        add(method, f"{k} a list", **{k: v.tolist()})

    def cost(method, names=("Q", "R"), every=False):
        """Every refusal of a cost matrix (`every`), or the two that show the method's name went into the message."""
        for name in names:
            k = 2 if name == "R" else n
            good = torch.eye(k, dtype=torch.float64)
            skew = good.clone()
            skew[0, 1] = 0.5
            faults = (("a string", "x"), ("None", None), ("one too long", torch.eye(k + 1)), ("not finite", NAN * good),
                      ("not symmetric", skew), ("a list that is not symmetric", skew.tolist()))
            for label, bad in faults if every else faults[2:5:2]:
                if not (name == "Q_final" and bad is None):
                    add(method, f"{name} {label}", **{name: bad})

    def riccati(method, into):
        tensors(method)
        cost(method, every=method == "lqr_gains_into")
        z = lambda *shape: torch.zeros(*shape, dtype=dt)
        add(method, "knots 0", knots=0)
        add(method, "knots no divisor of the lanes", knots=5)
        add(method, "knots more than the lanes", knots=2 * L)
        add(method, "A None", A=None)
        add(method, "A of two axes", A=z(n, n))
        add(method, "B None", B=None)
        if not into:
            add(method, "A an array", A=z(L, n, n).numpy())
            add(method, "A of another dtype", A=_other(z(L, n, n)))
            add(method, "B of two axes", B=z(L, n))
            add(method, "B of another dtype", B=_other(z(L, n, 2)))
            add(method, "B of other lanes", B=z(L + K, n, 2))
            add(method, "A of other lanes", A=z(L + K, n, n))

    riccati("lqr_gains_into", True)
    add("lqr_gains_into", "sweeps 0", sweeps=0)
    add("lqr_gains_into", "nothing asked for", gains_out=None, P_out=None, weights_out=None)
    add("lqr_gains_into", "weights without actions", actions=None)
    add("lqr_gains_into", "weights without obs", obs=None)
    riccati("lqr_gains", False)
    add("lqr_gains", "sweeps 0", sweeps=0)
    add("lqr_gains", "nothing asked for", want_gains=False, want_P=False, want_weights=False)
    add("lqr_gains", "weights without actions", actions=None)
    add("lqr_gains", "weights without obs", obs=None)

    def scalars(method):
        for label, bad in (("a string", "x"), ("None", None), ("not finite", NAN), ("infinite", INF), ("negative", -1.0)):
            add(method, f"mu {label}", mu=bad)
        for label, bad in (("a string", "xy"), ("a number", 1.0), ("none of them", ()), ("17 of them", (1.0,) * 17), ("not finite", (1.0, NAN)),
                           ("a tensor that is not finite", torch.tensor([1.0, INF]))):
            add(method, f"alphas {label}", alphas=bad)
        add(method, "weights without actions", actions=None)
        add(method, "weights without obs", obs=None)
        add(method, "weights without alphas", alphas=None)
        z = lambda *shape: torch.zeros(*shape, dtype=dt)
        add(method, "mu_dev and mu", mu_dev=z(M))
        for label, bad in (("one too long", z(M + 1)), ("of another dtype", _other(z(M))), ("not contiguous", z(2 * M)[::2]), ("a list", [0.0] * M),
                           ("of two axes", z(M, 1))):
            add(method, f"mu_dev {label}", mu=0.0, mu_dev=bad)
    riccati("ilqr_backward_into", True)
    scalars("ilqr_backward_into")
    add("ilqr_backward_into", "nothing asked for", gains_out=None, ff_out=None, P_out=None, p_out=None, dv_out=None, weights_out=None)
    riccati("ilqr_backward", False)
    scalars("ilqr_backward")
    add("ilqr_backward", "nothing asked for", want_gains=False, want_ff=False, want_P=False, want_p=False, want_dv=False, want_weights=False)

    def search_geometry(method):
        z = lambda *shape: torch.zeros(*shape, dtype=dt)
        tensors(method)
        cost(method, ("Q", "R", "Q_final"), every=method == "ilqr_line_search_into")
        add(method, "target None", target=None)
        add(method, "target of one axis", target=z(D))
        add(method, "knot_obs an array", knot_obs=z(K, N, D).numpy())
        add(method, "knot_obs of two axes", knot_obs=z(N, D))
        add(method, "target of 3 trajectories", target=z(3, D))
        add(method, "target of no trajectory", target=z(0, D))
        add(method, "target of more trajectories than lanes", target=z(2 * N, D))
        add(method, "knot_obs of no knot", knot_obs=z(0, N, D))
        # 17 candidates per trajectory, and more lanes than an int32 index addresses (tensors without storage)
        steered = {"ilqr_steer_into": dict(alphas=(1.0,) * 17, dv=z(K, 2, 1)), "ilqr_steer": dict(alphas=(1.0,) * 17, dv=z(K, 1, 2))}
        add(method, "17 candidates", knot_obs=z(K, 17, D), end_obs=z(17, D), actions=z(K, 17, 2), target=z(1, D), **steered.get(method, {}))
        if method.endswith("_into"):
            add(method, "lanes beyond int32", knot_obs=torch.empty(2 ** 20, 4096, D, dtype=dt, device="meta"),
                target=torch.empty(256, D, dtype=dt, device="meta"))
        add(method, "end_obs None", end_obs=None)
        add(method, "actions None", actions=None)
    search_geometry("ilqr_line_search_into")
    add("ilqr_line_search_into", "cost None", cost=None)
    add("ilqr_line_search_into", "choice None", choice=None)
    search_geometry("ilqr_line_search")
    without = lambda method, key: {k: v for k, v in _valid(dt, method)["nominal"].items() if k != key}
    for label, bad in (("empty", {}), ("a list", [1, 2]), ("without lx", without("ilqr_line_search", "lx"))):
        add("ilqr_line_search", f"nominal {label}", nominal=bad)

    def steering(method):
        search_geometry(method)
        for label, bad in (("a string", "xy"), ("None", None), ("a number", 1.0), ("none of them", ()), ("one of them", (1.0,)),
                           ("three of them", (1.0, 0.5, 0.25)), ("not finite", (1.0, NAN))):
            add(method, f"alphas {label}", alphas=bad)
        for label, bad in (("unknown member", dict(rule=dict(unknown=1.0))), ("unknown keyword", dict(always=True)),
                           ("member a string", dict(rule=dict(armijo="x"))), ("keyword not finite", dict(tol=NAN)),
                           ("grow below 1", dict(rule=dict(grow=0.5))), ("armijo negative", dict(armijo=-1.0)), ("shrink above 1", dict(shrink=2.0)),
                           ("mu_max below mu_start", dict(mu_max=0.01))):
            add(method, f"rule {label}", **bad)
        add(method, "dv None", dv=None)
    steering("ilqr_steer_into")
    for name in ("cost", "mu", "status", "choice"):
        add("ilqr_steer_into", f"{name} None", **{name: None})
    steering("ilqr_steer")
    for label, bad in (("None", None), ("empty", {}), ("a list", [1, 2]), ("without cost", without("ilqr_steer", "cost"))):
        add("ilqr_steer", f"nominal {label}", nominal=bad)
    add("ilqr_steer", "dv in the kernel's layout", dv=torch.zeros(K, 2, M, dtype=dt))
    add("ilqr_steer", "mu of another dtype", nominal__mu=_other(torch.zeros(M, dtype=dt)))
    add("ilqr_steer", "status of another dtype", nominal__status=torch.zeros(M, dtype=dt))
    add("ilqr_steer", "iters one too long", nominal__iters=torch.zeros(M + 1, dtype=torch.int32))

    def count_of(method, name):
        for label, bad in (("a bool", True), ("0", 0), ("a float", 2.0), ("None", None), ("no divisor of the lanes", 3),
                           ("more than the lanes", 2 * N)):
            add(method, f"{name} {label}", **{name: bad})

    def number(method, name, bad_values):
        for label, bad in (("a string", "x"), ("None", None), ("not finite", NAN), ("infinite", INF), ("negative", -1.0)) + bad_values:
            add(method, f"{name} {label}", **{name: bad})

    for method in ("mppi_update_into", "mppi_update"):
        z = lambda *shape: torch.zeros(*shape, dtype=dt)
        tensors(method)
        count_of(method, "samples")
        number(method, "temperature", (("0", 0.0), ("too small to invert", 1e-320), ("a bool", False)))
        add(method, "tail unknown", tail="wrap")
        add(method, "actions None", actions=None)
        add(method, "actions of two axes", actions=z(N, 2))
        add(method, "actions of no knot", actions=z(0, N, 2))
        for label, bad in (("a bool", True), ("negative", -1), ("beyond the knots", K + 1), ("a float", 1.0), ("None", None)):
            add(method, f"shift {label}", shift=bad)
        add(method, "returns None", returns=None)
    same = torch.zeros(K, M, 2, dtype=dt)
    add("mppi_update_into", "nominal_in None", nominal_in=None)
    add("mppi_update_into", "nominal_out None", nominal_out=None)
    add("mppi_update_into", "nominal_out is nominal_in", nominal_in=same, nominal_out=same)
    add("mppi_update", "nominal None", nominal=None)
    add("mppi_update", "table in the kernel's layout", table=torch.zeros(K, 2, R1, N, dtype=dt))
    add("mppi_update", "table no view of the kernel's layout", table=torch.zeros(N, K, 2, R1, dtype=dt))
    add("mppi_update", "table a string", table="x")

    for method in ("pf_update_into", "pf_update"):
        z = lambda *shape: torch.zeros(*shape, dtype=dt)
        tensors(method)
        count_of(method, "particles")
        number(method, "resample_ratio", (("a bool", True),))
        add(method, "obs None", obs=None)
        add(method, "obs of one axis", obs=z(N))
        add(method, "meas None", meas=None)
        add(method, "prec None", prec=None)
    same = torch.zeros(S, M, dtype=dt)
    add("pf_update_into", "logw_out None", logw_out=None)
    add("pf_update_into", "index None", index=None)
    add("pf_update_into", "logw_out is logw_in", logw_in=same, logw_out=same)
    return out


def _outcome(s, rec, reached, method, kw):
    """[exception type, message] of one call; a call that came through names the library it reached."""
    del rec.calls[:], reached[:]
    try:
        getattr(s, method)(**kw)
    except Exception as e:                        # every kind: the recording names the type
        assert not rec.calls and not reached, f"{method} raised {e!r} after it reached a library"
        return [type(e).__name__, str(e)]
    return ["no exception", f"reached {[name for name, _ in rec.calls]}"]


def _outcomes(dt, monkeypatch):
    rec = Recorder()
    s, reached = _sim(dt, monkeypatch, rec)
    return {name: _outcome(s, rec, reached, method, kw) for name, (method, kw) in _cases(dt).items()}


def _recorded(entry, dt):
    """A recording holds one [type, message] where both dtypes gave the same, else one per dtype."""
    return entry[str(dt)] if isinstance(entry, dict) else entry


@pytest.mark.parametrize("dt", DTYPES, ids=str)
def test_one_invalid_argument_raises_what_it_always_raised(dt, monkeypatch):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert list(golden)[0] == RECORDED_ON
    got = _outcomes(dt, monkeypatch)
    assert set(got) == set(golden) - {RECORDED_ON} and len(got) == 502
    wrong = {name: (out, _recorded(golden[name], dt)) for name, out in got.items() if out != _recorded(golden[name], dt)}
    assert not wrong, "\n".join(f"{name}:\n  got      {a}\n  recorded {b}" for name, (a, b) in wrong.items())
    assert not any(out[0] == "no exception" for out in got.values())


if __name__ == "__main__":                        # record: `PYTHONPATH=. python tests/test_controller_calls_host.py`, on a clean commit
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    commit = subprocess.check_output(["git", "-C", root, "rev-parse", "--short", "HEAD"], text=True).strip()
    with pytest.MonkeyPatch.context() as mp:
        a, b = (_outcomes(dt, mp) for dt in DTYPES)
    recording = {RECORDED_ON: f"commit {commit}, gym-os2r_amd/sim.py"}
    recording.update({name: a[name] if a[name] == b[name] else {str(DTYPES[0]): a[name], str(DTYPES[1]): b[name]} for name in a})
    with open(GOLDEN, "w") as f:
        json.dump(recording, f, indent=0, sort_keys=False)
        f.write("\n")
    print(f"{len(a)} cases recorded on {commit}")
