"""The contract of include/os2r_sysid.h restated in numpy, operation by operation in the dtype given: os2ri_perturb and the three
steps of os2ri_update (the sums of a segment, the 64 partials and the adjacent-pair tree over the segments of a set, and the
verdict, the damping and the damped Gauss-Newton step of a set).  tests/test_sysid_host.py holds it against an independent
statement (np.einsum, np.linalg.solve) and runs the whole identification loop with it on the CPU oracle; tests/test_gpu_sysid.py
holds the device against it bit for bit.  Not a test module."""
import numpy as np

CHUNKS = 64
STATE = ("theta_best", "cost_best", "hess", "grad", "lam", "status", "iters")
CONSTANT_NAMES = ("shrink", "grow", "lam_min", "lam_max", "diag_floor", "tol", "cost_floor")


def nsums(P):
    return P * (P + 1) // 2 + P + 1


def _positive(x):
    """Finite and > 0."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & (x > 0)


def points(theta, h, lo, hi, dtype):
    """plus = min(theta + h, hi), minus = max(theta - h, lo) with the selects of the contract; theta [..., P]."""
    theta, h, lo, hi = (np.asarray(a, dtype) for a in (theta, h, lo, hi))
    with np.errstate(all="ignore"):
        v = theta + h
        plus = np.where(v > hi, hi, v).astype(dtype)
        v = theta - h
        minus = np.where(v < lo, lo, v).astype(dtype)
    return plus, minus


def fresh_state(theta0, lam0, dtype):
    theta0 = np.asarray(theta0, dtype)
    T, P = theta0.shape
    return dict(theta_best=theta0.copy(), cost_best=np.full(T, np.inf, dtype), hess=np.zeros((T, P, P), dtype), grad=np.zeros((T, P), dtype),
                lam=np.full(T, lam0, dtype), status=np.zeros(T, np.int32), iters=np.zeros(T, np.int32))


def restate_perturb(theta, base, rows, h, lo, hi, dtype):
    """theta [T, P], base [F, M], rows [P] (row of parameter p in the packed array) -> params [F, (2 P + 1) M]."""
    theta, base = np.asarray(theta, dtype), np.asarray(base, dtype)
    T, P = theta.shape
    F, M = base.shape
    plus, minus = points(theta, h, lo, hi, dtype)
    out = np.tile(base, (1, 2 * P + 1)).reshape(F, 2 * P + 1, M)
    t = np.arange(M) % T
    for p, r in enumerate(rows):
        out[r] = theta[t, p][None, :]
        out[r, 1 + p] = plus[t, p]
        out[r, 1 + P + p] = minus[t, p]
    return np.ascontiguousarray(out.reshape(F, (2 * P + 1) * M))


def restate_segments(obs, meas, done, prec, P, dtype):
    """Steps 1 and 2: -> (sums [E, M], valid int32 [M])."""
    obs, meas, prec = np.asarray(obs, dtype), np.asarray(meas, dtype), np.asarray(prec, dtype)
    K, N, D = obs.shape
    M = meas.shape[1]
    assert N == (2 * P + 1) * M
    lanes = obs.reshape(K, 2 * P + 1, M, D)
    sums = np.zeros((nsums(P), M), dtype)
    kept = _positive(prec)
    with np.errstate(all="ignore"):
        for k in range(K):
            for d in range(D):
                if not kept[d]:
                    continue
                use = np.isfinite(meas[k, :, d])
                w = prec[d]
                r = (lanes[k, 0, :, d] - meas[k, :, d]).astype(dtype)
                diff = (lanes[k, 1:1 + P, :, d] - lanes[k, 1 + P:, :, d]).astype(dtype)       # [P, M]
                wr = (w * r).astype(dtype)
                wd = (w * diff).astype(dtype)

                def add(e, term):
                    sums[e] = np.where(use, (sums[e] + term.astype(dtype)).astype(dtype), sums[e])
                add(0, wr * r)
                for p in range(P):
                    add(1 + p, wd[p] * r)
                    for q in range(p + 1):
                        add(1 + P + p * (p + 1) // 2 + q, wd[p] * diff[q])
    valid = np.isfinite(sums).all(0)
    if done is not None:
        valid &= ~(np.asarray(done).reshape(K, 2 * P + 1, M) != 0).any((0, 1))
    return sums, valid.astype(np.int32)


def tree_total(terms, valid, dtype):
    """Step 3 for one set: terms [Q] of its segments in order, valid [Q] -> the total."""
    terms = np.asarray(terms)
    Q = terms.shape[0]
    rounds = (Q + CHUNKS - 1) // CHUNKS
    pad = np.zeros(rounds * CHUNKS, terms.dtype)
    pad[:Q] = terms
    ok = np.zeros(rounds * CHUNKS, bool)
    ok[:Q] = np.asarray(valid) != 0
    part = np.zeros(CHUNKS, dtype)
    with np.errstate(all="ignore"):
        for r in range(rounds):
            sl = slice(r * CHUNKS, (r + 1) * CHUNKS)
            part = np.where(ok[sl], (part + pad[sl]).astype(dtype), part)
        while part.shape[0] > 1:
            part = (part[0::2] + part[1::2]).astype(dtype)
    return part[0]


def restate_totals(sums, valid, T, dtype):
    """-> (totals [E, T], count int32 [T])."""
    E, M = sums.shape
    tot = np.zeros((E, T), dtype)
    for t in range(T):
        for e in range(E):
            tot[e, t] = tree_total(sums[e, t::T], valid[t::T], dtype)
    return tot, np.array([int(valid[t::T].sum()) for t in range(T)], np.int32)


def _constants(consts, dtype):
    get = (lambda n: consts[n]) if isinstance(consts, dict) else (lambda n: getattr(consts, n))
    return {n: dtype(get(n)) for n in CONSTANT_NAMES}


def _bits(x):
    return np.asarray(x).view(np.uint64 if np.asarray(x).dtype == np.float64 else np.uint32)


def solve_damped(hess, grad, lam, diag_floor, dtype):
    """Step 6 for one set: -> (delta [P], failed)."""
    P = grad.shape[0]
    A = np.array(hess, dtype)
    zero = np.zeros(P, dtype)
    with np.errstate(all="ignore"):
        for p in range(P):
            hpp = A[p, p]
            big = diag_floor if hpp < diag_floor else hpp
            A[p, p] = dtype(hpp + dtype(lam * big))
        L = np.zeros((P, P), dtype)
        for j in range(P):
            acc = A[j, j]
            for k in range(j):
                acc = dtype(acc - dtype(L[j, k] * L[j, k]))
            if not (np.isfinite(acc) and acc > 0):
                return zero, j + 1
            L[j, j] = np.sqrt(acc)
            for i in range(j + 1, P):
                acc = A[i, j]
                for k in range(j):
                    acc = dtype(acc - dtype(L[i, k] * L[j, k]))
                L[i, j] = dtype(acc / L[j, j])
        y = np.zeros(P, dtype)
        for i in range(P):
            acc = dtype(-grad[i])
            for k in range(i):
                acc = dtype(acc - dtype(L[i, k] * y[k]))
            y[i] = dtype(acc / L[i, i])
        x = np.zeros(P, dtype)
        for i in range(P - 1, -1, -1):
            acc = y[i]
            for k in range(P - 1, i, -1):
                acc = dtype(acc - dtype(L[k, i] * x[k]))
            x[i] = dtype(acc / L[i, i])
    return x, 0


def restate_sets(tot, count, theta, h, lo, hi, state, consts, dtype):
    """Steps 4 to 7 -> dict of the state after, theta_next, cost, valid, accepted, failed, delta."""
    theta = np.asarray(theta, dtype)
    T, P = theta.shape
    k = _constants(consts, dtype)
    h, lo, hi = (np.asarray(a, dtype) for a in (h, lo, hi))
    out = {n: np.array(state[n]) for n in STATE}
    out.update(theta_next=np.zeros((T, P), dtype), cost=np.zeros(T, dtype), valid=np.array(count, np.int32), accepted=np.zeros(T, np.uint8),
               failed=np.zeros(T, np.int32), delta=np.zeros((T, P), dtype))
    plus, minus = points(theta, h, lo, hi, dtype)
    with np.errstate(all="ignore"):
        Delta = (plus - minus).astype(dtype)
        for t in range(T):
            old, lam = state["cost_best"][t], state["lam"][t]
            if state["status"][t] != 0 or count[t] == 0:
                out["theta_next"][t] = state["theta_best"][t] if state["status"][t] != 0 else theta[t]
                out["cost"][t] = old
                continue
            J = dtype(tot[0, t] / dtype(2))
            accept = bool(_bits(J) < _bits(old))
            if accept:
                held = Delta[t] == 0
                H, g = np.zeros((P, P), dtype), np.zeros(P, dtype)
                for p in range(P):
                    g[p] = dtype(0) if held[p] else dtype(tot[1 + p, t] / Delta[t, p])
                    for q in range(p + 1):
                        if held[p] or held[q]:
                            v = dtype(1 if p == q else 0)
                        else:
                            v = dtype(tot[1 + P + p * (p + 1) // 2 + q, t] / dtype(Delta[t, p] * Delta[t, q]))
                        H[p, q] = H[q, p] = v
                out["theta_best"][t], out["cost_best"][t], out["hess"][t], out["grad"][t] = theta[t], J, H, g
                nl = dtype(lam * k["shrink"])
                nl = k["lam_min"] if nl < k["lam_min"] else nl
                status = 1 if (J <= k["cost_floor"] or (np.isfinite(old) and dtype(old - J) <= dtype(k["tol"] * old))) else 0
            else:
                nl = dtype(lam * k["grow"])
                status = 2 if nl > k["lam_max"] else 0
            out["lam"][t], out["status"][t], out["iters"][t] = nl, status, state["iters"][t] + 1
            out["cost"][t], out["accepted"][t] = J, 1 if accept else 0
            delta, failed = solve_damped(out["hess"][t], out["grad"][t], nl, k["diag_floor"], dtype)
            nxt = (out["theta_best"][t] + delta).astype(dtype)
            nxt = np.where(nxt < lo, lo, nxt)
            nxt = np.where(nxt > hi, hi, nxt)
            out["theta_next"][t], out["delta"][t], out["failed"][t] = nxt, delta, failed
    return out


def restate_update(obs, meas, done, prec, theta, h, lo, hi, state, consts, dtype):
    """os2ri_update as a whole; the dict also holds `sums`, `seg_valid` and `totals`."""
    theta = np.asarray(theta, dtype)
    T, P = theta.shape
    sums, seg_valid = restate_segments(obs, meas, done, prec, P, dtype)
    tot, count = restate_totals(sums, seg_valid, T, dtype)
    out = restate_sets(tot, count, theta, h, lo, hi, state, consts, dtype)
    out.update(sums=sums, seg_valid=seg_valid, totals=tot)
    return out


def plain_step(obs, meas, prec, theta, h, lo, hi, lam, diag_floor):
    """An independent statement of one damped Gauss-Newton step of one set in float64: the Jacobian by central differences,
    J'WJ and J'Wr by np.einsum, the step by np.linalg.solve.  Every segment valid, every reading there, every slot kept.
    -> (cost, H, g, delta)."""
    obs, meas = np.asarray(obs, np.float64), np.asarray(meas, np.float64)
    K, N, D = obs.shape
    M = meas.shape[1]
    P = (N // M - 1) // 2
    lanes = obs.reshape(K, 2 * P + 1, M, D)
    theta, h, lo, hi = (np.asarray(a, np.float64) for a in (theta, h, lo, hi))
    Delta = np.minimum(theta + h, hi) - np.maximum(theta - h, lo)               # (its own statement of the two points)
    r = lanes[:, 0] - meas                                                   # [K, M, D]
    jac = (lanes[:, 1:1 + P] - lanes[:, 1 + P:]) / Delta[:, None, None]       # [K, P, M, D]
    w = np.asarray(prec, np.float64)
    H = np.einsum("kpmd,d,kqmd->pq", jac, w, jac)
    g = np.einsum("kpmd,d,kmd->p", jac, w, r)
    cost = 0.5 * np.einsum("kmd,d,kmd->", r, w, r)
    A = H + lam * np.diag(np.maximum(np.diag(H), diag_floor))
    return cost, H, g, np.linalg.solve(A, -g)


# ---------------------------------------------------------------------------------------
# the two identification problems of the whole-loop tests, and the loop itself
# ---------------------------------------------------------------------------------------
LOOP_SEED, LOOP_LAM0, LOOP_ITERS, LOOP_BOUND = 0, 1e-3, 6, 1e-4
CASES = {
    # name: mode, contact, M, K, parameters (field name, dof name or None), truth, start, h, lo, hi
    "A": dict(mode="fixed_hip", contact=False, M=8, K=5, params=(("damping", "hip_joint"), ("damping", "knee_joint"), ("gravity", None)),
              truth=(0.02, 0.005, -9.6), start=(0.0, 0.0, -9.80665), h=(1e-3, 1e-3, 1e-2), lo=(0.0, 0.0, -11.0), hi=(0.1, 0.1, -9.0)),
    "B": dict(mode="free_hip", contact=True, M=16, K=10, params=(("mu", "knee_joint"), ("friction", "knee_joint"), ("mass_scale", "knee_joint")),
              truth=(0.6, 0.003, 1.1), start=(1.0, 0.001, 1.0), h=(1e-2, 1e-4, 1e-2), lo=(0.1, 0.0, 0.5), hi=(2.0, 0.05, 1.5)),
}
FIELD_OF = {"mass_scale": 0, "damping": 1, "friction": 2, "mu": 3, "gravity": 4}


def loop_case(name, oracle_py, seed=LOOP_SEED):
    """Case `name` -> dict: the config maker, sel, rows, the start states q0, qd0 [nq, M], the actions [K, M, 2], base [F, M] (the
    nominal parameters of the segments), the measured observations meas [K, M, D] logged by an oracle that holds the truth, and
    the steps and bounds.  Everything random comes from np.random.default_rng(seed), drawn in the order q, qd, actions."""
    from helpers import lying_states, make_config
    c = dict(CASES[name])
    M, K = c["M"], c["K"]

    def config(num_envs, dtype=None):
        kw = {} if dtype is None else dict(dtype=dtype)
        return make_config(c["mode"], "BalancingV1", False, num_envs=num_envs, contact=c["contact"], seed=3, auto_reset=False, **kw)
    cfg, _, model = config(M)
    nq, names = model["nq"], model["dof_names"]
    sel = [(FIELD_OF[f], 0 if dof is None else names.index(dof)) for f, dof in c["params"]]
    rows = [f * nq + i for f, i in sel]
    rng = np.random.default_rng(seed)
    real = oracle_py.OracleSim(cfg)
    real.reset()
    if c["contact"]:
        q0, qd0 = lying_states(model, M, rng)
    else:
        q0, qd0 = real.get_state()
        q0 = q0 + rng.normal(0, 0.1, (nq, M))
        qd0 = qd0 + rng.normal(0, 1.0, (nq, M))
    actions = rng.uniform(-1, 1, (K, M, 2))
    base = np.concatenate([real.get_params(f) for f in range(5)], 0)
    truth = base.copy()
    for r, v in zip(rows, c["truth"]):
        truth[r] = v
    for f in range(5):
        real.set_params(f, truth[f * nq:f * nq + (1 if f == 4 else nq)])
    real.set_state(q0, qd0)
    meas = np.stack([real.step(actions[k])[0] for k in range(K)])
    real.close()
    c.update(config=config, nq=nq, sel=sel, rows=rows, q0=q0, qd0=qd0, actions=actions, base=base, meas=meas, D=meas.shape[2])
    return c


def oracle_rollout(sim, nq, params, q0, qd0, actions):
    """set_params x 5 -> set_state -> K steps of an OracleSim of N lanes: -> (obs [K, N, D], done uint8 [K, N])."""
    for f in range(5):
        sim.set_params(f, params[f * nq:f * nq + (1 if f == 4 else nq)])
    sim.set_state(q0, qd0)
    outs = [sim.step(a) for a in actions]
    return np.stack([o[0] for o in outs]), np.stack([o[2] for o in outs])


def run_loop(c, rollout, update, iters=LOOP_ITERS, lam0=LOOP_LAM0):
    """The identification loop of case c: rollout(params [F, N]) -> (obs, done); update(obs, done, theta, state) -> the dict of
    restate_update.  -> the list of those dicts, one per iteration."""
    P = len(c["sel"])
    theta = np.array([c["start"]], np.float64)
    state = fresh_state(theta, lam0, np.float64)
    history = []
    for _ in range(iters):
        params = restate_perturb(theta, c["base"], c["rows"], c["h"], c["lo"], c["hi"], np.float64)
        obs, done = rollout(params)
        out = update(obs, done, theta, state)
        history.append(out)
        state = {n: out[n] for n in STATE}
        theta = out["theta_next"]
    return history


# ---------------------------------------------------------------------------------------
# crafted single calls
# ---------------------------------------------------------------------------------------
DEFAULTS = dict(shrink=0.5, grow=10.0, lam_min=1e-9, lam_max=1e6, diag_floor=1e-12, tol=0.0, cost_floor=0.0)
ROLES = ("fresh", "reject", "lam_max", "tol", "cost_floor", "no_valid", "done_minus", "nan_reading", "frozen", "nan_plus", "nan_nominal")


def random_problem(T, Q, K, P, D, dtype, seed=0):
    """A random call of T sets with Q segments each: obs [K, N, D], meas [K, M, D], done (all 0), prec, theta, a fresh state,
    infinite bounds.  The lanes follow a random linear model, so the system is positive definite where K D Q >= P."""
    rng = np.random.default_rng([seed, T, Q, K, P, D])
    M = T * Q
    meas = rng.normal(0, 1, (K, M, D))
    nominal = meas + rng.normal(0, 0.1, (K, M, D))
    slope = rng.normal(0, 1, (P, K, M, D))
    h = 0.01 * (1.0 + np.arange(P) / 4.0)
    lanes = np.concatenate([nominal[None], nominal[None] + slope * h[:, None, None, None] + rng.normal(0, 1e-4, (P, K, M, D)),
                            nominal[None] - slope * h[:, None, None, None]], 0)            # [S, K, M, D]
    obs = np.ascontiguousarray(lanes.transpose(1, 0, 2, 3).reshape(K, (2 * P + 1) * M, D)).astype(dtype)
    theta = rng.normal(0, 1, (T, P)).astype(dtype)
    c = dict(T=T, Q=Q, M=M, K=K, P=P, D=D, obs=obs, meas=meas.astype(dtype), done=np.zeros((K, (2 * P + 1) * M), np.uint8),
             prec=(0.5 + rng.uniform(0, 1, D)).astype(dtype), theta=theta, h=h, lo=np.full(P, -np.inf), hi=np.full(P, np.inf),
             state=fresh_state(theta + dtype(0.125), 1e-3, dtype), consts=dict(DEFAULTS))
    return c


def shaped_problem(T, Q, K, P, D, dtype):
    """random_problem with, where there are three sets, one that rejects (set 1: a best cost of 1e-30) and one with a segment
    lost to a done byte (set 2), and a NaN reading in the first segment."""
    c = random_problem(T, Q, K, P, D, dtype, seed=1)
    c["meas"][0, 0, D - 1] = np.nan
    if T >= 3:
        c["state"]["cost_best"][1] = 1e-30
        c["state"]["hess"][1] = np.eye(P, dtype=dtype) * dtype(3)
        c["state"]["grad"][1] = dtype(0.25)
        c["done"][K - 1, (1 + P) * c["M"] + 2] = 1                 # the first minus lane of segment 2, which is of set 2
    return c


def crafted_roles(dtype, K=3, P=3, D=5, Q=2):
    """One set per role of ROLES (set t plays ROLES[t]), Q = 2 segments each; parameter 1 sits half a step below its upper bound,
    so its quotient is one-sided; the slots 1 (prec 0) and 3 (prec +inf) are dropped.  -> the problem, c["J"] the cost of every set."""
    T = len(ROLES)
    c = random_problem(T, Q, K, P, D, dtype, seed=2)
    M, S = c["M"], 2 * P + 1
    role = {name: t for t, name in enumerate(ROLES)}
    lanes = c["obs"].reshape(K, S, M, D)
    c["prec"][1], c["prec"][3] = 0.0, np.inf
    c["theta"][:, 1] = dtype(0.75)
    c["hi"][1] = 0.75 + c["h"][1] / 2
    c["consts"].update(tol=1e-6, cost_floor=1e-12, lam_max=5.0)
    t = role["cost_floor"]                                       # both segments reproduce the log but for 1e-9
    for m in (t, t + T):
        lanes[:, 0, m] = c["meas"][:, m] + dtype(1e-9)
    for m in (role["no_valid"], role["no_valid"] + T):
        c["done"][0, (1 + P + 1) * M + m] = 1
    c["done"][K - 1, (1 + P) * M + role["done_minus"]] = 1        # one of the two segments is lost
    c["meas"][1, role["nan_reading"], 0] = np.nan
    c["meas"][1, role["nan_reading"] + T, 2] = np.inf
    lanes[0, 1 + 2, role["nan_plus"] + T, 4] = np.nan
    lanes[K - 1, 0, role["nan_nominal"], 0] = np.nan
    st = c["state"]
    st["lam"][role["lam_max"]] = 1.0
    for name in ("reject", "lam_max"):
        st["cost_best"][role[name]] = 1e-30
        st["hess"][role[name]] = np.eye(P, dtype=dtype) * dtype(2) + dtype(0.25)
        st["grad"][role[name]] = np.arange(1, P + 1, dtype=dtype) / dtype(8)
    f = role["frozen"]
    st["status"][f], st["iters"][f], st["cost_best"][f], st["lam"][f] = 2, 17, 0.3, 123.0
    st["hess"][f] = np.arange(P * P, dtype=dtype).reshape(P, P) / dtype(7)
    st["grad"][f] = -1.5
    first = restate_update(c["obs"], c["meas"], c["done"], c["prec"], c["theta"], c["h"], c["lo"], c["hi"], st, c["consts"], dtype)
    c["J"] = first["cost"].copy()
    st["cost_best"][role["tol"]] = c["J"][role["tol"]] * dtype(1 + 1e-7)
    c["role"] = role
    return c


def crafted_held(dtype):
    """Parameter 2 of three has lo = hi = theta: it is held in every set."""
    c = random_problem(2, 3, 2, 3, 4, dtype, seed=3)
    c["theta"][:, 2] = dtype(0.5)
    c["lo"][2] = c["hi"][2] = 0.5
    return c


def crafted_pivot(dtype):
    """lam = lam_min = 0 and a parameter the observations do not depend on (0: its plus and minus lanes are equal): the factor
    fails in column 0."""
    c = random_problem(1, 4, 2, 3, 4, dtype, seed=4)
    lanes = c["obs"].reshape(c["K"], 2 * c["P"] + 1, c["M"], c["D"])
    lanes[:, 1 + c["P"]] = lanes[:, 1]
    c["state"]["lam"][:] = 0
    c["consts"].update(lam_min=0.0)
    return c


def restate(c, dtype):
    return restate_update(c["obs"], c["meas"], c["done"], c["prec"], c["theta"], c["h"], c["lo"], c["hi"], c["state"], c["consts"], dtype)
