"""Shared by tests/test_setpoint_host.py and tests/test_gpu_setpoint.py: the yardstick of ``mjb_setpoint_ctrl``.  Not a test module.

The yardstick is never the kernel: ``restate`` is a plain numpy restatement of steps 1-7 of include/mjbatch.h (the same round-robin
schedule, the same skip rule, the same noise floor), run in ``np.longdouble`` (tol = its own epsilon) as the truth and in
``np.float64`` as the measure of what float64 arithmetic alone loses.  A bound is 8 x the float64 restatement's own figure for that
case, with a floor: the worst float64-restatement figure over the whole case list (five problems per case), measured on the CPU with
``python -m tests.setpoint_common`` and written below.

Error measures: ``ctrl``: max|u - u*| / max|u*| * rcond (the loss of a least-squares solve scales with 1 / rcond); ``sv``:
max|sv - sv*| / sv*_1; ``pinv``: max|P - P*| / max|P*| * rcond; ``residual``: |r - r*| / max_i (|qfrc_i| + sum_a |u*_a| |moment_ai|), the size of the terms it is summed
from; ``sweeps`` within 1 of the restatement's."""
from __future__ import annotations

import numpy as np

FACTOR = 8.0
# the worst float64-restatement figures over CASES x 5 problems (python -m tests.setpoint_common prints them)
FLOOR = {"ctrl": 1.10e-15, "sv": 3.84e-15, "pinv": 8.44e-16, "residual": 7.14e-16}
RCOND_MIN, MAX_SWEEPS = 1e-12, 30


def bound(f64_value, what):
    return max(FACTOR * f64_value, FLOOR[what])


def schedule(nu):
    """The rounds of one sweep: n' = nu rounded up to even, n' - 1 rounds; round rd: pair 0 = (n' - 1, rd), pair k = ((rd + k) mod
    (n' - 1), (rd - k) mod (n' - 1)); each as (min, max); a pair with an index >= nu is idle."""
    n2 = nu + (nu & 1)
    m = n2 - 1
    rounds = []
    for rd in range(m):
        pairs = []
        for k in range(n2 // 2):
            a, b = (m, rd) if k == 0 else ((rd + k) % m, (rd - k) % m)
            if max(a, b) < nu:
                pairs.append((min(a, b), max(a, b)))
        rounds.append(pairs)
    return rounds


def restate(moment, qfrc, dtype, rcond_min=RCOND_MIN, max_sweeps=MAX_SWEEPS):
    """ONE problem: moment [nu, nv], qfrc [nv].  Returns dict ctrl [nu], sv [min(nu, nv)], rcond, rank, residual, status, sweeps,
    pinv [nv, nu] - the NaN and +inf of a failed problem included."""
    moment, qfrc = np.asarray(moment), np.asarray(qfrc)
    nu, nv = moment.shape
    r = min(nu, nv)
    T = dtype
    nan = lambda *s: np.full(s, np.nan)
    if not (np.isfinite(moment).all() and np.isfinite(qfrc).all()):
        return {"ctrl": nan(nu), "sv": nan(r), "rcond": np.nan, "rank": 0, "residual": np.inf, "status": 1, "sweeps": 0, "pinv": nan(nv, nu)}
    with np.errstate(over="ignore"):
        if not np.isfinite((moment.astype(np.float64) ** 2).sum()):   # finite entries whose squares overflow in float64: no norm can be formed
            return {"ctrl": nan(nu), "sv": nan(r), "rcond": np.nan, "rank": 0, "residual": np.inf, "status": 1, "sweeps": 0, "pinv": nan(nv, nu)}
    tol = T(np.finfo(T).eps)
    G, V, q = moment.T.astype(T).copy(), np.eye(nu, dtype=T), qfrc.astype(T)
    floor = tol * tol * (G * G).sum()
    rounds = [(np.array([p[0] for p in pairs], dtype=int), np.array([p[1] for p in pairs], dtype=int)) for pairs in schedule(nu)]
    sweeps, converged = 0, False
    with np.errstate(all="ignore"):
        while sweeps < max_sweeps:
            rotated = False
            for I, J in rounds:
                if I.size == 0:
                    continue
                gi, gj = G[:, I], G[:, J]
                a, b, c = (gi * gi).sum(0), (gj * gj).sum(0), (gi * gj).sum(0)
                act = ~((c == 0) | (np.abs(c) <= tol * np.sqrt(a) * np.sqrt(b)) | (np.minimum(a, b) <= floor))
                if not act.any():
                    continue
                rotated = True
                I, J, a, b, c = I[act], J[act], a[act], b[act], c[act]
                z = (b - a) / (T(2) * c)
                t = np.where(z == 0, T(1), np.copysign(T(1), z) / (np.abs(z) + np.hypot(T(1), z)))
                cs = T(1) / np.sqrt(T(1) + t * t)
                sn = cs * t
                for M in (G, V):
                    x, y = M[:, I].copy(), M[:, J].copy()
                    M[:, I], M[:, J] = cs * x - sn * y, sn * x + cs * y
            sweeps += 1
            if not rotated:
                converged = True
                break
        s2 = (G * G).sum(0)
        sg = np.sqrt(s2)
        order = np.argsort(-sg, kind="stable")[:r]
        sv = sg[order]
        rcond = T(0) if sv[0] == 0 else sv[-1] / sv[0]
        rank = int((sv > T(rcond_min) * sv[0]).sum())
        status = 2 if not converged else 3 if not (rcond >= rcond_min) else 0
        out = {"sv": sv, "rcond": rcond, "rank": rank, "status": status, "sweeps": sweeps}
        if status:
            return {**out, "ctrl": nan(nu), "residual": np.inf, "pinv": nan(nv, nu)}
        keep = [j for j in order if sg[j] != 0]
        w = (G[:, keep] * q[:, None]).sum(0) / s2[keep]
        ctrl = (V[:, keep] * w[None, :]).sum(1) if keep else np.zeros(nu, dtype=T)
        residual = np.abs(ctrl @ moment.astype(T) - q).max()
        pinv = (G[:, keep] / s2[keep][None, :]) @ V[:, keep].T if keep else np.zeros((nv, nu), dtype=T)
    return {**out, "ctrl": ctrl, "residual": residual, "pinv": pinv}


# ---- the cases: name -> make(n) giving (moment [n, nu, nv], qfrc [n, nv]), the launch's keywords and the expected status --------------
def gaussian(nu, nv, n, seed=0):
    """Gaussian rows scaled by exp(2 N(0, 1)): actuators whose gears differ by orders of magnitude."""
    rng = np.random.default_rng(1000 * nu + nv + 7919 * seed)
    return rng.normal(size=(n, nu, nv)) * np.exp(2.0 * rng.normal(size=(n, nu, 1))), rng.normal(size=(n, nv))


def selection(n, couplings=0, seed=3):
    """21 x 27: actuator a drives dof 6 + a with its own gear (20 .. 120), the 6-dof root is unactuated; `couplings` tendon-like
    off-diagonal entries."""
    rng = np.random.default_rng(seed)
    m = np.zeros((n, 21, 27))
    gear = rng.uniform(20.0, 120.0, size=(n, 21))
    m[:, np.arange(21), 6 + np.arange(21)] = gear
    for a, d, f in ((2, 11, 0.5), (9, 20, -0.3), (15, 7, 0.25))[:couplings]:
        m[:, a, d] = f * gear[:, a]
    return m, rng.normal(size=(n, 27))


def graded(cond, n, seed=5):
    """12 x 20 with singular values 1 .. 1 / cond, logarithmically spaced."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 12, 20))
    for e in range(n):
        U, _ = np.linalg.qr(rng.normal(size=(12, 12)))
        W, _ = np.linalg.qr(rng.normal(size=(20, 12)))
        out[e] = (U * np.logspace(0.0, -np.log10(cond), 12)) @ W.T
    return out, rng.normal(size=(n, 20))


SHAPES = [(1, 1), (1, 2), (4, 6), (3, 7), (21, 27), (31, 33), (32, 64), (32, 32), (8, 5), (17, 16), (32, 3), (6, 1)]
CASES = [(f"gauss{nu}x{nv}", (lambda n, nu=nu, nv=nv: gaussian(nu, nv, n)), {}, 0) for nu, nv in SHAPES] + [
    ("selection21x27", lambda n: selection(n), {}, 0),
    ("coupled21x27", lambda n: selection(n, couplings=3), {}, 0),
    ("graded1e3", lambda n: graded(1e3, n), {}, 0),
    ("graded1e8", lambda n: graded(1e8, n), {}, 0),
    ("graded1e11", lambda n: graded(1e11, n), {}, 0),
]


def _between(bad_m, bad_q, good):
    """The failing problem between two good ones of its shape."""
    gm, gq = good
    return np.stack([gm[0], bad_m, gm[1]]), np.stack([gq[0], bad_q, gq[1]])


def _dup():
    m, q = gaussian(4, 6, 3, seed=1)
    m[2, 3] = m[2, 1]
    return _between(m[2], q[2], (m, q))


def _zero_row():
    m, q = gaussian(4, 6, 3, seed=2)
    m[2, 2] = 0.0
    return _between(m[2], q[2], (m, q))


def _all_zero():
    m, q = gaussian(4, 6, 3, seed=3)
    return _between(np.zeros((4, 6)), q[2], (m, q))


def _nan():
    m, q = gaussian(4, 6, 3, seed=4)
    m[2, 1, 3] = np.nan
    return _between(m[2], q[2], (m, q))


def _overflow():
    m, q = gaussian(4, 6, 3, seed=5)
    m[2, 1, 3] = 1e200                                             # finite, its square is not
    return _between(m[2], q[2], (m, q))


def _graded13():
    gm, gq = graded(1e3, 2, seed=6)
    bm, bq = graded(1e13, 1, seed=7)
    return _between(bm[0], bq[0], (gm, gq))


def _one_sweep():
    gm, gq = selection(2, seed=8)                                  # orthogonal rows: one clean sweep, status 0 at max_sweeps = 1
    bm, bq = selection(1, couplings=3, seed=9)
    return _between(bm[0], bq[0], (gm, gq))


# (name, make() -> (moment [3, nu, nv], qfrc [3, nv]) with the bad problem in the middle, keywords, status of the bad problem)
STATUS_CASES = [("graded1e13", _graded13, {}, 3), ("duplicated_row", _dup, {}, 3), ("zero_row", _zero_row, {}, 3), ("all_zero", _all_zero, {}, 3),
                ("nan_entry", _nan, {}, 1), ("overflowing_square", _overflow, {}, 1), ("max_sweeps_1", _one_sweep, {"max_sweeps": 1}, 2)]

_MADE, _REF = {}, {}


def problems(name, make, n):
    """``make(n)``, computed once per (name, n) and left unchanged: every test works on a copy."""
    if (name, n) not in _MADE:
        _MADE[(name, n)] = make(n)
    m, q = _MADE[(name, n)]
    return m.copy(), q.copy()


def references(key, moment, qfrc, **kw):
    """(float64 restatements, long-double restatements) of every problem, computed once per key and shared."""
    if key not in _REF:
        n = moment.shape[0]
        _REF[key] = ([restate(moment[e], qfrc[e], np.float64, **kw) for e in range(n)],
                     [restate(moment[e], qfrc[e], np.longdouble, **kw) for e in range(n)])
    return _REF[key]


def figures(x, tr, moment, qfrc):
    """The four error figures of one solved problem ``x`` against the truth ``tr`` (pinv: None when x has none), in long double."""
    L = lambda v: np.asarray(v, dtype=np.longdouble)
    rc = L(tr["rcond"])
    umax, pmax = np.abs(L(tr["ctrl"])).max(), np.abs(L(tr["pinv"])).max()
    qmax = (np.abs(L(qfrc)) + np.abs(L(tr["ctrl"])) @ np.abs(L(moment))).max()      # the size of the terms the residual is summed from
    out = {"ctrl": float(np.abs(L(x["ctrl"]) - L(tr["ctrl"])).max() / (umax if umax > 0 else 1) * rc),
           "sv": float(np.abs(L(x["sv"]) - L(tr["sv"])).max() / L(tr["sv"])[0]),
           "residual": float(abs(L(x["residual"]) - L(tr["residual"])) / (qmax if qmax > 0 else 1))}
    if x.get("pinv") is not None:
        out["pinv"] = float(np.abs(L(x["pinv"]) - L(tr["pinv"])).max() / (pmax if pmax > 0 else 1) * rc)
    return out


def judge(key, moment, qfrc, got, label, record=None, expect=0, **kw):
    """The comparison every test makes, per launch of problems that are all expected to be solved: ``got`` (ctrl, sv, rcond, rank,
    residual, status, sweeps [n, ...], pinv or None) against the long-double truth within ``bound`` of the float64 restatement's own
    figure, problem by problem; status and rank equal, sweeps within 1, rcond bitwise sv_r / sv_1 of the returned sv.
    ``record(key, value, bound)`` is told each figure (the largest share of its bound over the launch)."""
    f64, tr = references(key, moment, qfrc, **kw)
    n = moment.shape[0]
    assert [f["status"] for f in f64] == [expect] * n == [t["status"] for t in tr], (label, "the restatement itself must agree with the case")
    assert np.asarray(got["status"]).tolist() == [expect] * n, (label, got["status"])
    worst = {}
    for e in range(n):
        assert abs(int(got["sweeps"][e]) - f64[e]["sweeps"]) <= 1, (label, e, int(got["sweeps"][e]), f64[e]["sweeps"])
        assert int(got["rank"][e]) == tr[e]["rank"], (label, e, int(got["rank"][e]), tr[e]["rank"])
        sv = np.asarray(got["sv"][e])
        assert got["rcond"][e] == (sv[-1] / sv[0] if sv[0] != 0 else 0.0), (label, e, got["rcond"][e])
        assert (np.diff(sv) <= 0).all(), (label, e, "sv is not sorted")
        x = {k: (None if got.get(k) is None else got[k][e]) for k in ("ctrl", "sv", "residual", "pinv")}
        mine, np64 = figures(x, tr[e], moment[e], qfrc[e]), figures(f64[e], tr[e], moment[e], qfrc[e])
        for what, v in mine.items():
            b = bound(np64[what], what)
            if what not in worst or v / b > worst[what][0] / worst[what][2]:
                worst[what] = (v, np64[what], b)
    for what, (v, v64, b) in sorted(worst.items()):
        print(f"{label} {what}: kernel {v:.2e}  float64 numpy {v64:.2e}  bound {b:.2e}")
        if record:
            record(f"{label}/{what}", v, b)
        assert v <= b, (label, what, v, v64, b)
    return f64, tr


OUTPUTS = ("ctrl", "sv", "rcond", "rank", "residual", "status", "sweeps", "pinv")


def check_statuses(solve, label):
    """The status and isolation test of both suites: ``solve(moment, qfrc, **kw)`` -> outputs.  The failed problem (the middle one of
    three) has the status, NaN in ctrl and pinv, +inf in residual and what was reached in the rest (sweeps within 1 of the
    restatement's, sv within its bound where there are any); its neighbours are solved and are bitwise what a launch of those two
    alone returns."""
    for name, make, kw, status in STATUS_CASES:
        m, q = problems("status/" + name, lambda n: make(), 3)
        f64, tr = references("status/" + name, m, q, **kw)
        assert [f["status"] for f in f64] == [0, status, 0] == [t["status"] for t in tr], (label, name, [f["status"] for f in f64])
        got = solve(m, q, **kw)
        assert np.asarray(got["status"]).tolist() == [0, status, 0], (label, name, got["status"])
        assert np.isnan(got["ctrl"][1]).all() and np.isnan(got["pinv"][1]).all() and got["residual"][1] == np.inf, (label, name)
        assert abs(int(got["sweeps"][1]) - f64[1]["sweeps"]) <= 1, (label, name, got["sweeps"][1], f64[1]["sweeps"])
        if status == 1:
            assert np.isnan(got["sv"][1]).all() and np.isnan(got["rcond"][1]) and got["rank"][1] == 0 and got["sweeps"][1] == 0, (label, name)
        else:
            sv_t = np.asarray(tr[1]["sv"], dtype=np.longdouble)
            scale = sv_t[0] if sv_t[0] > 0 else 1.0
            err = lambda s: float(np.abs(np.asarray(s, dtype=np.longdouble) - sv_t).max() / scale)
            if status == 3:                                         # converged: the singular values are those of the restatement
                assert err(got["sv"][1]) <= bound(err(f64[1]["sv"]), "sv"), (label, name, err(got["sv"][1]), err(f64[1]["sv"]))
                assert got["rcond"][1] < RCOND_MIN and int(got["rank"][1]) == tr[1]["rank"] < min(m.shape[1:]), (label, name, got["rcond"][1], got["rank"][1])
            assert np.isfinite(got["sv"][1]).all() and np.isfinite(got["rcond"][1]), (label, name)
        if name == "all_zero":
            assert got["rcond"][1] == 0.0 and (got["sv"][1] == 0.0).all() and got["rank"][1] == 0, (label, name)
        if name == "zero_row":
            assert got["rcond"][1] == 0.0 and got["sv"][1][-1] == 0.0, (label, name)
        keep = [0, 2]
        alone = solve(m[keep], q[keep], **kw)
        for key in OUTPUTS:
            assert np.array_equal(np.asarray(got[key])[keep], np.asarray(alone[key])), (label, name, key)
        assert np.isfinite(np.asarray(got["ctrl"])[keep]).all() and np.isfinite(np.asarray(got["pinv"])[keep]).all(), (label, name)


if __name__ == "__main__":                                        # the floors: the worst float64-restatement figures over the case list
    worst = {}
    for name, make, kw, _ in CASES:
        m, q = problems(name, make, 5)
        f64, tr = references(name, m, q, **kw)
        for e in range(5):
            for what, v in figures(f64[e], tr[e], m[e], q[e]).items():
                worst[what] = max(worst.get(what, 0.0), v)
        print(name, "sweeps", [f["sweeps"] for f in f64], "status", [f["status"] for f in f64], "rcond", f"{float(tr[0]['rcond']):.2e}")
    print({k: f"{v:.2e}" for k, v in worst.items()})
