"""Shared by tests/test_dlyap_host.py and tests/test_gpu_dlyap.py: the yardstick of ``mjb_lqr_dlyap``.  Not a test module.

The yardstick is never the kernel: ``restate`` is a plain numpy restatement of the squared Smith iteration of include/mjbatch.h (same
symmetrisation, same stopping rule: the FIRST ``change <= tol``), run in ``np.longdouble`` with ``tol = 1e-17`` as the truth and in
``np.float64`` as the measure of what float64 arithmetic alone loses; ``lqr_common.bound`` turns the two into the tolerance (8 x the
float64 restatement's own error, floor 1e-13; floor 1e-11 against scipy).  ``residual`` is the relative residual of the Lyapunov
equation itself, in long double.

The systems are those of ``dare_common.CASES``, each with the gain of the float64 DARE restatement; all their closed loops have a
spectral radius between 0.96 and 0.998 and converge in 10-14 iterations.  On the humanoid fixture the closed loop keeps two modes of
modulus exactly 1 that S does not see: the long-double Lyapunov restatement at 1e-17 never stops there (change collapses to 5e-18 at
iteration 19, then doubles with every iteration), so its truth is the long-double DARE solution - policy evaluation of the optimal
gain is X."""
from __future__ import annotations

import numpy as np

from tests import dare_common as dc
from tests.lqr_common import FLOOR, FLOOR_DARE, bound, rel_err  # noqa: F401  (re-exported)

TOL, MAX_ITER = 1e-12, 64
TRUTH_TOL, TRUTH_MAX_ITER = 1e-17, 64
CASES = dc.CASES


def closed_loop(A, B, K, Q, R, dtype, feedback_sign=-1):
    """Steps 1 and 2: (M, S) in ``dtype``.  B, K None: M = A; R or K None: S = sym(Q).  Only the lower triangles of Q and R are read."""
    c = lambda x: None if x is None else np.asarray(x).astype(dtype)
    A, B, K, Q, R = (c(x) for x in (A, B, K, Q, R))
    half = dtype(0.5)
    low = lambda X: np.tril(X) + np.tril(X, -1).T
    M, V = A.copy(), low(Q)
    if K is not None:
        Ks = dtype(feedback_sign) * K
        M = A + B @ Ks
        if R is not None:
            V = V + Ks.T @ (low(R) @ Ks)
    return M, half * (V + V.T)


def restate(A, B, K, Q, R, dtype, tol=TOL, max_iter=MAX_ITER, feedback_sign=-1, transpose=False, x0=None):
    """ONE problem.  Returns dict P [nx, nx], J (None without x0), status, iters, change - the NaN and +inf of a failed problem included."""
    nx = np.asarray(A).shape[0]
    half = dtype(0.5)
    fail = lambda status, iters, change: {"P": np.full((nx, nx), np.nan), "J": None if x0 is None else np.inf, "status": status,
                                          "iters": iters, "change": float(change) if np.isfinite(change) else np.inf}
    with np.errstate(all="ignore"):
        M, P = closed_loop(A, B, K, Q, R, dtype, feedback_sign)
        if not (np.isfinite(M).all() and np.isfinite(P).all()):
            return fail(1, 0, np.inf)
        iters, change = 0, np.inf
        while True:
            T = M @ (P @ M.T) if transpose else M.T @ (P @ M)
            Pn = P + half * (T + T.T)
            M = M @ M
            iters += 1
            if not (np.isfinite(Pn).all() and np.isfinite(M).all()):
                return fail(2, iters, np.inf)
            num, den = np.abs(Pn - P).max(), np.abs(Pn).max()
            change = dtype(0) if num == 0 and den == 0 else num / den
            P = Pn
            if change <= tol:
                break
            if iters == max_iter:
                return fail(3, iters, change)
    J = None
    if x0 is not None:
        x = np.asarray(x0).astype(dtype)
        J = x @ (P @ x)
    return {"P": P, "J": J, "status": 0, "iters": iters, "change": float(change)}


def truth(A, B, K, Q, R, **kw):
    return restate(A, B, K, Q, R, np.longdouble, tol=TRUTH_TOL, max_iter=TRUTH_MAX_ITER, **kw)


def residual(A, B, K, Q, R, P, feedback_sign=-1, transpose=False):
    """max|M'PM + S - P| / max|P| (the Gramian form with ``transpose``) in long double."""
    M, S = closed_loop(A, B, K, Q, R, np.longdouble, feedback_sign)
    P = np.asarray(P, dtype=np.longdouble)
    res = (M @ P @ M.T if transpose else M.T @ P @ M) + S - P
    return float(np.abs(res).max() / np.abs(P).max())


def cost_of(P, x0):
    """x0' P x0 in long double."""
    P, x = np.asarray(P, dtype=np.longdouble), np.asarray(x0, dtype=np.longdouble)
    return x @ (P @ x)


# ---- the cases: those of dare_common with K [n, nu, nx] (the float64 DARE restatement's gain) and x0 [n, nx] added ---------------------
_GAINS = {}


def with_gain(case, seed=7):
    """A copy of a dare_common case dict with "K" and "x0" added."""
    out = {k: np.array(v) for k, v in case.items()}
    n = out["A"].shape[0]
    sols = [dc.restate(out["A"][e], out["B"][e], out["Q"][e], out["R"][e], np.float64) for e in range(n)]
    assert all(s["status"] == 0 for s in sols), "the DARE restatement must design the case"
    out["K"] = np.stack([s["K"] for s in sols])
    out["x0"] = np.random.default_rng(seed).normal(size=(n, out["A"].shape[1]))
    return out


def gain_case(name, make, n):
    """``with_gain(make(n))``, computed once per (name, n) and left unchanged: every test works on a copy."""
    if (name, n) not in _GAINS:
        _GAINS[(name, n)] = with_gain(make(n))
    return {k: v.copy() for k, v in _GAINS[(name, n)].items()}


def humanoid_case(scales=(1.0,)):
    """The humanoid balance design (tests/golden/dare_humanoid.npz) with the float64 DARE restatement's gain, one copy per entry of
    ``scales`` with Q scaled by it; "X" is the long-double DARE solution, the truth of P."""
    key = ("humanoid", tuple(scales))
    if key not in _GAINS:
        case = with_gain(dc.humanoid_case(scales))
        tr = [dc.truth(case["A"][e], case["B"][e], case["Q"][e], case["R"][e]) for e in range(len(scales))]
        assert all(t["status"] == 0 for t in tr)
        case["X"] = np.stack([t["X"] for t in tr])
        _GAINS[key] = case
    return {k: v.copy() for k, v in _GAINS[key].items()}


def _systems(case):
    n = case["A"].shape[0]
    opt = lambda k, e: None if case.get(k) is None else case[k][e]
    return [(case["A"][e], opt("B", e), opt("K", e), case["Q"][e], opt("R", e)) for e in range(n)]


def judge(case, got, label, record=None, truth_P=None, shared_gain=False, **kw):
    """The comparison every test makes, per launch: P of ``got`` (P, J [n, ...], status, iters) against the long-double truth within
    ``bound`` of the float64 restatement's error, the residual likewise, iters within 1, P bitwise symmetric, and J within ``bound`` of
    x0' P x0 of the returned P in long double (the measure: the same sum evaluated by numpy in float64).  ``kw``: feedback_sign,
    transpose.  ``record(key, value, bound)`` is told each figure.  Returns the float64 restatements.

    Every problem must be solved, unless ``shared_gain``: one system's gain on the other systems of a case need not stabilise them, so
    there the float64 restatement says which problems end with which status (problem 0, whose own gain it is, always with 0); a
    problem it fails must show that status, NaN, +inf and iters within 1, and the comparisons are made on the rest."""
    sys_ = _systems(case)
    n = len(sys_)
    f64 = [restate(*s, np.float64, **kw) for s in sys_]
    expect = [f["status"] for f in f64]
    assert expect[0] == 0 and (shared_gain or expect == [0] * n), f"the restatement itself must solve the case: {expect}"
    assert np.asarray(got["status"]).tolist() == expect, (label, got["status"], expect)
    ok = [e for e in range(n) if expect[e] == 0]
    it = np.asarray(got["iters"])
    for e in range(n):
        assert abs(int(it[e]) - f64[e]["iters"]) <= 1, (label, e, int(it[e]), f64[e]["iters"])
        if expect[e]:
            assert np.isnan(got["P"][e]).all() and (got.get("J") is None or got["J"][e] == np.inf), (label, e)
    if truth_P is None:
        tr = [truth(*sys_[e], **kw) for e in ok]
        assert all(t["status"] == 0 for t in tr), "the long-double restatement itself must solve the case"
        truth_P = np.stack([t["P"] for t in tr])
    else:
        truth_P = np.asarray(truth_P)[ok]
    P = np.asarray(got["P"])[ok]
    mine, np64 = rel_err(P, truth_P), rel_err(np.stack([f64[e]["P"] for e in ok]), truth_P)
    print(f"{label} P: kernel {mine:.2e}  float64 numpy {np64:.2e}  bound {bound(np64):.2e}")
    if record:
        record(f"{label}/P", mine, bound(np64))
    assert mine <= bound(np64), (label, "P", mine, np64)
    r_mine = max(residual(*sys_[e], P[i], **kw) for i, e in enumerate(ok))
    r_np64 = max(residual(*sys_[e], f64[e]["P"], **kw) for e in ok)
    print(f"{label} residual: kernel {r_mine:.2e}  float64 numpy {r_np64:.2e}  bound {bound(r_np64):.2e}")
    if record:
        record(f"{label}/residual", r_mine, bound(r_np64))
    assert r_mine <= bound(r_np64), (label, r_mine, r_np64)
    assert np.array_equal(P, P.transpose(0, 2, 1)), f"{label}: P is not bitwise symmetric"
    if case.get("x0") is not None and got.get("J") is not None:
        x0 = case["x0"][ok]
        ref = np.array([cost_of(P[i], x0[i]) for i in range(len(ok))])
        j64 = np.array([x0[i] @ (P[i] @ x0[i]) for i in range(len(ok))])
        rel = lambda j: float(np.abs((np.asarray(j, dtype=np.longdouble) - ref) / ref).max())
        j_mine, j_np64 = rel(np.asarray(got["J"])[ok]), rel(j64)
        print(f"{label} J: kernel {j_mine:.2e}  float64 numpy {j_np64:.2e}  bound {bound(j_np64):.2e}")
        if record:
            record(f"{label}/J", j_mine, bound(j_np64))
        assert j_mine <= bound(j_np64), (label, "J", j_mine, j_np64)
    return f64


# ---- the failures: reported through memory, written as NaN and +inf, isolated ----------------------------------------------------------
def _bad_cases():
    """(name, case, max_iter, status): problem 2 of 5 is bad (every problem with max_iter = 3)."""
    base = gain_case("gen7x3", lambda n: dc.generator_case(7, 3, n), 5)
    nan_a = {k: v.copy() for k, v in base.items()}
    nan_a["A"][2, 3, 1] = np.nan
    swapped = gain_case("gen12x4", lambda n: dc.generator_case(12, 4, n), 5)     # another system's gain: rho 2.2 - 2.6, overflow at iteration 9
    swapped["K"][2] = swapped["K"][3]

    def two(M, Q):                                                # 2 x 2 systems, problem 2 replaced by M with a zero gain
        case = gain_case("gen2x1", lambda n: dc.generator_case(2, 1, n), 5)
        case["A"][2], case["K"][2], case["Q"][2] = M, 0.0, Q
        return case
    unstable = two(np.diag([1.1, 0.5]), np.eye(2))               # overflow at iteration 12
    marginal = two(np.array([[1.0, 1.0], [0.0, 0.5]]), np.eye(2))   # P doubles for ever: change 0.5 at 64
    return [("nan_in_A", nan_a, MAX_ITER, 1), ("swapped_gain", swapped, MAX_ITER, 2), ("unstable_2x2", unstable, MAX_ITER, 2),
            ("max_iter_3", base, 3, 3), ("marginal_2x2", marginal, MAX_ITER, 3)]


def check_statuses(solve, label):
    """The status and isolation test of both suites: ``solve(case, max_iter)`` -> outputs (P, J, status, iters, change).  The failed
    problem has the status, NaN for P, +inf for J, iters within 1 of the restatement's and change as stated; the other four are bitwise
    what a launch of those four alone returns."""
    for name, case, max_iter, status in _bad_cases():
        got = solve(case, max_iter)
        bad = [0, 1, 2, 3, 4] if name == "max_iter_3" else [2]
        keep = [e for e in range(5) if e not in bad]
        assert np.asarray(got["status"]).tolist() == [status if e in bad else 0 for e in range(5)], (label, name, got["status"])
        for e in bad:
            assert np.isnan(got["P"][e]).all() and got["J"][e] == np.inf, (label, name, e)
            ref = restate(*_systems(case)[e], np.float64, max_iter=max_iter)
            assert ref["status"] == status and abs(int(got["iters"][e]) - ref["iters"]) <= 1, (label, name, got["iters"][e], ref["iters"])
            assert not np.isnan(got["change"][e]), (label, name)
            if status == 3:
                assert TOL < got["change"][e] < np.inf, (label, name, got["change"][e])
            else:
                assert got["change"][e] == np.inf, (label, name, got["change"][e])
        if name == "marginal_2x2":
            assert int(got["iters"][2]) == 64 and got["change"][2] == 0.5, (got["iters"][2], got["change"][2])
        if not keep:
            continue
        assert np.isfinite(got["P"][keep]).all() and np.isfinite(got["J"][keep]).all(), (label, name)
        alone = solve({k: v[keep] for k, v in case.items()}, max_iter)
        for key in ("P", "J", "change", "iters", "status"):
            assert np.array_equal(np.asarray(got[key])[keep], np.asarray(alone[key])), (label, name, key)
