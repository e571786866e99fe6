"""Shared by tests/test_dare_host.py and tests/test_gpu_dare.py: the yardstick of ``mjb_lqr_dare``.  Not a test module.

The yardstick is never the kernel: ``restate`` is a plain numpy restatement of the doubling algorithm of include/mjbatch.h (same pivot
rule, same stopping rule), run in ``np.longdouble`` with ``tol = 1e-17`` as the truth and in ``np.float64`` as the measure of what
float64 arithmetic alone loses; ``lqr_common.bound`` turns the two into the tolerance (8 x the float64 restatement's own error, with
the floor).  ``residual`` is the relative residual of the Riccati equation itself, in long double."""
from __future__ import annotations

import os

import numpy as np

from tests.lqr_common import EDGE_SIZES, FLOOR, FLOOR_DARE, _chol_solve, bound, generate, rel_err  # noqa: F401  (re-exported)

TOL, MAX_ITER = 1e-12, 32
TRUTH_TOL, TRUTH_MAX_ITER = 1e-17, 64
GENERATOR_SIZES = [(4, 1), (7, 3), (12, 4), (17, 5), (54, 21), (64, 32)]
MECHANICAL_SIZES = [(6, 2), (54, 21)]
HUMANOID = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dare_humanoid.npz")


def _lu(W):
    """In-place-style LU with partial pivoting, the pivot the LOWEST index among the rows of largest |.|: (LU, perm) or None at a
    pivot that is zero or not finite."""
    W = W.copy()
    n = W.shape[0]
    perm = np.arange(n)
    for j in range(n):
        col = np.abs(W[j:, j])
        best = col[0]
        p = j
        for i in range(1, n - j):
            if col[i] > best:
                best, p = col[i], j + i
        if not (best > 0) or not np.isfinite(best):
            return None
        if p != j:
            W[[j, p]] = W[[p, j]]
            perm[[j, p]] = perm[[p, j]]
        W[j + 1:, j] = W[j + 1:, j] / W[j, j]
        W[j + 1:, j + 1:] -= np.outer(W[j + 1:, j], W[j, j + 1:])
    return W, perm


def _lu_solve(lu, R):
    W, perm = lu
    n = W.shape[0]
    Y = R[perm].copy()
    for j in range(n):
        Y[j] = Y[j] - W[j, :j] @ Y[:j]
    for j in range(n - 1, -1, -1):
        Y[j] = (Y[j] - W[j, j + 1:] @ Y[j + 1:]) / W[j, j]
    return Y


def restate(A, B, Q, R, dtype, tol=TOL, max_iter=MAX_ITER):
    """ONE problem.  Returns dict X [nx, nx], K [nu, nx], status, iters, change - the zeros of a failed problem included."""
    A, B, Q, R = (np.asarray(x).astype(dtype) for x in (A, B, Q, R))
    nx, nu = A.shape[0], B.shape[1]
    half, eye = dtype(0.5), np.eye(nx, dtype=dtype)
    sym = lambda M: half * (M + M.T)
    fail = lambda status, iters, change: {"X": np.zeros((nx, nx), dtype=dtype), "K": np.zeros((nu, nx), dtype=dtype), "status": status,
                                          "iters": iters, "change": float(change) if np.isfinite(change) else np.inf}
    Z = _chol_solve(R, B.T.copy())
    if Z is None:
        return fail(1, 0, np.inf)
    G, H, Ak = sym(B @ Z), Q.copy(), A.copy()
    iters, change = 0, np.inf
    while True:
        lu = _lu(eye + G @ H)
        if lu is None:
            return fail(2, iters, change)
        with np.errstate(all="ignore"):                          # a system that is not stabilisable overflows: status 2 below
            XA, XG = _lu_solve(lu, Ak), _lu_solve(lu, G)
            Hn = sym(H + Ak.T @ (H @ XA))
            G = sym(G + Ak @ XG @ Ak.T)
            Ak = Ak @ XA
            change = np.abs(Hn - H).max() / np.abs(Hn).max()
        H = Hn
        iters += 1
        if not (np.isfinite(H).all() and np.isfinite(G).all() and np.isfinite(Ak).all()):
            return fail(2, iters, np.inf)
        if change <= tol:
            break
        if iters == max_iter:
            return fail(3, iters, change)
    Kt = _chol_solve(R + B.T @ H @ B, B.T @ H @ A)
    if Kt is None:
        return fail(1, iters, change)
    return {"X": H, "K": Kt, "status": 0, "iters": iters, "change": float(change)}


def truth(A, B, Q, R):
    return restate(A, B, Q, R, np.longdouble, tol=TRUTH_TOL, max_iter=TRUTH_MAX_ITER)


def residual(A, B, Q, R, X):
    """max|A'XA - X - A'XB (R + B'XB)^-1 B'XA + Q| / max|X| in long double."""
    A, B, Q, R, X = (np.asarray(x, dtype=np.longdouble) for x in (A, B, Q, R, X))
    BXA = B.T @ X @ A
    S = _chol_solve(R + B.T @ X @ B, BXA)
    if S is None:
        return np.inf
    res = A.T @ X @ A - X - BXA.T @ S + Q
    return float(np.abs(res).max() / np.abs(X).max())


# ---- the cases, all seeded: dicts of A [n, nx, nx], B [n, nx, nu], Q [n, nx, nx], R [n, nu, nu] --------------------------------------
def generator_case(nx, nu, n, seed=0):
    p = generate(nx, nu, 1, n, seed=seed, constant=True)
    return {"A": p["A"][0].copy(), "B": p["B"][0].copy(), "Q": p["Q"].copy(), "R": p["R"].copy()}


def mechanical_case(nx, nu, n, seed=0):
    """Unstable 'mechanical' systems x = (q, v), nq = nx / 2: q' = q + h v, v' = v + h (Kq q - D v) + h Bu u with an indefinite
    stiffness Kq (some modes fall over), and Q zero on the velocity block (singular)."""
    rng = np.random.default_rng(1000 + seed)
    nq, h = nx // 2, 0.01
    A, B, Q, R = [], [], [], []
    for _ in range(n):
        M = rng.normal(size=(nq, nq)) / np.sqrt(nq)
        Kq = 4.0 * (M + M.T) + np.diag(rng.uniform(-20.0, 20.0, size=nq))
        D = np.diag(rng.uniform(0.0, 0.5, size=nq))
        Ae = np.eye(nx)
        Ae[:nq, nq:] = h * np.eye(nq)
        Ae[nq:, :nq] = h * Kq
        Ae[nq:, nq:] -= h * D
        Be = np.zeros((nx, nu))
        Be[nq:] = h * rng.normal(size=(nq, nu)) * 5.0
        Qe = np.zeros((nx, nx))
        Qe[:nq, :nq] = np.diag(rng.uniform(1.0, 10.0, size=nq))
        W = rng.normal(size=(nu, nu))
        A.append(Ae); B.append(Be); Q.append(Qe); R.append(0.1 * np.eye(nu) + 0.01 * W @ W.T)
    return {k: np.stack(v) for k, v in (("A", A), ("B", B), ("Q", Q), ("R", R))}


def zero_column_case(n, seed=0):
    """(7, 3) generator systems whose A has column 2 zeroed (a state nothing depends on: A is singular)."""
    p = generator_case(7, 3, n, seed=seed + 50)
    p["A"][:, :, 2] = 0.0
    return p


def humanoid_case(scales=(1.0,)):
    """The tutorial's humanoid balance design (tests/golden/dare_humanoid.npz, made by tests/golden/make_dare_humanoid.py), one copy
    per entry of ``scales`` with Q scaled by it."""
    z = np.load(HUMANOID)
    n = len(scales)
    return {"A": np.stack([z["A"]] * n), "B": np.stack([z["B"]] * n), "Q": np.stack([s * z["Q"] for s in scales]), "R": np.stack([z["R"]] * n)}


CASES = [(f"gen{nx}x{nu}", lambda n, nx=nx, nu=nu: generator_case(nx, nu, n)) for nx, nu in GENERATOR_SIZES] + \
        [(f"mech{nx}x{nu}", lambda n, nx=nx, nu=nu: mechanical_case(nx, nu, n)) for nx, nu in MECHANICAL_SIZES] + \
        [("zerocol7x3", lambda n: zero_column_case(n))] + \
        [(f"gen{nx}x{nu}", lambda n, nx=nx, nu=nu: generator_case(nx, nu, n)) for nx, nu in EDGE_SIZES]     # the edges of the launch dispatch


def judge(case, got, label, record=None):
    """The comparison every test makes, per launch: the errors of ``got`` (X, K [n, ...], status, iters) against the long-double truth
    within ``bound`` of the float64 restatement's, the residual likewise, iters within 1.  ``record(key, value, bound)`` is told each figure."""
    n = case["A"].shape[0]
    sys_ = [(case["A"][e], case["B"][e], case["Q"][e], case["R"][e]) for e in range(n)]
    tr = [truth(*s) for s in sys_]
    f64 = [restate(*s, np.float64) for s in sys_]
    assert all(t["status"] == 0 for t in tr) and all(f["status"] == 0 for f in f64), "the restatement itself must solve the case"
    assert np.asarray(got["status"]).tolist() == [0] * n, got["status"]
    for key in ("X", "K"):
        ref = np.stack([t[key] for t in tr])
        mine, np64 = rel_err(got[key], ref), rel_err(np.stack([f[key] for f in f64]), ref)
        print(f"{label} {key}: kernel {mine:.2e}  float64 numpy {np64:.2e}  bound {bound(np64):.2e}")
        if record:
            record(f"{label}/{key}", mine, bound(np64))
        assert mine <= bound(np64), (label, key, mine, np64)
    r_mine = max(residual(*s, got["X"][e]) for e, s in enumerate(sys_))
    r_np64 = max(residual(*s, f["X"]) for s, f in zip(sys_, f64))
    print(f"{label} residual: kernel {r_mine:.2e}  float64 numpy {r_np64:.2e}  bound {bound(r_np64):.2e}")
    if record:
        record(f"{label}/residual", r_mine, bound(r_np64))
    assert r_mine <= bound(r_np64), (label, r_mine, r_np64)
    it = np.asarray(got["iters"])
    for e in range(n):
        assert abs(int(it[e]) - f64[e]["iters"]) <= 1, (label, e, int(it[e]), f64[e]["iters"])
    X = np.asarray(got["X"])
    assert np.array_equal(X, X.transpose(0, 2, 1)), f"{label}: X is not bitwise symmetric"
    return tr, f64


# ---- the failures: reported through memory, written as zeros, isolated ---------------------------------------------------------------
def _bad_cases():
    base = generator_case(7, 3, 5)
    neg_r = {k: v.copy() for k, v in base.items()}
    neg_r["R"][2] = -np.eye(3)
    two = generator_case(2, 1, 5)
    unstab = {k: v.copy() for k, v in two.items()}
    unstab["A"][2], unstab["B"][2], unstab["Q"][2], unstab["R"][2] = np.diag([1.1, 0.5]), np.array([[0.0], [1.0]]), np.eye(2), np.eye(1)
    return [("negative_R", neg_r, MAX_ITER, 1), ("not_stabilisable", unstab, MAX_ITER, 2), ("max_iter_3", base, 3, 3)]


def check_statuses(solve, label):
    """The status and isolation test of both suites: ``solve(case, max_iter)`` -> outputs.  The failed problem (index 2 of 5; every problem with max_iter = 3)
    has the status, zeros for X and K and finite iters / change; the other four are bitwise what a launch of those four alone returns."""
    for name, case, max_iter, status in _bad_cases():
        got = solve(case, max_iter)
        bad = [0, 1, 2, 3, 4] if status == 3 else [2]
        keep = [e for e in range(5) if e not in bad]
        assert np.asarray(got["status"]).tolist() == [status if e in bad else 0 for e in range(5)], (label, name, got["status"])
        for e in bad:
            assert np.array_equal(got["X"][e], np.zeros_like(got["X"][e])) and np.array_equal(got["K"][e], np.zeros_like(got["K"][e])), (label, name)
            assert 0 <= got["iters"][e] <= max_iter and not np.isnan(got["change"][e]), (label, name, got["iters"][e], got["change"][e])
        assert np.isfinite(got["X"]).all() and np.isfinite(got["K"]).all(), (label, name)
        if status == 3:
            assert (np.asarray(got["iters"]) == 3).all() and (np.asarray(got["change"]) > TOL).all()
            continue
        if status == 2:
            ref = restate(case["A"][2], case["B"][2], case["Q"][2], case["R"][2], np.float64)
            assert ref["status"] == 2 and abs(int(got["iters"][2]) - ref["iters"]) <= 1, (got["iters"][2], ref["iters"])
        alone = solve({k: v[keep] for k, v in case.items()}, max_iter)
        for key in ("X", "K", "change", "iters", "status"):
            assert np.array_equal(np.asarray(got[key])[keep], np.asarray(alone[key])), (label, name, key)
