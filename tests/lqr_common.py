"""Shared by tests/test_lqr_host.py and tests/test_gpu_lqr.py: the yardstick of the LQR kernels.  Not a test module.

The yardstick is never the kernel: ``restate`` is a plain numpy restatement of the recursion of ``mjb_lqr_backward``
(include/mjbatch.h), run in ``np.longdouble`` as the truth and in ``np.float64`` as the measure of what float64 arithmetic alone
loses; ``bound`` turns the two into the tolerance (8 x the float64 restatement's own error, with an absolute floor)."""
from __future__ import annotations

import numpy as np

SIZES = [(4, 1, 200), (7, 3, 64), (12, 4, 200), (54, 21, 100), (64, 32, 50)]
OUTPUTS = ("k", "K", "V0x", "V0xx", "dV")
FACTOR, FLOOR, FLOOR_DARE = 8.0, 1e-13, 1e-11


def generate(nx, nu, T, B, seed=0, constant=False):
    """B random systems: A_t = I + 0.02 G / sqrt(nx) + 0.005 G_t / sqrt(nx), B_t = 0.05 G, Q = diag(U[0.1, 10]), R = 0.01 I,
    VxxT = 20 Q, VxT = 0, lx ~ N(0, 1), lu ~ 0.1 N(0, 1), mu = 1e-6.  Arrays are [T, B, ...]; Q, R, VxxT per system [B, ...]."""
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(B, nx, nx))
    Gt = rng.normal(size=(T, B, nx, nx)) * (0.0 if constant else 1.0)
    A = np.eye(nx)[None, None] + 0.02 * G[None] / np.sqrt(nx) + 0.005 * Gt / np.sqrt(nx)
    Bm = np.broadcast_to(0.05 * rng.normal(size=(1, B, nx, nu)), (T, B, nx, nu)).copy()
    Q = np.stack([np.diag(rng.uniform(0.1, 10.0, size=nx)) for _ in range(B)])
    R = np.broadcast_to(0.01 * np.eye(nu), (B, nu, nu)).copy()
    return {"A": A, "B": Bm, "Q": Q, "R": R, "VxxT": 20.0 * Q, "VxT": np.zeros((B, nx)),
            "lx": rng.normal(size=(T, B, nx)), "lu": 0.1 * rng.normal(size=(T, B, nu)), "mu": 1e-6}


def _chol_solve(M, R):
    """X with M X = R by Cholesky in M's dtype, or None at a pivot that is <= 0 or not finite."""
    n = M.shape[0]
    W, L = M.copy(), np.zeros_like(M)
    for j in range(n):
        d = W[j, j]
        if not (d > 0) or not np.isfinite(d):
            return None
        s = np.sqrt(d)
        L[j, j] = s
        L[j + 1:, j] = W[j + 1:, j] / s
        W[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    Y = R.copy()
    for j in range(n):
        Y[j] = (Y[j] - L[j, :j] @ Y[:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        Y[j] = (Y[j] - L[j + 1:, j] @ Y[j + 1:]) / L[j, j]
    return Y


def restate(A, Bm, lx, lu, lxx, luu, lux, VxT, VxxT, mu, dtype):
    """ONE trajectory.  A [T, nx, nx], Bm [T, nx, nu], lx [T, nx], lu [T, nu]; lxx, luu, lux [T, ...] or constant [...] (lux None = 0).
    Returns dict k [T, nu], K [T, nu, nx], V0x, V0xx, dV [2], status - the zeros of a failed trajectory included."""
    c = lambda x: None if x is None else np.asarray(x).astype(dtype)
    A, Bm, lx, lu, lxx, luu, lux, Vx, Vxx = (c(x) for x in (A, Bm, lx, lu, lxx, luu, lux, VxT, VxxT))
    mu = dtype(mu)
    T, nx, nu = A.shape[0], A.shape[1], Bm.shape[2]
    at = lambda x, t, nd: x if x.ndim == nd else x[t]
    k, K = np.zeros((T, nu), dtype=dtype), np.zeros((T, nu, nx), dtype=dtype)
    dV = np.zeros(2, dtype=dtype)
    half, eye = dtype(0.5), np.eye(nu, dtype=dtype)
    for t in range(T - 1, -1, -1):
        At, Bt = A[t], Bm[t]
        Qx, Qu = at(lx, t, 1) + At.T @ Vx, at(lu, t, 1) + Bt.T @ Vx
        Qxx = at(lxx, t, 2) + At.T @ Vxx @ At
        Quu = at(luu, t, 2) + Bt.T @ Vxx @ Bt + mu * eye
        Qux = Bt.T @ Vxx @ At
        if lux is not None:
            Qux = at(lux, t, 2) + Qux
        X = _chol_solve(Quu, np.concatenate([Qux, Qu[:, None]], axis=1))
        if X is None:
            k[:t + 1] = 0; K[:t + 1] = 0
            return {"k": k, "K": K, "V0x": np.zeros(nx, dtype=dtype), "V0xx": np.zeros((nx, nx), dtype=dtype), "dV": np.zeros(2, dtype=dtype), "status": 1 + t}
        K[t], k[t] = -X[:, :nx], -X[:, nx]
        dV[0] += k[t] @ Qu
        dV[1] += half * (k[t] @ Quu @ k[t])
        Vx = Qx + K[t].T @ Quu @ k[t] + K[t].T @ Qu + Qux.T @ k[t]
        Vxx = Qxx + K[t].T @ Quu @ K[t] + K[t].T @ Qux + Qux.T @ K[t]
        Vxx = half * (Vxx + Vxx.T)
    return {"k": k, "K": K, "V0x": Vx, "V0xx": Vxx, "dV": dV, "status": 0}


def restate_batch(p, dtype, lux=None, constant_cost=True):
    """``restate`` for every system of a ``generate`` dict: outputs stacked [B, ...]."""
    B = p["A"].shape[1]
    res = [restate(p["A"][:, e], p["B"][:, e], p["lx"][:, e], p["lu"][:, e], p["Q"][e], p["R"][e], None if lux is None else lux[:, e],
                   p["VxT"][e], p["VxxT"][e], np.asarray(p["mu"]).reshape(-1)[e if np.ndim(p["mu"]) else 0], dtype) for e in range(B)]
    return {key: np.stack([np.asarray(r[key]) for r in res]) for key in OUTPUTS + ("status",)}


def rel_err(x, truth):
    """max|x - truth| / max|truth| (0 / 0 = 0), evaluated in long double."""
    x, truth = np.asarray(x, dtype=np.longdouble), np.asarray(truth, dtype=np.longdouble)
    den = np.abs(truth).max()
    num = np.abs(x - truth).max()
    return float(num / den) if den > 0 else float(num)


def bound(f64_value, floor=FLOOR):
    return max(FACTOR * f64_value, floor)


def restate_candidates(A, Bm, k, K, u, alphas, dx0, lo, hi, dtype):
    """ONE trajectory: A [T, nx, nx], Bm [T, nx, nu], k [T, nu], K [T, nu, nx], u [T, nu] -> cand [nalpha, T, nu]."""
    c = lambda x: None if x is None else np.asarray(x).astype(dtype)
    A, Bm, k, K, u, alphas, dx0, lo, hi = (c(x) for x in (A, Bm, k, K, u, alphas, dx0, lo, hi))
    T, nx, nu = A.shape[0], A.shape[1], Bm.shape[2]
    out = np.zeros((len(alphas), T, nu), dtype=dtype)
    for j, a in enumerate(alphas):
        dx = np.zeros(nx, dtype=dtype) if dx0 is None else dx0.copy()
        for t in range(T):
            ct = u[t] + a * k[t] + K[t] @ dx
            if lo is not None:
                ct = np.maximum(ct, lo)
            if hi is not None:
                ct = np.minimum(ct, hi)
            out[j, t] = ct
            dx = A[t] @ dx + Bm[t] @ (ct - u[t])
    return out
