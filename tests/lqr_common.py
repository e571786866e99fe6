"""Shared by tests/test_lqr_host.py and tests/test_gpu_lqr.py: the yardstick of the LQR kernels.  Not a test module.

The yardstick is never the kernel: ``restate`` is a plain numpy restatement of the recursion of ``mjb_lqr_backward``
(include/mjbatch.h), run in ``np.longdouble`` as the truth and in ``np.float64`` as the measure of what float64 arithmetic alone
loses; ``bound`` turns the two into the tolerance (8 x the float64 restatement's own error, with an absolute floor)."""
from __future__ import annotations

import numpy as np

SIZES = [(4, 1, 200), (7, 3, 64), (12, 4, 200), (54, 21, 100), (64, 32, 50)]
# (nx, nu) at the edges of the launch dispatch: lqr_waves(nx) is 1 for nx <= 16 and 4 above, and the backward, box and DARE launches
# take <1, 8> for nx <= 16, nu <= 8, <1, kLqrMaxNu> for nx <= 16, nu > 8 and <4, kLqrMaxNu> for nx > 16 (NW waves, MU the unroll bound
# of the register-resident substitutions).  Every product is made of 16 x 16 tiles, at most four per wave.
EDGE_SIZES = [
    (1, 1),      # <1, 8>: the smallest system, every product one tile holding one entry
    (2, 2),      # <1, 8>: the smallest with off-diagonal entries and a pivot choice in the LU
    (3, 9),      # <1, 32>: nu = 9 is the first size past the MU switch; nu > nx
    (8, 9),      # <1, 32>: nu = 9 beside nx = 8 (nu > nx by one)
    (15, 16),    # <1, 32>: the last size with one partial tile per side; nu = 16 fills its tile
    (16, 8),     # <1, 8>: the largest one-wave state with the largest nu of the short unroll
    (16, 9),     # <1, 32>: the same state on the other side of the MU switch
    (16, 32),    # <1, 32>: B'VB is 2 x 2 tiles - all four tile slots of the single wave are used
    (17, 9),     # <4, 32>: the first four-wave state (two tiles per side, the second holding one row), nu past the MU switch
    (17, 32),    # <4, 32>: the first four-wave state with the largest nu (nu > nx, 2 x 2 tiles in every product)
    (33, 9),     # <4, 32>: three tiles per side, the last holding one row (DARE and Lyapunov)
]
# (nx, nu, T) of the backward pass at those edges: every size above but (33, 9), the horizons cut so that a case stays quick, and the
# horizons T = 1 and T = 2 (the prefetch of step t - 1 is guarded by t > 0: T = 1 never prefetches, T = 2 prefetches once)
EDGE_BACKWARD = [(1, 1, 1), (2, 2, 40), (3, 9, 40), (8, 9, 40), (15, 16, 30), (16, 8, 30), (16, 9, 30), (16, 32, 20), (17, 9, 20), (17, 32, 12),
                 (12, 4, 1), (12, 4, 2)]
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


# ---- the candidate loop at its edges ----------------------------------------------------------------------------------------------------
# (nx, nu, T, B, nalpha).  The kernel's 256 threads loop over nalpha * nu controls and nalpha * nx states per step: one item; fewer
# items than threads (45 and 15); nu > nx with 2048 and 1024 items (8 and 4 passes); the largest call (2048 and 4096 items); odd
# counts (147 and 378 items: less than one pass, and a second pass partly filled).
CAND_SIZES = [(1, 1, 20, 3, 1), (3, 9, 20, 3, 5), (16, 32, 12, 2, 64), (64, 32, 8, 2, 64), (54, 21, 10, 2, 7)]
CAND_HOST_SIZES = CAND_SIZES[:3]                                 # what the host emulation runs: the three smaller ones
# (dx0, bounds): dx0 absent, one per trajectory [B, nx], one shared [nx]; both bounds as numbers, one side only, per-actuator arrays
CAND_VARIANTS = [("none", "both"), ("per_env", "both"), ("shared", "both"), ("per_env", "lo_only"), ("per_env", "hi_only"), ("per_env", "per_actuator")]
CAND_LO, CAND_HI, CAND_TIGHT, CAND_WIDE = -0.8, 0.9, 0.3, 1e3
_CAND = {}


def candidate_case(nx, nu, T, B, na):
    """The inputs of one size, computed once and never modified, time-major: A [T, B, nx, nx], B [T, B, nx, nu], the gains k [T, B, nu],
    K [T, B, nu, nx] of the float64 restatement of the backward pass, a nominal u [T, B, nu] inside [CAND_LO, CAND_HI] with some entries
    on them, dx0 [B, nx], and alphas = 0 followed by 1 ... 1e-3 (nalpha = 1: the full step alone)."""
    key = (nx, nu, T, B, na)
    if key not in _CAND:
        p = generate(nx, nu, T, B)
        sol = restate_batch(p, np.float64)
        assert (sol["status"] == 0).all()
        rng = np.random.default_rng(5)
        c = {"A": p["A"], "B": p["B"], "k": np.ascontiguousarray(sol["k"].transpose(1, 0, 2)), "K": np.ascontiguousarray(sol["K"].transpose(1, 0, 2, 3)),
             "u": np.clip(rng.normal(size=(T, B, nu)), CAND_LO, CAND_HI), "dx0": 0.1 * rng.normal(size=(B, nx)),
             "alphas": np.array([1.0]) if na == 1 else np.concatenate([[0.0], np.logspace(0, -3, na - 1)])}
        _CAND[key] = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in c.items()}
    return _CAND[key]


def candidate_variant(c, dx0_kind, bounds_kind):
    """(dx0, lo, hi) of a variant: dx0 None, [B, nx] or [nx] (the first trajectory's, for all); lo / hi None or [nu].  per_actuator:
    the even actuators are held in [-CAND_TIGHT, CAND_TIGHT] (inside the nominal's range: they clamp), the odd ones in
    [-CAND_WIDE, CAND_WIDE] (never reached)."""
    nu = c["u"].shape[2]
    dx0 = {"none": None, "per_env": c["dx0"], "shared": c["dx0"][0].copy()}[dx0_kind]
    if bounds_kind == "per_actuator":
        half = np.where(np.arange(nu) % 2 == 0, CAND_TIGHT, CAND_WIDE)
        return dx0, -half, half
    lo = None if bounds_kind == "hi_only" else np.full(nu, CAND_LO)
    hi = None if bounds_kind == "lo_only" else np.full(nu, CAND_HI)
    return dx0, lo, hi


def candidate_restatement(c, dx0, lo, hi, dtype, alphas=None):
    """``restate_candidates`` for every trajectory of a ``candidate_case``: [B, nalpha, T, nu]."""
    B = c["A"].shape[1]
    alphas = c["alphas"] if alphas is None else alphas
    return np.stack([restate_candidates(c["A"][:, e], c["B"][:, e], c["k"][:, e], c["K"][:, e], c["u"][:, e], alphas,
                                        None if dx0 is None else dx0[e] if dx0.ndim == 2 else dx0, lo, hi, dtype) for e in range(B)])


def judge_candidates(c, got, dx0_kind, bounds_kind, label, record=None):
    """The comparison both suites make on a variant: each trajectory of ``got`` [B, nalpha, T, nu] against the long-double restatement
    within ``bound`` of the float64 restatement's own error; and, on the long-double restatement alone, that the variant is what it
    says - some control is clamped on each bounded side and some is free, with per-actuator bounds every even actuator is clamped at
    some step (nu = 1 has no second actuator: there the one actuator is clamped at some steps and free at others) and no odd one ever
    is, and a dx0 changes the result.  Returns the long-double restatement."""
    dx0, lo, hi = candidate_variant(c, dx0_kind, bounds_kind)
    truth, f64 = candidate_restatement(c, dx0, lo, hi, np.longdouble), candidate_restatement(c, dx0, lo, hi, np.float64)
    at_lo = np.zeros(truth.shape, dtype=bool) if lo is None else truth == lo
    at_hi = np.zeros(truth.shape, dtype=bool) if hi is None else truth == hi
    clamped = at_lo | at_hi
    assert (lo is None or at_lo.any()) and (hi is None or at_hi.any()) and not clamped.all(), (label, "the variant clamps nothing or everything")
    if bounds_kind == "per_actuator":
        per = clamped.any(axis=(0, 1, 2))
        assert per[0::2].all() and not per[1::2].any(), (label, per)
        assert np.abs(truth[..., 1::2]).max(initial=0.0) < 0.5 * CAND_WIDE
    if dx0 is not None:
        assert not np.array_equal(truth, candidate_restatement(c, None, lo, hi, np.longdouble)), (label, "dx0 changes nothing")
    for e in range(truth.shape[0]):
        mine, np64 = rel_err(got[e], truth[e]), rel_err(f64[e], truth[e])
        print(f"{label} env {e}: kernel {mine:.3e}  float64 numpy {np64:.3e}  bound {bound(np64):.3e}")
        if record:
            record(f"{label}/env{e}", mine, bound(np64), f"(float64 numpy restatement: {np64:.3e})")
        assert mine <= bound(np64), (label, e, mine, np64)
    return truth
