"""Shared by tests/test_lqr_box_host.py and tests/test_gpu_lqr_box.py: the yardstick of the control-limited backward pass
(``mjb_lqr_backward_box``, include/mjbatch.h).  Not a test module.

``restate_box`` is a plain numpy restatement of the contract: per step the box QP ``min x' Quu x / 2 + Qu' x, lob <= x <= hib`` by
projected Newton (Tassa, Mansard, Todorov, ICRA 2014), the polish solve on the final clamped set, the unchanged value update.  It is
built on ``lqr_common._chol_solve`` applied to the COMPACT free block - the kernel never gathers that block - and runs in
``np.longdouble`` (truth) and ``np.float64`` (the measure of the bound, as in ``lqr_common``)."""
from __future__ import annotations

import numpy as np

from tests import lqr_common as lc

QP_MAX_ITER, QP_MAX_TRIALS, ARMIJO, SHRINK = 64, 64, 0.1, 0.6
OUTPUTS = lc.OUTPUTS
BOUNDS = (0.5, 2.0)


def box_inputs(nx, nu, T, B, b, seed=7):
    """The inputs the issue sets: ``generate(nx, nu, T, B)`` (seed 0), lo = -b, hi = 1.25 b, u = clip(0.6 b N(0, 1), lo, hi) [T, B, nu]."""
    p = lc.generate(nx, nu, T, B)
    lo, hi = np.full(nu, -b), np.full(nu, 1.25 * b)
    p["lo"], p["hi"] = lo, hi
    p["u"] = np.clip(0.6 * b * np.random.default_rng(seed).normal(size=(T, B, nu)), lo, hi)
    return p


def _clip(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def _clamped(x, g, lo, hi):
    return ((x == lo) & (g > 0)) | ((x == hi) & (g < 0))


def box_qp(Quu, Qu, lob, hib):
    """One QP in Quu's dtype.  Returns x (the last iterate), c (its clamped set), iterations, 'ok' / 'cap' / 'search' / None at a bad
    pivot, and whether the Armijo search ran."""
    dtype = Quu.dtype.type
    x = _clip(np.zeros_like(Qu), lob, hib)
    f = lambda y: y @ Qu + dtype(0.5) * (y @ Quu @ y)
    g = Qu + Quu @ x
    c = _clamped(x, g, lob, hib)
    iters, searched = 0, False
    while True:
        iters += 1
        if c.all():
            return x, c, iters, "ok", searched
        fr = ~c
        sol = lc._chol_solve(Quu[np.ix_(fr, fr)], (Qu[fr] + Quu[np.ix_(fr, c)] @ x[c])[:, None])
        if sol is None:
            return x, c, iters, None, searched
        xs = x.copy()
        xs[fr] = -sol[:, 0]
        if np.array_equal(_clip(xs, lob, hib), xs):
            x = xs
            g = Qu + Quu @ x
            c2 = _clamped(x, g, lob, hib)
            if np.array_equal(c2, c):
                return x, c, iters, "ok", searched
            c = c2
        else:
            searched = True
            d = xs - x
            sdotg, fold, s, xt = g @ d, f(x), dtype(1.0), None
            for _ in range(QP_MAX_TRIALS):
                y = _clip(x + s * d, lob, hib)
                if sdotg < 0 and f(y) - fold <= dtype(ARMIJO) * s * sdotg:
                    xt = y
                    break
                s = s * dtype(SHRINK)
            if xt is None:
                return x, c, iters, "search", searched
            x = xt
            g = Qu + Quu @ x
            c = _clamped(x, g, lob, hib)
        if iters == QP_MAX_ITER:
            return x, c, iters, "cap", searched


def restate_box(A, Bm, lx, lu, lxx, luu, lux, VxT, VxxT, mu, u, lo, hi, dtype):
    """ONE trajectory (the arguments of ``lqr_common.restate`` plus u [T, nu], lo / hi [nu] or None).  Returns the outputs of
    ``restate`` plus clamped [T] (bit masks), cmask [T, nu], qp_iters, margin (the smallest distance of a free control from its bounds
    or |g| of a clamped one), searches (QPs in which the Armijo search ran)."""
    c_ = lambda x: None if x is None else np.asarray(x).astype(dtype)
    A, Bm, lx, lu, lxx, luu, lux, Vx, Vxx, u = (c_(x) for x in (A, Bm, lx, lu, lxx, luu, lux, VxT, VxxT, u))
    T, nx, nu = A.shape[0], A.shape[1], Bm.shape[2]
    lo = np.full(nu, -np.inf, dtype=dtype) if lo is None else c_(lo)
    hi = np.full(nu, np.inf, dtype=dtype) if hi is None else c_(hi)
    mu = dtype(mu)
    at = lambda x, t, nd: x if x.ndim == nd else x[t]
    k, K = np.zeros((T, nu), dtype=dtype), np.zeros((T, nu, nx), dtype=dtype)
    cmask = np.zeros((T, nu), dtype=bool)
    dV = np.zeros(2, dtype=dtype)
    half, eye = dtype(0.5), np.eye(nu, dtype=dtype)
    status, qp_iters, margin, searches = 0, 0, np.inf, 0

    def failed(t):
        k[:t + 1] = 0; K[:t + 1] = 0; cmask[:t + 1] = False
        return {"k": k, "K": K, "V0x": np.zeros(nx, dtype=dtype), "V0xx": np.zeros((nx, nx), dtype=dtype), "dV": np.zeros(2, dtype=dtype),
                "status": 1 + t, "clamped": _bits(cmask), "cmask": cmask, "qp_iters": qp_iters, "margin": margin, "searches": searches}

    for t in range(T - 1, -1, -1):
        At, Bt = A[t], Bm[t]
        Qx, Qu = at(lx, t, 1) + At.T @ Vx, at(lu, t, 1) + Bt.T @ Vx
        Qxx = at(lxx, t, 2) + At.T @ Vxx @ At
        Quu = at(luu, t, 2) + Bt.T @ Vxx @ Bt + mu * eye
        Qux = Bt.T @ Vxx @ At
        if lux is not None:
            Qux = at(lux, t, 2) + Qux
        lob, hib = lo - u[t], hi - u[t]
        x, c, iters, how, searched = box_qp(Quu, Qu, lob, hib)
        qp_iters, searches = max(qp_iters, iters), searches + int(searched)
        if how is None:
            return failed(t)
        if how != "ok" and status == 0:
            status = -(1 + t)
        fr = ~c
        kt, Kt = x.copy(), np.zeros((nu, nx), dtype=dtype)
        if fr.any():                                             # the polish: one solve on the final set
            X = lc._chol_solve(Quu[np.ix_(fr, fr)], np.concatenate([Qux[fr], (Qu[fr] + Quu[np.ix_(fr, c)] @ x[c])[:, None]], axis=1))
            if X is None:
                return failed(t)
            Kt[fr], kt[fr] = -X[:, :nx], -X[:, nx]
        kt = _clip(kt, lob, hib)
        g = Qu + Quu @ kt
        with np.errstate(invalid="ignore"):
            m = np.where(c, np.abs(g), np.minimum(kt - lob, hib - kt))
        margin = min(margin, float(m.min()))
        k[t], K[t], cmask[t] = kt, Kt, c
        dV[0] += kt @ Qu
        dV[1] += half * (kt @ Quu @ kt)
        Vx = Qx + Kt.T @ Quu @ kt + Kt.T @ Qu + Qux.T @ kt
        Vxx = Qxx + Kt.T @ Quu @ Kt + Kt.T @ Qux + Qux.T @ Kt
        Vxx = half * (Vxx + Vxx.T)
    return {"k": k, "K": K, "V0x": Vx, "V0xx": Vxx, "dV": dV, "status": status, "clamped": _bits(cmask), "cmask": cmask,
            "qp_iters": qp_iters, "margin": margin, "searches": searches}


def _bits(cmask):
    """[T, nu] bool -> [T] int32 bit masks (bit a = control a; nu = 32 wraps into the sign bit as the kernel's int32 does)."""
    w = (cmask.astype(np.uint64) << np.arange(cmask.shape[1], dtype=np.uint64)[None]).sum(axis=1)
    return w.astype(np.uint32).view(np.int32)


def restate_box_batch(p, dtype, lo="p", hi="p"):
    """``restate_box`` for every system of a ``box_inputs`` dict (``lo`` / ``hi``: "p" = the dict's, or an array / None): stacked [B, ...]."""
    B = p["A"].shape[1]
    lo = p["lo"] if isinstance(lo, str) else lo
    hi = p["hi"] if isinstance(hi, str) else hi
    res = [restate_box(p["A"][:, e], p["B"][:, e], p["lx"][:, e], p["lu"][:, e], p["Q"][e], p["R"][e], None, p["VxT"][e], p["VxxT"][e],
                       np.asarray(p["mu"]).reshape(-1)[e if np.ndim(p["mu"]) else 0], p["u"][:, e], lo, hi, dtype) for e in range(B)]
    out = {key: np.stack([np.asarray(r[key]) for r in res]) for key in OUTPUTS + ("status", "clamped", "cmask", "qp_iters", "searches")}
    out["margin"] = min(r["margin"] for r in res)
    return out


_CASES = {}


def case(nx, nu, T, b, B=3, shared_cost=False):
    """Inputs and the two restatements of one (size, bound): computed once, shared among the tests, never modified.
    ``shared_cost``: every system takes the first one's Q (and VxxT = 20 Q), the form passed once with both strides 0."""
    key = (nx, nu, T, b, B, shared_cost)
    if key not in _CASES:
        p = box_inputs(nx, nu, T, B, b)
        if shared_cost:
            p["Q"] = np.broadcast_to(p["Q"][0], p["Q"].shape).copy()
            p["VxxT"] = 20.0 * p["Q"]
        _CASES[key] = (p, restate_box_batch(p, np.longdouble), restate_box_batch(p, np.float64))
    return _CASES[key]


MARGIN_MIN = 1e-6


def preconditions(truth, f64):
    """What every test asserts on the restatement before it looks at the kernel: the two precisions find the same clamped sets, no
    decision is closer than 1e-6 to flipping, every QP ended through the tolerance-free criterion."""
    assert np.array_equal(truth["cmask"], f64["cmask"])
    assert (truth["status"] == 0).all() and (f64["status"] == 0).all()
    assert min(truth["margin"], f64["margin"]) >= MARGIN_MIN, (truth["margin"], f64["margin"])
    assert 1 <= int(truth["qp_iters"].max()) <= QP_MAX_ITER


def enumerate_qp(Quu, Qu, lob, hib):
    """The QP's solution by enumeration in long double: every assignment of {free, at lob, at hib} to the controls, the KKT point of
    each, the feasible one with multipliers of the right sign.  Independent of ``box_qp``."""
    import itertools

    ld = np.longdouble
    Quu, Qu, lob, hib = (np.asarray(x, dtype=ld) for x in (Quu, Qu, lob, hib))
    n, best = len(Qu), None
    for assign in itertools.product((0, 1, 2), repeat=n):
        a = np.array(assign)
        x = np.where(a == 1, lob, np.where(a == 2, hib, ld(0)))
        fr = a == 0
        if not np.isfinite(x).all():
            continue
        if fr.any():
            x[fr] = np.linalg.solve(Quu[np.ix_(fr, fr)].astype(np.float64), -(Qu[fr] + Quu[np.ix_(fr, ~fr)] @ x[~fr]).astype(np.float64))
            r = Quu[np.ix_(fr, fr)] @ x[fr] + Qu[fr] + Quu[np.ix_(fr, ~fr)] @ x[~fr]          # one step of refinement in long double
            x[fr] = x[fr] - np.linalg.solve(Quu[np.ix_(fr, fr)].astype(np.float64), r.astype(np.float64))
        g = Qu + Quu @ x
        if (x >= lob).all() and (x <= hib).all() and (g[a == 1] >= 0).all() and (g[a == 2] <= 0).all():
            val = x @ Qu + ld(0.5) * (x @ Quu @ x)
            if best is None or val < best[0]:
                best = (val, x)
    return best[1]
