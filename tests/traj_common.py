"""Shared by tests/test_traj_cost_host.py and tests/test_gpu_traj_cost.py: the yardstick of ``mjb_traj_cost`` / ``mjb_traj_select``.
Not a test module.

The yardstick is never the kernel: ``restate_cost`` / ``restate_select`` are plain numpy restatements of the formulas in
include/mjbatch.h (the quaternion difference of ``mjb_differentiate_pos`` included), run in ``np.longdouble`` as the truth and in
``np.float64`` as the measure of what float64 arithmetic alone loses; the bound is ``lqr_common.bound`` of the two (8 x the float64
restatement's own error, floor 1e-13), errors measured with ``lqr_common.rel_err``."""
from __future__ import annotations

import numpy as np

COST_OUTPUTS = ("cost", "cost_t", "lx", "lu", "VxT")
JNT_FREE = 0


def joint_table(cm):
    return (np.ascontiguousarray(cm.jnt_type, dtype=np.int32), np.ascontiguousarray(cm.jnt_qposadr, dtype=np.int32),
            np.ascontiguousarray(cm.jnt_dofadr, dtype=np.int32))


def _quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], dtype=a.dtype)


def differentiate_pos(table, nv, qref, qpos, dtype):
    """``mjb_differentiate_pos(out, 1, qref, qpos)`` for ONE configuration, in ``dtype``: scalar joints subtract, a free joint subtracts
    its position and turns conj(qref) * qpos into angle * axis (angle in (-pi, pi])."""
    jt, jq, jd = table
    qref, qpos = np.asarray(qref).astype(dtype), np.asarray(qpos).astype(dtype)
    out = np.zeros(nv, dtype=dtype)
    pi = dtype(4) * np.arctan(dtype(1))
    for j in range(len(jt)):
        qa, da = int(jq[j]), int(jd[j])
        if jt[j] != JNT_FREE:
            out[da] = qpos[qa] - qref[qa]
            continue
        out[da:da + 3] = qpos[qa:qa + 3] - qref[qa:qa + 3]
        q1 = qref[qa + 3:qa + 7]
        qd = _quat_mul(np.array([q1[0], -q1[1], -q1[2], -q1[3]], dtype=dtype), qpos[qa + 3:qa + 7])
        sn = np.sqrt(qd[1] * qd[1] + qd[2] * qd[2] + qd[3] * qd[3])
        if sn < 1e-15:
            continue
        ang = dtype(2) * np.arctan2(sn, qd[0])
        if ang > pi:
            ang -= dtype(2) * pi
        out[da + 3:da + 6] = qd[1:] * (ang / sn)
    return out


def restate_cost(table, nq, nv, nu, x, u, x_ref, u_ref, Q, R, Qf, dtype):
    """``x [B, T+1, nq+nv]`` (point 0 = the start state), ``u [B, T, nu]``, ``x_ref`` like ``x`` or ``[nq+nv]``, ``u_ref`` like ``u``,
    ``[nu]`` or None, ``Q [B, T, nx, nx]`` or ``[nx, nx]``, ``R`` likewise, ``Qf [B, nx, nx]`` or ``[nx, nx]``.  The inputs are widened
    to ``dtype`` exactly (they are float32 or float64 values); every operation after that is ``dtype`` arithmetic."""
    B, T, nx = x.shape[0], x.shape[1] - 1, 2 * nv
    c = lambda a: np.asarray(a).astype(dtype)
    x, u = c(x), c(u)
    x_ref = np.broadcast_to(c(x_ref), x.shape)
    u_ref = np.zeros(u.shape, dtype=dtype) if u_ref is None else np.broadcast_to(c(u_ref), u.shape)
    Q, R, Qf = np.broadcast_to(c(Q), (B, T, nx, nx)), np.broadcast_to(c(R), (B, T, nu, nu)), np.broadcast_to(c(Qf), (B, nx, nx))
    half = dtype(0.5)
    out = {"cost": np.zeros(B, dtype=dtype), "cost_t": np.zeros((B, T + 1), dtype=dtype), "lx": np.zeros((B, T, nx), dtype=dtype),
           "lu": np.zeros((B, T, nu), dtype=dtype), "VxT": np.zeros((B, nx), dtype=dtype), "dx": np.zeros((B, T + 1, nx), dtype=dtype)}
    for e in range(B):
        for t in range(T + 1):
            dx = np.concatenate([differentiate_pos(table, nv, x_ref[e, t, :nq], x[e, t, :nq], dtype), x[e, t, nq:] - x_ref[e, t, nq:]])
            out["dx"][e, t] = dx
            if t == T:
                out["VxT"][e] = Qf[e] @ dx
                out["cost_t"][e, t] = half * (dx @ out["VxT"][e])
                continue
            du = u[e, t] - u_ref[e, t]
            out["lx"][e, t], out["lu"][e, t] = Q[e, t] @ dx, R[e, t] @ du
            out["cost_t"][e, t] = half * (dx @ out["lx"][e, t]) + half * (du @ out["lu"][e, t])
        s = out["cost_t"][e].sum()
        out["cost"][e] = s if np.isfinite(s) else np.inf
    return out


def restate_select(cost, cand, mode, temperature, dtype):
    """``cost [G, n]``, ``cand [G, n, T, nu]`` -> u [G, T, nu] (NaN rows where no cost is finite: not written), best, best_cost, weights."""
    G, n = cost.shape
    cost_d, cand_d = np.asarray(cost).astype(dtype), np.asarray(cand).astype(dtype)
    u = np.full(cand.shape[:1] + cand.shape[2:], np.nan, dtype=dtype)
    best, best_cost, w = np.full(G, -1, dtype=np.int64), np.full(G, np.inf, dtype=dtype), np.zeros((G, n), dtype=dtype)
    for g in range(G):
        fin = np.isfinite(cost[g])
        if not fin.any():
            continue
        cmin = cost_d[g][fin].min()
        best[g] = int(np.flatnonzero(fin & (cost_d[g] == cmin))[0])
        best_cost[g] = cmin
        if mode == "argmin":
            u[g] = cand_d[g, best[g]]
            continue
        ex = np.zeros(n, dtype=dtype)
        ex[fin] = np.exp(-(cost_d[g][fin] - cmin) / dtype(temperature))
        w[g] = ex / ex.sum()
        u[g] = np.tensordot(w[g], cand_d[g], axes=(0, 0))
    return {"u": u, "best": best, "best_cost": best_cost, "weights": w}


def _rand_unit_quat(rng, size):
    q = rng.normal(size=size + (4,))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def generate(cm, T, B, seed=0, state_dtype=np.float64, per_point_cost=False):
    """A test case on compiled model ``cm``: ``x [B, T+1, nq+nv]`` in ``state_dtype``, ``u [B, T, nu]`` float64, references and dense,
    non-diagonal, symmetric positive definite cost matrices (one for all points, or one per (t, e)).  Every free joint of ``x`` is
    rotated against its reference by an angle in [0.05, 2.5] rad about a random axis - away from the pi wrap and from the zero-angle
    branch; point (0, 1) has qpos == qref exactly (dx = 0 there)."""
    rng = np.random.default_rng(seed)
    nq, nv, nu, nx = int(cm.nq), int(cm.nv), int(cm.nu), 2 * int(cm.nv)
    jt, jq, _ = joint_table(cm)
    x_ref = rng.normal(size=(B, T + 1, nq + nv)) * 0.5
    x = x_ref + rng.normal(size=x_ref.shape) * 0.3
    for j in range(len(jt)):
        if jt[j] != JNT_FREE:
            continue
        qa = int(jq[j])
        qr = _rand_unit_quat(rng, (B, T + 1))
        ang = rng.uniform(0.05, 2.5, size=(B, T + 1, 1))
        axis = rng.normal(size=(B, T + 1, 3))
        axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
        rot = np.concatenate([np.cos(0.5 * ang), np.sin(0.5 * ang) * axis], axis=-1)
        x_ref[..., qa + 3:qa + 7] = qr
        for e in range(B):
            for t in range(T + 1):
                x[e, t, qa + 3:qa + 7] = _quat_mul(qr[e, t], rot[e, t])
    x = x.astype(state_dtype)
    x_ref[0, 1, :nq] = x[0, 1, :nq]                               # exactly equal after widening

    def spd(n, lead):
        G = rng.normal(size=lead + (n, n))
        M = G @ np.swapaxes(G, -1, -2) / n + np.eye(n) * rng.uniform(0.1, 10.0, size=lead + (n, 1))
        return 0.5 * (M + np.swapaxes(M, -1, -2))

    lead = (B, T) if per_point_cost else ()
    return {"x": x, "u": rng.normal(size=(B, T, nu)), "x_ref": x_ref, "u_ref": rng.normal(size=(B, T, nu)) * 0.1,
            "Q": spd(nx, lead), "R": spd(nu, lead), "Qf": spd(nx, (B,) if per_point_cost else ()), "nq": nq, "nv": nv, "nu": nu}


def float32_ulp_error(x32, truth):
    """max |x32 - float32(truth)| in float32 ulps of float32(truth): a float32 output is the rounding of a float64 value that close to
    the truth, so it may land on a neighbour of the truth's own rounding - at most 1."""
    t32 = np.asarray(truth).astype(np.float32)
    ulp = np.spacing(np.abs(t32)).astype(np.float64)
    return float((np.abs(np.asarray(x32, dtype=np.float64) - t32.astype(np.float64)) / ulp).max())
