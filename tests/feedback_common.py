"""Shared by tests/test_feedback_host.py and tests/test_gpu_feedback.py: the yardstick of ``mjb_feedback_law``.  Not a test module.

The yardstick is never the kernel: ``restate`` is a plain numpy restatement of the law in include/mjbatch.h (the quaternion difference
of ``mjb_differentiate_pos`` through ``traj_common.differentiate_pos``), run in ``np.longdouble`` as the truth and in ``np.float64`` as
the measure of what float64 arithmetic alone loses.  A bound is 8 x the float64 restatement's own figure for that environment, with a
floor: the worst float64-restatement figure over the whole case list (five environments, three steps per case), measured on the CPU
with ``python -m tests.feedback_common`` and written below.  For float32 data ``2^-24 |truth|`` is added for the one output rounding.

Error measure of actuator ``a``: ``|u_a - u*_a| / (|u0_a| + sum_k |K[a, k]| |dx*_k|)``, the size of the terms ``u_a`` is summed from; the
figure of an environment is the largest over its actuators."""
from __future__ import annotations

import numpy as np

from tests.traj_common import differentiate_pos

FACTOR = 8.0
FLOOR = 1.92e-16       # the worst float64-restatement figure over CASES (python -m tests.feedback_common prints it)
NOT_FINITE, CLIPPED = 1, 2
JNT_FREE, JNT_HINGE = 0, 3


def bound(f64_value):
    return max(FACTOR * f64_value, FLOOR)


# ---- synthetic joint tables: name -> (jnt_type, jnt_qposadr, jnt_dofadr, nq, nv, nu) ----------------------------------------------------
def _table(kinds):
    jt, jq, jd, nq, nv = [], [], [], 0, 0
    for k in kinds:
        jt.append(k); jq.append(nq); jd.append(nv)
        nq += 7 if k == JNT_FREE else 1
        nv += 6 if k == JNT_FREE else 1
    return (np.array(jt, dtype=np.int32), np.array(jq, dtype=np.int32), np.array(jd, dtype=np.int32)), nq, nv


SHAPES = {
    "hinge_pair": ([JNT_HINGE] * 2, 1),                                   # 1 x 4: nu * nx below one wavefront
    "drone": ([JNT_FREE], 4),                                             # nq 7, nv 6
    "humanoid": ([JNT_FREE] + [JNT_HINGE] * 21, 21),                      # nx 54, nu * nx = 1134: no multiple of 64
    "two_free": ([JNT_FREE] + [JNT_HINGE] * 52 + [JNT_FREE], 32),          # nv 64, nu 32: both limits at once
}


def shape(name):
    kinds, nu = SHAPES[name]
    table, nq, nv = _table(kinds)
    return table, nq, nv, nu


def limits(nu, seed=0):
    """Every second actuator ctrl-limited, with a range some controls of ``problem`` leave."""
    rng = np.random.default_rng(77 + seed)
    limited = (np.arange(nu) % 2 == 0).astype(np.int32)
    half = rng.uniform(0.5, 3.0, size=nu)
    mid = rng.normal(size=nu) * 0.3
    return limited, np.ascontiguousarray(np.stack([mid - half, mid + half], axis=1))


def _unit_quats(rng, shape_):
    q = rng.normal(size=shape_ + (4,))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def problem(table, nq, nv, nu, B, T, seed=0, gain=1.0):
    """Materialised K [B, T, nu, 2nv], u0 [B, T, nu], q0 [B, T, nq], v0 [B, T, nv] and a state qpos [B, nq], qvel [B, nv]: random gains,
    unit quaternions (set-point and state a generic rotation apart), float64."""
    rng = np.random.default_rng(1000 * nv + nu + 7919 * seed)
    jt, jq, _ = table
    K = rng.normal(size=(B, T, nu, 2 * nv)) * gain
    u0 = rng.normal(size=(B, T, nu))
    q0, v0 = rng.normal(size=(B, T, nq)), rng.normal(size=(B, T, nv))
    qpos, qvel = rng.normal(size=(B, nq)), rng.normal(size=(B, nv))
    for j in range(len(jt)):
        if jt[j] == JNT_FREE:
            a = int(jq[j]) + 3
            q0[..., a:a + 4] = _unit_quats(rng, (B, T))
            qpos[..., a:a + 4] = _unit_quats(rng, (B,))
    return K, u0, q0, v0, qpos, qvel


def restate(table, nv, K, u0, q0, v0, qpos, qvel, sign, clip, limited, ctrlrange, dtype):
    """ONE environment at one step: K [nu, 2nv], u0 [nu], q0 [nq], v0 [nv] or None, qpos [nq], qvel [nv] (float32 or float64 values,
    widened exactly).  Returns ``(u [nu] in dtype, status bits, scale [nu])`` - the zeros of a step that is not finite included."""
    c = lambda a: np.asarray(a).astype(dtype)
    nu = K.shape[0]
    ins = [K, u0, q0, qpos, qvel] + ([] if v0 is None else [v0])
    with np.errstate(all="ignore"):
        dx = np.concatenate([differentiate_pos(table, nv, q0, qpos, dtype), c(qvel) - (dtype(0) if v0 is None else c(v0))])
        s = (c(K) * dx[None, :]).sum(axis=1)
        u = c(u0) + dtype(sign) * s
        scale = np.abs(c(u0)) + (np.abs(c(K)) * np.abs(dx)[None, :]).sum(axis=1)
        if not all(np.isfinite(np.asarray(x, dtype=np.float64)).all() for x in ins) or not np.isfinite(u.astype(np.float64)).all():
            return np.zeros(nu, dtype=dtype), NOT_FINITE, scale
        bits = 0
        if clip:
            lo = np.where(limited != 0, c(ctrlrange)[:, 0], dtype(-np.inf))
            hi = np.where(limited != 0, c(ctrlrange)[:, 1], dtype(np.inf))
            if ((u < lo) | (u > hi)).any():
                bits = CLIPPED
            u = np.minimum(np.maximum(u, lo), hi)
    return u, bits, scale


_REF = {}


def references(key, table, nv, K, u0, q0, v0, qpos, qvel, sign, clip, limited, ctrlrange):
    """(float64 restatements, long-double restatements) of every environment of one step (K [B, nu, 2nv], ...), computed once per key
    and shared."""
    if key not in _REF:
        B = qpos.shape[0]
        one = lambda e, dt: restate(table, nv, K[e], u0[e], q0[e], None if v0 is None else v0[e], qpos[e], qvel[e], sign, clip, limited, ctrlrange, dt)
        _REF[key] = ([one(e, np.float64) for e in range(B)], [one(e, np.longdouble) for e in range(B)])
    return _REF[key]


def figure(u, truth, scale):
    L = lambda v: np.asarray(v, dtype=np.longdouble)
    sc_ = np.where(L(scale) > 0, L(scale), 1)
    return float((np.abs(L(u) - L(truth)) / sc_).max())


def judge(key, got_u, got_status, refs, label, data_f32=False, record=None):
    """``got_u [B, nu]``, ``got_status [B]`` of one step against ``refs = references(...)``: per environment the status equals the
    restatement's and the figure lies within ``bound`` of the float64 restatement's own (+ 2^-24 |truth| / scale for float32 data)."""
    f64, tr = refs
    worst = None
    for e in range(len(tr)):
        u_t, bits_t, scale = tr[e]
        u_64, bits_64, _ = f64[e]
        assert bits_64 == bits_t, (label, e, "the restatement itself must agree with the case", bits_64, bits_t)
        assert int(got_status[e]) == bits_t, (label, e, int(got_status[e]), bits_t)
        mine, np64 = figure(got_u[e], u_t, scale), figure(u_64, u_t, scale)
        b = bound(np64)
        if data_f32:
            b += float((np.abs(u_t) / np.where(scale > 0, scale, 1)).max()) * 2.0 ** -24
        if worst is None or mine / b > worst[0] / worst[2]:
            worst = (mine, np64, b)
    mine, np64, b = worst
    print(f"{label}: kernel {mine:.2e}  float64 numpy {np64:.2e}  bound {b:.2e}")
    if record:
        record(label, mine, b)
    assert mine <= b, (label, mine, np64, b)


CASES = [(name, sign, clip) for name in SHAPES for sign, clip in ((-1, 1), (1, 0))]

if __name__ == "__main__":                                        # the floor: the worst float64-restatement figure over the case list
    worst = 0.0
    for name, sign, clip in CASES:
        table, nq, nv, nu = shape(name)
        limited, ctrlrange = limits(nu)
        K, u0, q0, v0, qpos, qvel = problem(table, nq, nv, nu, 5, 3)
        for t in range(3):
            f64, tr = references((name, sign, clip, t), table, nv, K[:, t], u0[:, t], q0[:, t], v0[:, t], qpos, qvel, sign, clip, limited, ctrlrange)
            w = max(figure(f64[e][0], tr[e][0], tr[e][2]) for e in range(5))
            worst = max(worst, w)
            print(name, sign, clip, t, f"{w:.2e}", "status", [x[1] for x in tr])
    print(f"FLOOR {worst:.2e}")
