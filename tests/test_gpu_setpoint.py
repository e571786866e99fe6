"""``mjb_setpoint_ctrl`` on the GPU (``mt.solve_setpoint``, ``mt.steady_ctrl0_device``).

The yardstick is never the kernel: the numpy restatement of ``tests/setpoint_common.py`` in long double is the truth, the same
restatement in float64 measures what float64 arithmetic alone loses, and every bound is 8 x that measure with the floors written
there.  Both values of every comparison go through ``tests.conftest.measured`` under ``setpoint/...``."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import setpoint_common as sc
from tests.conftest import MODELS, measured

pytestmark = pytest.mark.gpu

NB = 5


@pytest.fixture(scope="module")
def ctx():
    import torch

    from mujoco_template_amd import mj

    model = mj.MjModel.from_xml_path(MODELS["cartpole"])
    data = mj.MjData(model, batch=1, dtype="float64")
    return torch, model, data


def _dev(torch, x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype or torch.float64, device="cuda")


def _np(res):
    return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in sc.OUTPUTS}


def _record(key, value, tol):
    measured(key, value, tol, "(8 x the float64 numpy restatement's own figure, with the floor)")


def _solve(torch, data, m, q, dtype=None, **kw):
    import mujoco_template_amd as mt

    return _np(mt.solve_setpoint(data, _dev(torch, m, dtype), _dev(torch, q, dtype), want_pinv=True, **kw))


# ---- 1. the restatement cases, five distinct problems per launch ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("layout", ["dense", "strided", "shared_moment"])
@pytest.mark.parametrize("name,make,kw,status", sc.CASES, ids=[c[0] for c in sc.CASES])
def test_jacobi_solve_matches_the_restatement(ctx, name, make, kw, status, layout, dtype):
    """dense: moment [5, nu, nv], qfrc [5, nv].  strided: both as non-contiguous leading-axis views (every second block of a NaN-filled
    [10, ...] tensor), read in place.  shared_moment: the first problem's moment passed once as [nu, nv] against the five qfrc.
    float32: the case's values rounded to float32 and passed as float32 tensors; the restatement works on those rounded values."""
    import mujoco_template_amd as mt

    torch, _, data = ctx
    m, q = sc.problems(name, make, NB)
    tdt = torch.float32 if dtype == "float32" else torch.float64
    key = f"{name}/{NB}"
    if dtype == "float32":
        m, q = m.astype(np.float32).astype(np.float64), q.astype(np.float32).astype(np.float64)
        key += "/f32"
    nu, nv = m.shape[1:]
    if layout == "dense":
        got = _solve(torch, data, m, q, tdt, **kw)
    elif layout == "strided":
        wide = []
        for x in (m, q):
            w = torch.full((2 * NB,) + x.shape[1:], float("nan"), dtype=tdt, device="cuda")
            w[::2] = _dev(torch, x, tdt)
            wide.append(w[::2])
            assert not wide[-1].is_contiguous()
        res = mt.solve_setpoint(data, wide[0], wide[1], want_pinv=True, **kw)
        assert res.ctrl.shape == (NB, nu) and res.sv.shape == (NB, min(nu, nv)) and res.pinv.shape == (NB, nv, nu) and res.status.shape == (NB,)
        assert res.ctrl.dtype == torch.float64 and res.status.dtype == torch.int32
        got = _np(res)
    else:
        m = np.broadcast_to(m[0], m.shape).copy()
        key += "/shared"
        got = _np(mt.solve_setpoint(data, _dev(torch, m[0], tdt), _dev(torch, q, tdt), want_pinv=True, **kw))
    sc.judge(key, m, q, got, f"setpoint/{layout}/{dtype}/{name}", record=_record, expect=status, **kw)
    if name == "selection21x27" and layout != "shared_moment":
        assert got["sweeps"].tolist() == [1] * NB                  # orthogonal rows: the first sweep finds nothing to rotate
        assert np.array_equal(got["residual"], np.abs(q[:, :6]).max(axis=1))   # the root part of qfrc, which no actuator reaches


def test_float32_inputs_are_widened_exactly(ctx):
    torch, _, data = ctx
    m, q = sc.gaussian(21, 27, NB, seed=11)
    m32, q32 = m.astype(np.float32), q.astype(np.float32)
    narrow, wide = _solve(torch, data, m32, q32, torch.float32), _solve(torch, data, m32.astype(np.float64), q32.astype(np.float64))
    import mujoco_template_amd as mt

    mixed = _np(mt.solve_setpoint(data, _dev(torch, m32, torch.float32), _dev(torch, q32, torch.float64), want_pinv=True))   # each input has its own dtype
    for key in sc.OUTPUTS:
        assert np.array_equal(narrow[key], wide[key]) and np.array_equal(mixed[key], wide[key]), key
    assert narrow["status"].tolist() == [0] * NB


# ---- 2. statuses and isolation ----------------------------------------------------------------------------------------------------------
def test_failures_are_reported_not_propagated(ctx):
    torch, _, data = ctx
    sc.check_statuses(lambda m, q, **kw: _solve(torch, data, m, q, **kw), "gpu")


def test_results_do_not_depend_on_the_position_in_the_batch(ctx):
    """One problem alone, at index 3 of a batch of 5 and at index 129 of a batch of 130 (other workgroups, other compute units):
    bitwise the same outputs."""
    torch, _, data = ctx
    m, q = sc.gaussian(21, 27, 130, seed=21)
    pm, pq = sc.gaussian(21, 27, 1, seed=22)
    alone = _solve(torch, data, pm, pq)
    assert alone["status"].tolist() == [0]
    for n, at in ((5, 3), (130, 129)):
        mm, qq = m[:n].copy(), q[:n].copy()
        mm[at], qq[at] = pm[0], pq[0]
        got = _solve(torch, data, mm, qq)
        for key in sc.OUTPUTS:
            assert np.array_equal(got[key][at], alone[key][0]), (n, at, key)


# ---- 3. argument checks -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_leave_the_outputs_alone(ctx):
    import mujoco_template_amd as mt
    from mujoco_template_amd.exceptions import ConfigError, TemplateError
    from tests.test_gpu_rollout_ctrl import _hip_runtime

    torch, _, data = ctx
    m, q = sc.gaussian(4, 6, 3, seed=31)
    M, Q = _dev(torch, m), _dev(torch, q)
    for call in (lambda: mt.solve_setpoint(data, M.half(), Q),                                  # wrong dtype
                 lambda: mt.solve_setpoint(data, M.cpu(), Q),                                   # a CPU tensor
                 lambda: mt.solve_setpoint(data, M[:2], Q),                                     # mismatched nb
                 lambda: mt.solve_setpoint(data, M, Q[:, :5]),                                  # qfrc not [nv]
                 lambda: mt.solve_setpoint(data, torch.zeros((33, 6), dtype=torch.float64, device="cuda"), Q),
                 lambda: mt.solve_setpoint(data, torch.zeros((4, 65), dtype=torch.float64, device="cuda"), torch.zeros(65, dtype=torch.float64, device="cuda")),
                 lambda: mt.solve_setpoint(data, M, Q, max_sweeps=0), lambda: mt.solve_setpoint(data, M, Q, max_sweeps=65),
                 lambda: mt.solve_setpoint(data, M, Q, rcond_min=-1.0), lambda: mt.solve_setpoint(data, M, Q, rcond_min=float("nan"))):
        with pytest.raises(ConfigError):
            call()
    # the C entry point itself: rejected before anything is launched, the outputs keep their contents
    f = lambda *s: torch.full(s, -77.0, dtype=torch.float64, device="cuda")
    i = lambda: torch.full((3,), -77, dtype=torch.int32, device="cuda")
    outs = {"ctrl": f(3, 4), "sv": f(3, 4), "rcond": f(3), "residual": f(3), "pinv": f(3, 6, 4), "rank": i(), "sweeps": i(), "status": i()}
    ptrs = {k: v.data_ptr() for k, v in outs.items()}
    arrays = {"moment": (M.data_ptr(), 0, 24, 1), "qfrc": (Q.data_ptr(), 0, 6, 1)}
    good = {"batch": 3, "nu": 4, "nv": 6, "max_sweeps": 0, "rcond_min": 1e-12}
    host = np.zeros(64)
    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    assert _hip_runtime().hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(M.data_ptr())) == 0
    short = base.value + size.value - 8 * 72 + 8                 # a moment block that ends one element past its allocation
    bad = [("nu must lie", dict(sizes={**good, "nu": 33})), ("nv must lie", dict(sizes={**good, "nv": 65})), ("nu must lie", dict(sizes={**good, "nu": 0})),
           ("batch must be", dict(sizes={**good, "batch": 0})), ("max_sweeps must be", dict(sizes={**good, "max_sweeps": 65})),
           ("rcond_min must be", dict(sizes={**good, "rcond_min": -1.0})), ("rcond_min must be", dict(sizes={**good, "rcond_min": float("inf")})),
           ("strides must be", dict(arrays={**arrays, "moment": (M.data_ptr(), 0, -24, 1)})),
           ("strides must be", dict(arrays={**arrays, "qfrc": (Q.data_ptr(), 0, -6, 1)})),
           ("not device-accessible", dict(arrays={**arrays, "qfrc": (host.ctypes.data, 0, 6, 1)})),
           ("beyond its allocation", dict(arrays={**arrays, "moment": (short, 0, 24, 1)})),
           ("dtype", dict(arrays={**arrays, "moment": (M.data_ptr(), 0, 24, 2)})),
           ("moment is NULL", dict(arrays={**arrays, "moment": (0, 0, 24, 1)})), ("status is NULL", dict(ptrs={**ptrs, "status": 0})),
           ("ctrl is NULL", dict(ptrs={**ptrs, "ctrl": 0})), ("beyond its allocation", dict(sizes={**good, "batch": 1 << 24}))]
    for msg, kw in bad:
        with pytest.raises((ConfigError, TemplateError), match=msg):
            data.sim.setpoint_ctrl(kw.get("sizes", good), kw.get("arrays", arrays), kw.get("ptrs", ptrs))
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == -77).all()), k
    data.sim.setpoint_ctrl(good, {**arrays, "moment": (short - 8, 0, 24, 1)}, ptrs)   # ending exactly at the end of the block: accepted
    torch.cuda.synchronize()
    assert bool((outs["status"] != -77).all())                   # whatever lies there was solved or refused per problem
    outs["pinv"].fill_(-77.0)
    data.sim.setpoint_ctrl(good, arrays, {**ptrs, "pinv": 0})                      # and the same call, well-formed, runs; pinv is optional
    torch.cuda.synchronize()
    assert outs["status"].tolist() == [0, 0, 0] and bool((outs["pinv"] == -77).all()) and bool(torch.isfinite(outs["ctrl"]).all())


# ---- 4. end to end: the device form of steady_ctrl0 -----------------------------------------------------------------------------------
def _host_operands(mj, model, data, qpos0):
    """moment [B, nu, nv] and qfrc [B, nv] of the set-point through the host interface (what steady_ctrl0 solves), state restored."""
    from mujoco_template_amd.state_utils import _restore_state, _snapshot_state

    saved = _snapshot_state(data)
    mj.mj_resetData(model, data)
    data.qpos[...] = qpos0
    data.qvel[...] = 0.0
    mj.mj_forward(model, data)
    data.qacc[...] = 0.0
    mj.mj_inverse(model, data)
    B = data.batch
    out = np.array(data.actuator_moment, dtype=float).reshape(B, model.nu, model.nv), np.array(data.qfrc_inverse, dtype=float).reshape(B, model.nv)
    _restore_state(data, saved)
    mj.mj_forward(model, data)
    return out


def _ctrl_figure(u, tr):
    L = lambda v: np.asarray(v, dtype=np.longdouble)
    return float(np.abs(L(u) - L(tr["ctrl"])).max() / np.abs(L(tr["ctrl"])).max() * L(tr["rcond"]))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_humanoid_setpoints_under_randomised_mass(dtype):
    """models/humanoid.xml at its first keyframe, batch 4, body_mass scaled per environment by 0.8, 1.0, 1.2, 1.5.  The device path
    and the host steady_ctrl0 solve the same operands (downloaded here through the host interface).  Against the long-double
    restatement on those operands the device ctrl is within the bound of solve_setpoint, and device and host agree with each other
    within that same bound (the host's own distance from the truth is printed, not allowed for).  The four rows differ; the state
    fields and time are bitwise what they were."""
    import torch

    import mujoco_template_amd as mt
    from mujoco_template_amd import mj

    B = 4
    model = mj.MjModel.from_xml_path(MODELS["humanoid"])
    data = mj.MjData(model, batch=B, dtype=dtype, specialize=False)      # no per-model kernel is compiled for a set-point
    cm = data.sim.model.compiled
    mass = np.asarray(cm.body_mass, dtype=np.float64)[None] * np.array([0.8, 1.0, 1.2, 1.5])[:, None]
    data.sim.set_env_params(body_mass=mass)
    qpos0 = np.array(cm.arrays["key_qpos"]).reshape(-1, model.nq)[0]
    mj.mj_resetDataKeyframe(model, data, 1)                        # some other state with a clock that is not zero
    mj.mj_step(model, data, 3)
    dd = mt.DeviceData(data)
    fields = ("qpos", "qvel", "ctrl", "qacc", "qacc_warmstart", "time")
    before = {k: getattr(dd, k).clone() for k in fields}
    res = mt.steady_ctrl0_device(model, data, qpos0)
    assert res.ctrl.shape == (B, model.nu) and res.ctrl.dtype == torch.float64 and res.pinv is None
    for k in fields:
        assert torch.equal(getattr(dd, k), before[k]), k
    assert res.status.tolist() == [0] * B and res.rank.tolist() == [model.nu] * B
    host = np.atleast_2d(mt.steady_ctrl0(model, data, qpos0))      # (the host form ends with a forward pass that rewrites qacc)
    again =mt.steady_ctrl0_device(model, data, torch.as_tensor(qpos0, device="cuda").expand(B, -1), np.zeros(model.nv))
    assert torch.equal(again.ctrl, res.ctrl)                       # tensors with a batch axis and an explicit qvel0: the same set-point
    m, q = _host_operands(mj, model, data, qpos0)
    u = res.ctrl.cpu().numpy()
    for e in range(B):
        f64, tr = sc.restate(m[e], q[e], np.float64), sc.restate(m[e], q[e], np.longdouble)
        mine, np64, lapack = _ctrl_figure(u[e], tr), _ctrl_figure(f64["ctrl"], tr), _ctrl_figure(host[e], tr)
        print(f"humanoid {dtype} [{e}] ctrl: kernel {mine:.2e}  float64 numpy {np64:.2e}  host pinv {lapack:.2e}  rcond {float(tr['rcond']):.2e}")
        measured(f"setpoint/humanoid/{dtype}/ctrl_{e}", mine, sc.bound(np64, "ctrl"), "(8 x the float64 restatement's own figure, with the floor)")
        agree = float(np.abs(u[e] - host[e]).max() / np.abs(host[e]).max() * float(tr["rcond"]))
        measured(f"setpoint/humanoid/{dtype}/device_vs_host_{e}", agree, sc.bound(np64, "ctrl"), "(8 x the float64 restatement's own figure, with the floor)")
    for a in range(B):
        for b in range(a + 1, B):
            assert not np.array_equal(u[a], u[b]), (a, b)


def test_drone_hover_thrust_under_randomised_mass():
    """models/drone2/scene.xml at its hover keyframe, batch 4, float64, every body's mass scaled per environment.  Status 0; the
    residual is at the level of the host path's |ctrl0 @ moment - qfrc0| (both are rounding: within the residual bound of the
    restatement); and the realised vertical force (ctrl @ moment)[z] is each environment's weight, sum(body_mass_e) * |g| - a figure
    of the model.  The hovering drone is at rest, so inverse dynamics adds the weights of its bodies and nothing else: a handful of
    float64 roundings per body, allowed for as 64 eps relative, plus the residual bound on the realised force itself."""
    import torch

    import mujoco_template_amd as mt
    from mujoco_template_amd import mj

    B = 4
    model = mj.MjModel.from_xml_path(MODELS["drone2"])
    data = mj.MjData(model, batch=B, dtype="float64", specialize=False)
    cm = data.sim.model.compiled
    scale = np.random.default_rng(41).uniform(0.7, 1.4, size=B)
    mass = np.asarray(cm.body_mass, dtype=np.float64)[None] * scale[:, None]
    data.sim.set_env_params(body_mass=mass)
    qpos0 = np.array(cm.arrays["key_qpos"]).reshape(-1, model.nq)[0]
    res = mt.steady_ctrl0_device(model, data, qpos0)
    assert res.status.tolist() == [0] * B
    dd = mt.DeviceData(data)                                       # a call that fails after the state was written puts the state back
    fields = ("qpos", "qvel", "ctrl", "qacc", "qacc_warmstart", "time")
    before = {k: getattr(dd, k).clone() for k in fields}
    with pytest.raises(mt.ConfigError):
        mt.steady_ctrl0_device(model, data, qpos0 + 0.25, rcond_min=-1.0)
    for k in fields:
        assert torch.equal(getattr(dd, k), before[k]), k
    m, q = _host_operands(mj, model, data, qpos0)
    host = np.atleast_2d(mt.steady_ctrl0(model, data, qpos0))
    u, resid = res.ctrl.cpu().numpy(), res.residual.cpu().numpy()
    weight = mass.sum(axis=1) * abs(float(cm.gravity[2]))
    for e in range(B):
        f64, tr = sc.restate(m[e], q[e], np.float64), sc.restate(m[e], q[e], np.longdouble)
        terms = float((np.abs(q[e]) + np.abs(u[e]) @ np.abs(m[e])).max())
        r64 = float(abs(np.longdouble(f64["residual"]) - tr["residual"])) / terms
        host_resid = float(np.abs(host[e] @ m[e] - q[e]).max())
        print(f"drone [{e}] residual: kernel {resid[e]:.2e}  host path {host_resid:.2e}  terms {terms:.2e}")
        measured(f"setpoint/drone/residual_{e}", abs(resid[e] - float(tr["residual"])) / terms, sc.bound(r64, "residual"), "(the residual bound)")
        measured(f"setpoint/drone/residual_vs_host_{e}", abs(resid[e] - host_resid) / terms, sc.bound(r64, "residual") + 64 * 2.0 ** -52,
                 "(the residual bound + the host sum's own rounding)")
        fz = float((u[e] @ m[e])[2])
        assert abs(q[e][2] - weight[e]) <= 64 * 2.0 ** -52 * weight[e], (e, q[e][2], weight[e])
        measured(f"setpoint/drone/thrust_{e}", abs(fz - q[e][2]) / terms, sc.bound(r64, "residual"), "(the residual bound on the realised force)")
        measured(f"setpoint/drone/thrust_vs_weight_{e}", abs(fz - weight[e]) / weight[e], sc.bound(r64, "residual") * terms / weight[e] + 64 * 2.0 ** -52,
                 "(the residual bound + 64 eps for inverse dynamics)")
    assert len({float(x) for x in u[:, 0]}) == B                   # every environment hovers on its own thrust
