"""Equilibrium controls by inverse dynamics, for one state or a whole batch.

``steady_ctrl0(model, data, qpos0, qvel0=None)`` has the reference's signature, argument checks and exception types
(``mujoco_template/setpoints.py:10-58``): put the system at ``(qpos0, qvel0)``, ask for zero acceleration, read the
generalized force that inverse dynamics says is needed, and realise it with the actuators through the pseudo-inverse of
the actuator moment matrix.  Here the inverse dynamics AND the dense moment matrix come from one device pass
(``mjb_inverse``); the ``nu x nv`` pseudo-inverse and the conditioning guard are evaluated for all environments at once
with stacked ``numpy.linalg`` calls.  ``qpos0`` / ``qvel0`` may be single vectors (applied to every environment) or carry a
batch axis; the result is ``[nu]`` for ``batch == 1`` and ``[batch, nu]`` otherwise.  The caller's state is restored.

``steady_ctrl0_device`` is the same computation without the host: the set-point state is written through the device arrays, and
``solve_setpoint`` (``mjb_setpoint_ctrl``, a one-sided Jacobi SVD in float64, one wavefront per environment) reads ``qfrc_inverse``
and ``actuator_moment`` where ``mjb_inverse`` left them.  An ill-conditioned environment is reported in ``status``, not raised.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import mj
from .exceptions import CompatibilityError, ConfigError, TemplateError
from .state_utils import _restore_state, _snapshot_state

_RCOND_GUARD = 1e-12          # smallest / largest singular value below this = unusable moment matrix


def _checked(vec, n: int, what: str) -> np.ndarray:
    arr = np.asarray(vec, dtype=float)
    if arr.shape[-1] != n:
        raise ConfigError(f"{what} must have length model.{'nq' if what == 'qpos0' else 'nv'}")
    return arr


def _solve_for_ctrl(moment: np.ndarray, qfrc: np.ndarray) -> np.ndarray:
    """``u`` with ``u @ moment = qfrc`` in the least-squares sense, per environment: ``[B, nu, nv]``, ``[B, nv]`` -> ``[B, nu]``."""
    sv = np.linalg.svd(moment, compute_uv=False)                               # [B, min(nu, nv)]
    worst = np.where(sv.max(axis=-1) > 0, sv.min(axis=-1) / np.maximum(sv.max(axis=-1), 1e-300), 0.0)
    if sv.shape[-1] == 0 or np.any(worst < _RCOND_GUARD):
        raise TemplateError("Actuator moment matrix is singular or ill-conditioned at this state.")
    return np.einsum("bv,bvu->bu", qfrc, np.linalg.pinv(moment))


def steady_ctrl0(model: "mj.MjModel", data: "mj.MjData", qpos0: np.ndarray, qvel0: np.ndarray | None = None) -> np.ndarray:
    qpos0 = _checked(qpos0, model.nq, "qpos0")
    qvel0 = np.zeros(model.nv) if qvel0 is None else _checked(qvel0, model.nv, "qvel0")
    batch = int(getattr(data, "batch", 1))
    saved = _snapshot_state(data)
    try:
        mj.mj_resetData(model, data)
        data.qpos[...] = qpos0
        data.qvel[...] = qvel0
        mj.mj_forward(model, data)
        data.qacc[...] = 0.0
        mj.mj_inverse(model, data)                      # fills qfrc_inverse and the dense actuator moment
        if model.nu == 0:
            raise CompatibilityError("No actuators to realize inverse dynamics (nu=0).")
        qfrc = np.array(data.qfrc_inverse, dtype=float).reshape(batch, model.nv)
        moment = np.array(data.actuator_moment, dtype=float).reshape(batch, model.nu, model.nv)
        ctrl = _solve_for_ctrl(moment, qfrc)
        return ctrl[0] if batch == 1 else ctrl
    finally:
        _restore_state(data, saved)
        mj.mj_forward(model, data)


class SetpointResult(NamedTuple):
    ctrl: object      # [nb, nu] float64: the minimum-norm u of min |u @ moment - qfrc| (NaN where status != 0)
    sv: object        # [nb, min(nu, nv)] the singular values of moment, descending
    rcond: object     # [nb] smallest / largest singular value (0 for a zero matrix)
    rank: object      # [nb] int32: singular values above rcond_min x the largest
    residual: object  # [nb] max_i |(ctrl @ moment - qfrc)_i|: the force no actuator can supply (+inf where status != 0)
    status: object    # [nb] int32: 0 ok, 1 an entry not finite, 2 max_sweeps reached, 3 rcond < rcond_min (singular or ill-conditioned)
    sweeps: object    # [nb] int32 Jacobi sweeps done (the last, clean one included)
    pinv: object      # [nb, nv, nu] the pseudo-inverse of moment (NaN where status != 0), or None


def solve_setpoint(data, moment, qfrc, *, rcond_min: float = _RCOND_GUARD, max_sweeps: int | None = None, want_pinv: bool = False) -> SetpointResult:
    """``u`` with ``u @ moment = qfrc`` in the least-squares sense and of minimum norm, for ``nb`` problems in one kernel launch
    (``mjb_setpoint_ctrl``): what ``qfrc @ numpy.linalg.pinv(moment)`` behind ``numpy.linalg.svd`` gives per environment on the host.
    A one-sided (Hestenes) Jacobi SVD of ``moment'`` itself in float64 (include/mjbatch.h states it), so rows that differ by orders of
    magnitude (gear ratios) keep their relative accuracy and the conditioning guard tests the matrix's own condition number.

    ``moment [nb, nu, nv]`` or ``[nu, nv]`` (shared by all problems), ``qfrc [nb, nv]`` or ``[nv]``; ``nu <= 32``, ``nv <= 64``; torch
    tensors on the data's GPU, float32 or float64 each (float32 is widened exactly).  The leading axis may be strided: the views of
    ``sim.torch_view("actuator_moment")`` / ``("qfrc_inverse")`` and ``expand``-ed tensors are read in place; a trailing block that is
    not dense and row-major is copied once with ``.contiguous()``.

    **Failures.**  ``status`` 1: an entry is not finite; 2: ``max_sweeps`` (default 30, at most 64) sweeps all rotated something;
    3: ``rcond < rcond_min`` - the reference's "singular or ill-conditioned" ``TemplateError``, per environment.  There ``ctrl`` and
    ``pinv`` are NaN and ``residual`` is ``+inf``; ``sv``, ``rcond``, ``rank`` and ``sweeps`` hold what was reached.  No other problem
    is affected; a problem's results are bitwise the same at any position of any batch.  Enqueued on torch's current stream; nothing
    waits for the GPU and nothing is copied to the host."""
    import torch

    from .trajopt import _sim, _strided

    fn = "solve_setpoint"
    sim = _sim(data)
    dev = torch.device(f"cuda:{sim.device}")
    if not isinstance(moment, torch.Tensor) or moment.ndim not in (2, 3):
        raise ConfigError(f"{fn}: moment must be a float32 or float64 torch tensor [nb, nu, nv] or [nu, nv] on {dev}")
    if not isinstance(qfrc, torch.Tensor) or qfrc.ndim not in (1, 2):
        raise ConfigError(f"{fn}: qfrc must be a float32 or float64 torch tensor [nb, nv] or [nv] on {dev}")
    nu, nv = int(moment.shape[-2]), int(moment.shape[-1])
    if not 1 <= nu <= 32 or not 1 <= nv <= 64:
        raise ConfigError(f"{fn}: nu must lie in [1, 32] and nv in [1, 64], got moment {list(moment.shape)}")
    if max_sweeps is not None and (isinstance(max_sweeps, bool) or int(max_sweeps) != max_sweeps or not 1 <= max_sweeps <= 64):
        raise ConfigError(f"{fn}: max_sweeps must be None (30) or an integer in [1, 64]")
    if not (rcond_min >= 0) or not np.isfinite(rcond_min):
        raise ConfigError(f"{fn}: rcond_min must be finite and >= 0")
    lead = {name: int(x.shape[0]) for name, x, nd in (("moment", moment, 3), ("qfrc", qfrc, 2)) if x.ndim == nd}
    if len(set(lead.values())) > 1:
        raise ConfigError(f"{fn}: the leading sizes differ: {lead}")
    nb = next(iter(lead.values())) if lead else 1
    if nb < 1:
        raise ConfigError(f"{fn}: at least one problem is required")
    arrays, keep = {}, []
    both = (torch.float32, torch.float64)
    for name, x, trail in (("moment", moment, (nu, nv)), ("qfrc", qfrc, (nv,))):     # one step per problem: [nb, 1, *trail] views through _strided
        if x.ndim == len(trail) + 1:
            x = x.unsqueeze(1)
        p, _, es, t = _strided(fn, name, x, trail, nb, 1, dev, False, dtypes=both)
        arrays[name] = (p, 0, es, 0 if t.dtype == torch.float32 else 1); keep.append(t)
    opt = dict(dtype=torch.float64, device=dev)
    ctrl, sv = torch.empty((nb, nu), **opt), torch.empty((nb, min(nu, nv)), **opt)
    rcond, residual = torch.empty((nb,), **opt), torch.empty((nb,), **opt)
    pinv = torch.empty((nb, nv, nu), **opt) if want_pinv else None
    rank, sweeps, status = (torch.empty((nb,), dtype=torch.int32, device=dev) for _ in range(3))
    sim.setpoint_ctrl({"batch": nb, "nu": nu, "nv": nv, "max_sweeps": 0 if max_sweeps is None else int(max_sweeps), "rcond_min": float(rcond_min)},
                      arrays, {"ctrl": ctrl.data_ptr(), "sv": sv.data_ptr(), "rcond": rcond.data_ptr(), "residual": residual.data_ptr(),
                               "pinv": 0 if pinv is None else pinv.data_ptr(), "rank": rank.data_ptr(), "sweeps": sweeps.data_ptr(),
                               "status": status.data_ptr()}, keep=keep)
    return SetpointResult(ctrl, sv, rcond, rank, residual, status, sweeps, pinv)


def steady_ctrl0_device(model: "mj.MjModel", data: "mj.MjData", qpos0, qvel0=None, *, rcond_min: float = _RCOND_GUARD) -> SetpointResult:
    """``steady_ctrl0`` without the host: the controls that hold every environment at ``(qpos0, qvel0)`` with zero acceleration, as
    device tensors.  ``qpos0`` / ``qvel0`` are numpy arrays or torch tensors, ``[nq]`` / ``[nv]`` (every environment) or with a leading
    batch axis.  The state fields of ``DeviceData`` and ``time`` are saved as device clones, the set-point state is written with zero
    ``ctrl`` and ``qacc``, one forward pass and ``mjb_inverse`` run, ``solve_setpoint`` reads ``actuator_moment`` and ``qfrc_inverse``
    in place, and the state is restored and propagated again - all on torch's current stream, with no copy to the host and no wait.
    Per-environment parameters (``set_env_params``) are honoured because ``mjb_inverse`` honours them.

    Differences from ``steady_ctrl0``: the result is a ``SetpointResult`` of ``[batch, ...]`` tensors for every batch size (``ctrl``
    float64); an ill-conditioned or singular environment raises nothing - ``status`` says which ones failed, and their ``ctrl`` is NaN."""
    import torch

    from .device_data import STATE_FIELDS
    from .mj import _check

    fn = "steady_ctrl0_device"
    _check(model, data)
    if model.nu == 0:
        raise CompatibilityError("No actuators to realize inverse dynamics (nu=0).")
    sim = data.sim
    B, nq, nv, nu = int(sim.batch), int(model.nq), int(model.nv), int(model.nu)
    dev = torch.device(f"cuda:{sim.device}")
    dt = torch.float32 if sim.dtype == "float32" else torch.float64

    def state(x, n, what):
        try:
            t = x.to(device=dev, dtype=dt) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=dt).to(dev)
        except (TypeError, ValueError, RuntimeError) as exc:
            raise ConfigError(f"{fn}: {what} must be a tensor or an array: {exc}") from exc
        if tuple(t.shape) not in ((n,), (B, n)):
            raise ConfigError(f"{fn}: {what} must have length model.{'nq' if what == 'qpos0' else 'nv'} (shape [{n}] or [{B}, {n}]), got {list(t.shape)}")
        return t

    if not 1 <= nu <= 32 or not 1 <= nv <= 64:                     # before any state is written
        raise ConfigError(f"{fn}: the solver takes nu in [1, 32] and nv in [1, 64], this model has nu = {nu}, nv = {nv}")
    sim.use_torch_stream()
    q = state(qpos0, nq, "qpos0")
    v = None if qvel0 is None else state(qvel0, nv, "qvel0")
    data.push_host_edits()                                         # pending in-place edits of the host mirrors first, then the device writes
    view = {name: sim.torch_view(name) for name in STATE_FIELDS}
    time = sim.torch_view("time")
    saved = {name: t.clone() for name, t in view.items()}
    saved_time = time.clone()
    try:
        view["qpos"].copy_(q)
        if v is None:
            view["qvel"].zero_()
        else:
            view["qvel"].copy_(v)
        for name in ("ctrl", "qacc", "qacc_warmstart"):
            view[name].zero_()
        sim.forward()
        view["qacc"].zero_()                                       # the forward pass wrote its own: inverse dynamics is asked for zero
        sim.inverse()
        res = solve_setpoint(data, sim.torch_view("actuator_moment").view(B, nu, nv), sim.torch_view("qfrc_inverse"), rcond_min=rcond_min)
    finally:                                                       # whatever was raised, the caller's state comes back
        for name, t in saved.items():
            view[name].copy_(t)
        time.copy_(saved_time)
        sim.forward()
        for name in ("qacc", "qacc_warmstart"):                    # the caller's own, not this pass's
            view[name].copy_(saved[name])
        data.mark_device_newer()
    return res


__all__ = ["steady_ctrl0", "steady_ctrl0_device", "solve_setpoint", "SetpointResult"]
