"""Feedback laws from device tensors: per-environment and time-varying gains applied on the GPU.

The design chain ``set_env_params -> steady_ctrl0_device -> linearize_rollout -> solve_dare`` leaves ``ctrl0 [B, nu]``,
``K [B, nu, 2nv]`` and the set-point ``qpos0 [B, nq]`` on the device; ``lqr_backward`` leaves ``k [B, T, nu]`` and ``K [B, T, nu, 2nv]``
there.  This module applies them without a torch re-implementation of ``mj_differentiatePos`` (``mjb_feedback_law``, include/mjbatch.h)::

    dx = [ differentiatePos(q0 -> qpos, dt = 1) ; qvel - v0 ]        u = clip(u0 + feedback_sign * K dx)

* ``feedback_ctrl`` - one kernel launch that writes ``data.ctrl`` for step index ``t``;
* ``rollout_feedback`` - the closed-loop rollout: per step the law kernel, one engine step and the record, all stream-ordered;
* ``DeviceFeedbackController`` - the law as an ``Env`` controller with ``device_arrays = True``.

The arrays ``K [nu, 2nv]``, ``u0 [nu]``, ``q0 [nq]``, ``v0 [nv]`` are torch tensors on the data's GPU, float32 or float64 each, with the
leading axes ``()`` (shared), ``(B,)`` (per environment) or ``(B, T)`` (per environment and step).  A leading axis of size 1 or of stride
0 (``expand``) broadcasts and is read without a copy, any other leading stride is passed through as it is; only a trailing block that is
not dense and row-major is copied.  ``feedback_sign=-1`` is ``solve_dare``'s convention (``u = u0 - K dx``), ``+1`` ``lqr_backward``'s.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, NamedTuple

from .control import ControlSpace, ControllerCapabilities
from .exceptions import CompatibilityError, ConfigError


class FeedbackRollout(NamedTuple):
    state: object       # [B, T, 1+nq+nv]: time, qpos, qvel after each step (data's dtype)
    sensordata: object  # [B, T, nsensordata]
    control: object     # [B, T, nu]: the ctrl row each step applied - what ``rollout`` replays and ``lqr_backward`` takes as ``u``
    status: object      # [B] int32, sticky over the steps: bit 0 a value was not finite (that step's ctrl: zeros), bit 1 an actuator was clipped


def _sim(data):
    return getattr(data, "sim", data)


def _array(fn: str, name: str, x, trail: tuple, B: int, need_T: int, dev, optional: bool = False):
    """(address, step stride, env stride, dtype code, tensor kept alive) of one law input; ``need_T``: the steps an axis ``T`` must hold."""
    import torch

    if x is None:
        if optional:
            return (0, 0, 0, 1), None
        raise ConfigError(f"{fn}: {name} is required")
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.float64) or x.device != dev:
        raise ConfigError(f"{fn}: {name} must be a float32 or float64 torch tensor on {dev}")
    nt = len(trail)
    lead = tuple(x.shape[:x.ndim - nt]) if x.ndim >= nt else None
    if lead is None or tuple(x.shape[x.ndim - nt:]) != trail or len(lead) > 2 or (lead and lead[0] not in (1, B)):
        raise ConfigError(f"{fn}: {name} must have shape {list(trail)}, [{B}, ...] or [{B}, T, ...] with the trailing block {list(trail)}, got {list(x.shape)}")
    if len(lead) == 2 and lead[1] != 1 and lead[1] < need_T:
        raise ConfigError(f"{fn}: the T axis of {name} holds {lead[1]} steps, {need_T} are needed")
    dense, want = True, 1
    for size, stride in zip(reversed(trail), reversed(x.stride()[x.ndim - nt:])):      # the trailing block must be dense, row-major
        if size > 1 and stride != want:
            dense = False
        want *= size
    if x.numel() and not dense:
        x = x.contiguous()
    es = x.stride(0) if len(lead) >= 1 and lead[0] > 1 else 0
    ss = x.stride(1) if len(lead) == 2 and lead[1] > 1 else 0
    return (x.data_ptr(), ss, es, 0 if x.dtype == torch.float32 else 1), x


def _law(fn: str, data, K, u0, q0, v0, need_T: int, feedback_sign, clip, env_mask, status):
    """Checks shared by the three entry points.  Returns ``(sim, arrays, options, keep, status)``."""
    import torch

    sim = _sim(data)
    m = sim.model.compiled
    B, nq, nv, nu = int(sim.batch), int(m.nq), int(m.nv), int(m.nu)
    if nu == 0:
        raise CompatibilityError(f"{fn}: the model has no actuators (nu=0).")
    if not 1 <= nu <= 32 or not 1 <= nv <= 64:
        raise ConfigError(f"{fn}: the law kernel takes nu in [1, 32] and nv in [1, 64], this model has nu = {nu}, nv = {nv}")
    if feedback_sign not in (-1, 1):
        raise ConfigError(f"{fn}: feedback_sign must be -1 (solve_dare, set_feedback: u = u0 - K dx) or +1 (lqr_backward), got {feedback_sign!r}")
    dev = torch.device(f"cuda:{sim.device}")
    arrays, keep = {}, []
    for name, x, trail, opt in (("K", K, (nu, 2 * nv), False), ("u0", u0, (nu,), False), ("q0", q0, (nq,), False), ("v0", v0, (nv,), True)):
        arrays[name], t = _array(fn, name, x, trail, B, need_T, dev, optional=opt)
        keep.append(t)
    options = {"feedback_sign": int(feedback_sign), "clip": bool(clip)}
    if env_mask is not None:
        if not isinstance(env_mask, torch.Tensor) or env_mask.dtype not in (torch.bool, torch.uint8) or env_mask.device != dev or tuple(env_mask.shape) != (B,):
            raise ConfigError(f"{fn}: env_mask must be a bool or uint8 torch tensor [{B}] on {dev}")
        env_mask = env_mask.contiguous()
        keep.append(env_mask)
        options["env_mask"] = env_mask.data_ptr()
    if status is None:
        status = torch.zeros((B,), dtype=torch.int32, device=dev)
    elif not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or status.device != dev or tuple(status.shape) != (B,) or not status.is_contiguous():
        raise ConfigError(f"{fn}: status must be a contiguous int32 torch tensor [{B}] on {dev}")
    options["status"] = status.data_ptr()
    keep.append(status)
    return sim, arrays, options, keep, status


def feedback_ctrl(data, K, u0, q0, v0=None, *, t: int = 0, feedback_sign: int = -1, clip: bool = True, env_mask=None, status=None, out=None):
    """Write ``data.ctrl`` on the device from the current ``qpos`` / ``qvel`` and the law of step index ``t`` (one launch of
    ``mjb_feedback_law``); returns ``status [B]`` int32 (allocated and zeroed when ``None``; the kernel ORs into it: bit 0 a value of the
    environment's law or state, or a resulting control, was not finite - its ``ctrl`` is then zeros; bit 1 an actuator was clipped).

    ``data``: an ``MjData`` or a ``DeviceData``.  ``K``, ``u0``, ``q0``, ``v0`` (``None`` = zeros) as the module states; arrays with a
    ``T`` axis need ``T > t``.  ``clip=False`` leaves the controls unclipped.  ``env_mask [B]`` (bool or uint8): environments with a
    zero entry keep their ``ctrl``, ``status`` and record row - ``dare.status == 0`` feeds it directly.  ``out``: optional record in the
    data's dtype, ``[B, nu]`` or ``[B, T, nu]`` (row ``t``): the ``ctrl`` rows just written are stored there too.  An environment's
    ``ctrl`` is bitwise the same at any position of any batch and for any layout of the inputs.  Enqueued on torch's current stream;
    nothing waits for the GPU and nothing is copied to the host."""
    import torch

    fn = "feedback_ctrl"
    if isinstance(t, bool) or int(t) != t or t < 0:
        raise ConfigError(f"{fn}: t must be an integer >= 0, got {t!r}")
    t = int(t)
    sim, arrays, options, keep, status = _law(fn, data, K, u0, q0, v0, t + 1, feedback_sign, clip, env_mask, status)
    if out is not None:
        B, nu = int(sim.batch), int(sim.model.compiled.nu)
        want = torch.float32 if sim.dtype == "float32" else torch.float64
        ok = isinstance(out, torch.Tensor) and out.dtype == want and out.device == status.device and out.ndim in (2, 3) and \
            out.shape[0] == B and out.shape[-1] == nu and (nu == 1 or out.stride(-1) == 1)
        if not ok or (out.ndim == 3 and out.shape[1] <= t):
            raise ConfigError(f"{fn}: out must be a {want} torch tensor [{B}, {nu}] or [{B}, T, {nu}] with T > t and a dense last axis on {status.device}")
        options.update(u_rec=out.data_ptr(), u_rec_env_stride=out.stride(0), u_rec_step_stride=out.stride(1) if out.ndim == 3 else 0)
        keep.append(out)
    push = getattr(data, "push_host_edits", None)
    if push is not None:                                           # an MjData: pending in-place edits of the host mirrors first
        push()
    sim.feedback_law(arrays, options, t, keep=keep)
    mark = getattr(data, "mark_device_newer", None)
    if mark is not None:
        mark()
    return status


def rollout_feedback(model, data, K, u0, q0, v0=None, *, nstep: int, initial_state=None, initial_warmstart=None, feedback_sign: int = -1,
                     clip: bool = True, env_mask=None) -> FeedbackRollout:
    """Roll every environment of ``data`` forward ``nstep`` steps in closed loop: step ``t`` applies
    ``u_t = clip(u0_t + feedback_sign * K_t dx_t)`` with ``dx_t`` taken from the state before the step (``mjb_rollout_feedback``: per
    step the law kernel, what ``step(1)`` enqueues and the record, stream-ordered - no synchronisation, no host read between steps).

    ``K``, ``u0``, ``q0``, ``v0`` as the module states; arrays with a ``T`` axis need ``T >= nstep``.  ``initial_state`` and
    ``initial_warmstart`` as for ``rollout``: ``qacc_warmstart`` starts from ZERO unless given.  Environments with a zero ``env_mask``
    entry run open-loop on the ``ctrl`` they hold (their ``control`` rows say so).  Returns ``FeedbackRollout``: ``state`` and
    ``sensordata`` as ``rollout`` returns them, ``control [B, T, nu]`` - replayed through ``rollout`` from the same start it reproduces
    ``state`` bitwise - and the sticky ``status [B]``.  For the closed-loop forward pass of iLQR pass ``u0 = ubar + alpha * k``,
    ``q0`` / ``v0`` from the nominal states BEFORE each step and ``feedback_sign=+1``.  Nothing waits for the GPU."""
    import torch

    from .rollout import _front, _results

    fn = "rollout_feedback"
    if isinstance(nstep, bool) or nstep is None or int(nstep) != nstep or nstep < 1:
        raise ConfigError(f"{fn}: nstep must be an integer >= 1, got {nstep!r}")
    nstep = int(nstep)
    sim, arrays, options, keep, status = _law(fn, data, K, u0, q0, v0, nstep, feedback_sign, clip, env_mask, None)
    _, ring, spec, nstep, time_col = _front(fn, model, data, None, initial_state, initial_warmstart, nstep, False, False)
    m = sim.model.compiled
    B, nu = int(sim.batch), int(m.nu)
    ctrl = sim.torch_view("ctrl")
    if env_mask is None:
        control = torch.empty((B, nstep, nu), dtype=ctrl.dtype, device=ctrl.device)
    else:                                                           # a masked environment runs on the ctrl it holds: its rows say so
        control = ctrl.unsqueeze(1).repeat(1, nstep, 1)
    options.update(u_rec=control.data_ptr(), u_rec_step_stride=nu, u_rec_env_stride=nstep * nu)
    sim.rollout_feedback(arrays, options, nstep, obs_spec=spec, obs_out_ptr=ring.data_ptr(), obs_every=1, keep=keep + [control, ring])
    data.mark_device_newer()
    state, sens = _results(ring, time_col, 1 + m.nq + m.nv)
    return FeedbackRollout(state, sens, control, status)


@dataclass
class DeviceFeedbackController:
    """``ctrl = clip(ctrl0 + feedback_sign * K [q (-) qpos_goal ; qvel - qvel_goal])`` with device tensors that may differ per
    environment and per step - the law of ``LinearFeedbackController`` after a per-environment design, for ``Env.step``
    (``device_arrays = True``: called with ``DeviceData``, one ``mjb_feedback_law`` launch per control period, nothing on the host).
    The controller counts its own calls since ``prepare``: call ``n`` applies block ``n`` of arrays with a ``T`` axis.  ``status [B]``
    (int32, sticky; zeroed by ``prepare``) reports what ``feedback_ctrl`` reports."""

    K: Any = None                # [nu, 2nv], [B, nu, 2nv] or [B, T, nu, 2nv]
    ctrl0: Any = None            # [nu], [B, nu] or [B, T, nu]
    qpos_goal: Any = None        # [nq], [B, nq] or [B, T, nq]
    qvel_goal: Any = None        # None = zeros
    feedback_sign: int = -1
    env_mask: Any = None
    clip: bool = True
    capabilities: ControllerCapabilities = ControllerCapabilities(control_space=ControlSpace.TORQUE)
    device_arrays: bool = True
    step_count: int = field(default=0)
    status: Any = None

    def prepare(self, model: Any, data: Any) -> None:
        if model.nu == 0:
            raise CompatibilityError("DeviceFeedbackController requires nu>0.")
        self.step_count = 0
        self.status = None

    def __call__(self, model: Any, data: Any, t: Any) -> None:
        self.status = feedback_ctrl(data, self.K, self.ctrl0, self.qpos_goal, self.qvel_goal, t=self.step_count, feedback_sign=self.feedback_sign,
                                    clip=self.clip, env_mask=self.env_mask, status=self.status)
        self.step_count += 1


__all__ = ["feedback_ctrl", "rollout_feedback", "FeedbackRollout", "DeviceFeedbackController"]
