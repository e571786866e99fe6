"""``rollout`` - many open-loop trajectories in one kernel launch, the counterpart of ``mujoco.rollout.rollout``.

Sampling planners (predictive sampling, MPPI, CEM) and shooting trajectory optimisers evaluate known control sequences from given start
states and read back the state trajectories.  ``rollout`` runs them as ONE launch of the step kernel (``mjb_rollout_ctrl``): every
environment of ``data`` reads its control row of each step from a device tensor and records its state after each step into a ring on the
GPU; nothing crosses PCIe and there is no launch per step.

State layout: MuJoCo's full-physics state for models without actuator activations (``na = 0``): ``[time, qpos, qvel]``, width
``1 + nq + nv``.
"""

from __future__ import annotations

from typing import Any

from ._capi import CTRL_KEEP
from .exceptions import ConfigError
from .mj import MjData, MjModel, _check

# obs flags of the ring (ObsSpecDev::flags): the kernel writes qpos, qvel, sensordata, time in this order
_RING_FLAGS = 1 | 2 | 8 | 16
_RING_WARMSTART = 128       # + qacc_warmstart after the step, behind the time column


def _tensor(x: Any, dev, dtype, what: str):
    import torch

    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype)
    try:
        return torch.as_tensor(x, dtype=dtype).to(dev)
    except (TypeError, ValueError, RuntimeError) as exc:
        raise ConfigError(f"rollout: {what} must be a tensor or an array: {exc}") from exc


def _launch(fn: str, model: MjModel, data: MjData, control, initial_state, initial_warmstart, nstep, warmstart: bool, lead_row: bool):
    """The shared front of ``rollout`` and ``linearize_rollout``: checks, the start state written through the device arrays, one
    launch recording the ring.  Returns ``(buf, nstep, time_col)``: ``buf [nstep (+ 1), B, dim]`` with ring row ``t`` (the state after
    step ``t``: qpos | qvel | sensordata | time [| qacc_warmstart]) at ``buf[t + lead_row]``; with ``lead_row`` the columns qpos, qvel
    and qacc_warmstart of ``buf[0]`` hold the start state, so that ``buf[t]`` is the state BEFORE step ``t`` for every ``t``."""
    buf, ring, spec, nstep, time_col = _front(fn, model, data, control, initial_state, initial_warmstart, nstep, warmstart, lead_row)
    sim = data.sim
    if control is None:
        sim.rollout(nstep, CTRL_KEEP, obs_spec=spec, obs_out_ptr=ring.data_ptr(), obs_every=1)
    else:
        sim.rollout_ctrl(nstep, control, obs_spec=spec, obs_out_ptr=ring.data_ptr(), obs_every=1)
    data.mark_device_newer()
    return buf, nstep, time_col


def _front(fn: str, model: MjModel, data: MjData, control, initial_state, initial_warmstart, nstep, warmstart: bool, lead_row: bool):
    """Everything of ``_launch`` before the launch (also the front of ``feedback.rollout_feedback``): the checks, the start state and
    warm start written through the device arrays, the ring and its obs spec.  Returns ``(buf, ring, spec, nstep, time_col)``."""
    import torch

    _check(model, data)
    sim = data.sim
    m = sim.model.compiled
    B, nq, nv, nu = sim.batch, m.nq, m.nv, m.nu
    nx = 1 + nq + nv
    dev = torch.device(f"cuda:{sim.device}")
    dt = torch.float32 if sim.dtype == "float32" else torch.float64
    if control is None:
        if nstep is None or int(nstep) < 1:
            raise ConfigError(f"{fn}: without control, nstep must be given and >= 1")
        nstep = int(nstep)
    else:
        if not isinstance(control, torch.Tensor) or control.ndim not in (2, 3):
            raise ConfigError(f"{fn}: control must be a torch tensor [B, T, {nu}] or [T, {nu}]")
        T = int(control.shape[-2])
        nstep = T if nstep is None else int(nstep)
        if nstep < 1 or nstep > T:
            raise ConfigError(f"{fn}: nstep must lie in [1, {T}] (the control's steps), got {nstep}")

    sim.use_torch_stream()
    data.push_host_edits()                                      # pending in-place edits of the host mirrors first, then the device writes
    if initial_state is not None:
        s = _tensor(initial_state, dev, torch.float64, "initial_state")
        if s.shape not in ((nx,), (B, nx)):
            raise ConfigError(f"{fn}: initial_state must have shape [{nx}] or [{B}, {nx}] (time, qpos, qvel), got {list(s.shape)}")
        sim.torch_view("time")[:, 0].copy_(s[..., 0])
        sim.torch_view("qpos").copy_(s[..., 1:1 + nq])
        sim.torch_view("qvel").copy_(s[..., 1 + nq:])
    ws = sim.torch_view("qacc_warmstart")
    if initial_warmstart is None:
        ws.zero_()
    else:
        w = _tensor(initial_warmstart, dev, dt, "initial_warmstart")
        if w.shape != (B, nv):
            raise ConfigError(f"{fn}: initial_warmstart must have shape [{B}, {nv}], got {list(w.shape)}")
        ws.copy_(w)

    flags = _RING_FLAGS | (_RING_WARMSTART if warmstart else 0)
    specs = data.__dict__.get("_rollout_ring")                 # obs spec of the ring per flag word, per data object
    if specs is None:
        specs = {}
        object.__setattr__(data, "_rollout_ring", specs)
    spec = specs.get(flags)
    if spec is None:
        spec = specs[flags] = sim.make_obs_spec(flags)
    time_col = nq + nv + m.nsensordata
    buf = torch.empty((nstep + int(lead_row), B, spec.dim), device=dev, dtype=dt)
    if lead_row:
        buf[0, :, :nq].copy_(sim.torch_view("qpos"))
        buf[0, :, nq:nq + nv].copy_(sim.torch_view("qvel"))
        buf[0, :, time_col + 1:].copy_(ws)
    ring = buf[1:] if lead_row else buf
    return buf, ring, spec, nstep, time_col


def _results(ring, time_col: int, nx: int):
    """ring rows qpos | qvel | sensordata | time [| ...]  ->  [B, T, time | qpos | qvel | sensordata] in one gather"""
    import torch

    perm = torch.cat([torch.arange(time_col, time_col + 1, device=ring.device), torch.arange(time_col, device=ring.device)])   # built on the device: no host copy, nothing waits
    out = ring.permute(1, 0, 2).index_select(2, perm)
    return out[..., :nx], out[..., nx:]


def rollout(model: MjModel, data: MjData, control=None, *, initial_state=None, initial_warmstart=None, nstep: int | None = None,
            return_warmstart: bool = False):
    """Roll every environment of ``data`` forward open-loop and return ``(state [B, T, 1+nq+nv], sensordata [B, T, nsensordata])``.

    ``control``: torch tensor on the data's GPU in the data's dtype, ``[B, T, nu]`` (one sequence per environment) or ``[T, nu]`` (the
    same sequence for all; an ``expand``-ed tensor broadcasts without a copy); step ``t`` applies row ``t``.  ``control=None`` runs
    ``nstep`` steps on the current ``data.ctrl``.  ``nstep`` defaults to ``T`` and may be smaller.

    ``initial_state``: ``[B, 1+nq+nv]`` or ``[1+nq+nv]`` (broadcast) in the order time, qpos, qvel; ``None`` starts from the data's
    current state.  It is written through the device arrays (``time`` in float64).  ``qacc_warmstart`` (the solver's starting point) is
    set to ``initial_warmstart [B, nv]`` when given and to ZERO otherwise - also without ``initial_state`` - so that a rollout depends on
    the state it starts from and on nothing left over from earlier steps.

    Row ``t`` of the result is the state after step ``t`` and the sensors of that step's forward pass (MuJoCo's order).  Both
    results are torch tensors on the GPU in the data's dtype, views of one ``[B, T, 1+nq+nv+nsensordata]`` tensor; the time column is
    rounded to that dtype (``data.time`` itself stays float64).  The kernel records into a ``[T, B, dim]`` ring, and building the
    ``[B, T, ...]`` results from it costs one extra device copy.  ``data`` ends in the final state, ``data.ctrl`` holding the last
    applied control.  Everything is queued on torch's current stream; nothing waits for the GPU.

    ``return_warmstart=True`` adds a third result ``[B, T, nv]``: ``qacc_warmstart`` AFTER each step (the value ``data`` would hold had
    the rollout ended there; a view of the ring) - with the state, everything a per-step linearisation starts from.
    """
    ring, nstep, time_col = _launch("rollout", model, data, control, initial_state, initial_warmstart, nstep, bool(return_warmstart), False)
    m = data.sim.model.compiled
    state, sens = _results(ring, time_col, 1 + m.nq + m.nv)
    if return_warmstart:
        return state, sens, ring[..., time_col + 1:].permute(1, 0, 2)
    return state, sens


def linearize_rollout(model: MjModel, data: MjData, control=None, *, initial_state=None, initial_warmstart=None, nstep: int | None = None,
                      eps: float = 1e-6, centered: bool = True, sensor_derivatives: bool = False):
    """``rollout`` plus the finite-difference transition matrices along the trajectory: ``(state, sensordata, A, B)`` with
    ``A [B, T, 2nv, 2nv]`` and ``B [B, T, 2nv, nu]`` float64 on the GPU.  ``(A[:, t], B[:, t])`` linearise step ``t``: they are taken
    at the state, the solver warm start and the control the rollout had BEFORE step ``t`` (``t = 0``: the initial ones) - identical to
    the host loop ``for t: ctrl <- u[:, t]; (A_t, B_t) <- transition_fd(); step(1)`` from the same state and warm start.

    Two submissions and no host round trip: the rollout launch records qpos | qvel | ... | qacc_warmstart into its ring, and
    ``mjb_transition_fd_points`` reads the ``T x B`` points from that ring and from ``control`` in place (strided views, no staging
    copy) and writes ``[T, B, ...]`` blocks, of which ``A`` and ``B`` are permuted views.  Arguments as for ``rollout``.  Nothing waits
    for the GPU (except the first call and a call with more points per slab than any before, which allocate the FD scratch).  The
    second submission is checked after the first has been enqueued: should it fail (device allocation of the scratch or the result
    blocks), ``data`` is left in the rollout's final state and the exception is raised without (A, B).

    ``sensor_derivatives=True`` returns ``(state, sensordata, A, B, C, D)`` with the sensor Jacobians ``C [B, T, ns, 2nv]`` and
    ``D [B, T, ns, nu]`` (``ns = nsensordata``; permuted views like ``A`` and ``B``, from ``mjb_transition_fd_points_sensors``):
    ``C[:, t]`` and ``D[:, t]`` are the derivatives of ``sensordata[:, t]`` - the sensors of step ``t``'s forward pass - with respect to
    the state before step ``t`` and its control, taken at the same point, warm start and control as ``(A[:, t], B[:, t])``.  The other
    four results are bitwise those of the call without the flag."""
    import torch

    buf, nstep, time_col = _launch("linearize_rollout", model, data, control, initial_state, initial_warmstart, nstep, True, True)
    sim = data.sim
    m = sim.model.compiled
    B, nq, nv, nu = sim.batch, m.nq, m.nv, m.nu
    pre = buf[:nstep]                                            # row t: the state before step t
    if control is None:
        u = sim.torch_view("ctrl").unsqueeze(0).expand(nstep, B, nu)          # CTRL_KEEP leaves data.ctrl as it is
    elif control.ndim == 2:
        u = control[:nstep].unsqueeze(1).expand(nstep, B, nu)
    else:
        u = control.permute(1, 0, 2)[:nstep]
    mats = sim.transition_fd_points(pre[..., :nq], pre[..., nq:nq + nv], u, pre[..., time_col + 1:], eps=eps, centered=centered,
                                    sensors=bool(sensor_derivatives))
    state, sens = _results(buf[1:], time_col, 1 + nq + nv)
    return (state, sens, *(x.permute(1, 0, 2, 3) for x in mats))


__all__ = ["rollout", "linearize_rollout"]
