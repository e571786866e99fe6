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


def _tensor(x: Any, dev, dtype, what: str):
    import torch

    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype)
    try:
        return torch.as_tensor(x, dtype=dtype).to(dev)
    except (TypeError, ValueError, RuntimeError) as exc:
        raise ConfigError(f"rollout: {what} must be a tensor or an array: {exc}") from exc


def rollout(model: MjModel, data: MjData, control=None, *, initial_state=None, initial_warmstart=None, nstep: int | None = None):
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
    """
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
            raise ConfigError("rollout: without control, nstep must be given and >= 1")
        nstep = int(nstep)
    else:
        if not isinstance(control, torch.Tensor) or control.ndim not in (2, 3):
            raise ConfigError(f"rollout: control must be a torch tensor [B, T, {nu}] or [T, {nu}]")
        T = int(control.shape[-2])
        nstep = T if nstep is None else int(nstep)
        if nstep < 1 or nstep > T:
            raise ConfigError(f"rollout: nstep must lie in [1, {T}] (the control's steps), got {nstep}")

    sim.use_torch_stream()
    data.push_host_edits()                                      # pending in-place edits of the host mirrors first, then the device writes
    if initial_state is not None:
        s = _tensor(initial_state, dev, torch.float64, "initial_state")
        if s.shape not in ((nx,), (B, nx)):
            raise ConfigError(f"rollout: initial_state must have shape [{nx}] or [{B}, {nx}] (time, qpos, qvel), got {list(s.shape)}")
        sim.torch_view("time")[:, 0].copy_(s[..., 0])
        sim.torch_view("qpos").copy_(s[..., 1:1 + nq])
        sim.torch_view("qvel").copy_(s[..., 1 + nq:])
    ws = sim.torch_view("qacc_warmstart")
    if initial_warmstart is None:
        ws.zero_()
    else:
        w = _tensor(initial_warmstart, dev, dt, "initial_warmstart")
        if w.shape != (B, nv):
            raise ConfigError(f"rollout: initial_warmstart must have shape [{B}, {nv}], got {list(w.shape)}")
        ws.copy_(w)

    cached = data.__dict__.get("_rollout_ring")                # (obs spec of the ring, column order of the result) per data object
    if cached is None:
        spec = sim.make_obs_spec(_RING_FLAGS)
        perm = torch.cat([torch.tensor([spec.dim - 1]), torch.arange(spec.dim - 1)]).to(dev)
        cached = (spec, perm)
        object.__setattr__(data, "_rollout_ring", cached)
    spec, perm = cached
    ring = torch.empty((nstep, B, spec.dim), device=dev, dtype=dt)
    if control is None:
        sim.rollout(nstep, CTRL_KEEP, obs_spec=spec, obs_out_ptr=ring.data_ptr(), obs_every=1)
    else:
        sim.rollout_ctrl(nstep, control, obs_spec=spec, obs_out_ptr=ring.data_ptr(), obs_every=1)
    data.mark_device_newer()
    # ring row: qpos | qvel | sensordata | time  ->  [B, T, time | qpos | qvel | sensordata] in one gather
    out = ring.permute(1, 0, 2).index_select(2, perm)
    return out[..., :nx], out[..., nx:]


__all__ = ["rollout"]
