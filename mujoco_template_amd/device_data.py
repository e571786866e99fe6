"""``DeviceData`` - the GPU-resident state of one data object as zero-copy torch views.

``MjData`` presents the state as numpy views over a pinned host mirror; every refresh moves the whole state block over PCIe.  A
controller written in torch (an MLP policy, batched MPC sampling) wants the opposite: read ``qpos`` / ``qvel`` where they live and
write ``ctrl`` there.  ``DeviceData`` is that view (``BatchSim.torch_view``, ``__cuda_array_interface__``): no copy is made, in-place
writes to the state views are legal and the next launch on the data object reads them.  Work must be ordered on the library's
stream - ``Env`` binds it to torch's current stream (``BatchSim.use_torch_stream``) before it calls a device controller.

Shapes (dtype of the data unless noted): ``qpos [B, nq]``, ``qvel / qacc / qacc_warmstart [B, nv]``, ``ctrl [B, nu]``, ``time [B]``
(float64), ``xpos / xipos / subtree_com [B, nbody, 3]``, ``xquat [B, nbody, 4]``, ``site_xpos [B, nsite, 3]``, ``geom_xpos [B, ngeom, 3]``,
``sensordata [B, nsensordata]``, ``episode [B]`` (int32: resets of each environment by ``reset_envs``).  The derived arrays hold the
last forward pass (after a step: the pre-integration pass, as in MuJoCo).
"""

from __future__ import annotations

from typing import Any

STATE_FIELDS = ("qpos", "qvel", "ctrl", "qacc", "qacc_warmstart")
DERIVED_FIELDS = ("xpos", "xquat", "xipos", "site_xpos", "geom_xpos", "subtree_com", "sensordata")
_VEC = {"xpos": 3, "xquat": 4, "xipos": 3, "site_xpos": 3, "geom_xpos": 3, "subtree_com": 3}


class DeviceData:
    """Zero-copy torch views over one data object's device arrays (built once; valid while the data object lives)."""

    def __init__(self, data: Any):
        sim = getattr(data, "sim", data)                    # an MjData or a BatchSim
        self.sim = sim
        self.batch = int(sim.batch)
        self.dtype = sim.dtype
        for name in STATE_FIELDS:
            setattr(self, name, sim.torch_view(name))
        for name in DERIVED_FIELDS:
            v = sim.torch_view(name)
            if name in _VEC:
                v = v.view(self.batch, -1, _VEC[name])
            setattr(self, name, v)
        self.time = sim.torch_view("time")[:, 0]
        self.episode = sim.torch_view("episode")[:, 0]

    @property
    def device(self):
        return self.qpos.device

    def __repr__(self) -> str:
        return f"<DeviceData batch={self.batch} dtype={self.dtype} device={self.device}>"


__all__ = ["DeviceData", "STATE_FIELDS", "DERIVED_FIELDS"]
