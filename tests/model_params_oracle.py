"""Oracle side of the per-environment model parameters (``BatchSim.set_env_params``): the compiled model of ONE environment.

``env_compiled(cm, **values)`` copies the compiled model, writes that environment's values of the per-environment fields into the copy
and re-derives what the compiler derives from them, by the compiler's own rule (``csrc/mjb_mjcf.cpp``):

* ``body_subtreemass``: ``body_mass`` summed over the subtree (leaves to the root, body ids descending);
* ``pair_friction``: element-wise max of the two geoms' ``geom_friction``, stored ``[f0, f0, f1, f2, f2]``.

Everything else (``body_invweight0``, ``dof_invweight0``, ``meaninertia``, the pairs' solver constants) stays the compiled model's: the
semantics of editing ``mjModel`` without ``mj_setConst``.  ``env_oracle`` builds the ``mjo.OracleModel`` of that copy.
"""
from __future__ import annotations

import copy

import numpy as np

FIELDS = ("body_mass", "body_inertia", "dof_damping", "dof_armature", "actuator_gear", "actuator_gainprm", "actuator_biasprm",
          "geom_friction", "gravity")


def derive(cm) -> None:
    """Re-derive ``body_subtreemass`` and ``pair_friction`` of ``cm`` in place from its ``body_mass`` / ``geom_friction``."""
    A = cm.arrays
    parent = np.asarray(A["body_parentid"])
    sub = np.array(A["body_mass"], dtype=np.float64).reshape(-1)
    for b in range(cm.nbody - 1, 0, -1):
        sub[parent[b]] += sub[b]
    A["body_subtreemass"] = sub.reshape(np.shape(A["body_subtreemass"]))
    gf = np.asarray(A["geom_friction"], dtype=np.float64).reshape(-1, 3)
    g1, g2 = np.asarray(A["pair_geom1"]), np.asarray(A["pair_geom2"])
    f = np.maximum(gf[g1], gf[g2])
    A["pair_friction"] = np.stack([f[:, 0], f[:, 0], f[:, 1], f[:, 2], f[:, 2]], axis=1).reshape(np.shape(A["pair_friction"]))


def env_compiled(cm, **values):
    """A copy of the compiled model carrying one environment's ``values`` (field name -> that environment's array)."""
    c = copy.copy(cm)                                          # (the compiled model may hold a library handle: copy the data, not that)
    c.__dict__.pop("_device_model", None)
    c.arrays = {k: np.array(v, copy=True) for k, v in cm.arrays.items()}
    c.gravity = np.array(cm.gravity, dtype=np.float64, copy=True)
    for name, v in values.items():
        if name not in FIELDS:
            raise KeyError(name)
        if name == "gravity":
            c.gravity = np.array(v, dtype=np.float64).reshape(3)
        else:
            c.arrays[name] = np.array(v, dtype=np.float64).reshape(np.shape(cm.arrays[name]))
    derive(c)
    return c


def env_oracle(cm, **values):
    from oracle import mjo

    return mjo.OracleModel(env_compiled(cm, **values))


def row(params: dict, e: int) -> dict:
    """Environment e's values of a dict of [B, ...] per-environment arrays."""
    return {k: np.asarray(v)[e] for k, v in params.items()}
