"""Records tests/golden/rows_bits.npz: the BITS the fp32 step kernels produce for the constraint-row phase (limit and contact rows,
their caps and drop counts) and for short rollouts, on a real MI355X.  tests/test_gpu_rows_one_pass.py asserts byte equality with it
for the generic, the specialised and the two-wave kernel, so a change to make_constraint, the contact Jacobian, the fixed-tendon
Jacobian or the kinematics that is meant to keep every result bit for bit is compared against the build that wrote this file and
not only against another instantiation of the same source.

A pull request that changes upstream arithmetic ON PURPOSE (anything that moves a bit of qpos, qvel or a constraint row) regenerates
the fixture with the build it replaces reviewed, and says so:

    python tests/golden/make_rows_bits.py [OUT]      # needs the GPU; writes tests/golden/rows_bits.npz (or OUT)

Per case (see CASES) the file holds, for a dump at the start state and a dump after the rollout: efc_J, efc_D, efc_aref, efc_pos (as
uint32 views of the fp32 values, rows at and above nefc zeroed: they are never written), efc_type, and the counters; plus qpos / qvel
after the rollout as uint32 views.  The generic kernel writes the file; the generator refuses to write it unless the specialised and
the two-wave kernel give the same bytes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "rows_bits.npz")
ROW_ARRAYS = ("efc_J", "efc_D", "efc_aref", "efc_pos")
VARIANTS = ("generic", "spec", "two")          # two: the specialised two-wave kernel, where the model has one

# a hinge whose range is narrower than twice its limit margin: both sides of the limit are active at once
BOTH_SIDES_XML = """<mujoco><option timestep="0.005"/><worldbody>
  <body><joint name="h" type="hinge" axis="0 1 0" limited="true" range="-0.01 0.01" margin="0.05" damping="0.1"/>
    <geom type="capsule" size="0.03" fromto="0 0 0 0.3 0 0"/></body>
</worldbody><actuator><motor joint="h" gear="1" ctrllimited="true" ctrlrange="-1 1"/></actuator></mujoco>"""

# name -> model, batch, steps, caps, lanes, ctrl ("random" seed / scale, or a constant ctrl value)
CASES = {
    "humanoid": dict(model="humanoid", B=8, steps=40, ctrl=("random", 7, 1.0)),
    "humanoid_caps": dict(model="humanoid", B=8, steps=40, ctrl=("random", 7, 1.0), nefcmax=8, nconmax=2),
    "drone2_drop": dict(model="drone2", B=4, steps=100, ctrl=("zero",)),
    "drone2_flipped": dict(model="drone2", B=4, steps=30, ctrl=("zero",)),      # upside down in the floor: 20 contacts, more items than lanes
    "cartpole_limit": dict(model="cartpole", B=4, steps=60, ctrl=("const", 200.0)),
    "both_sides": dict(model="both_sides", B=2, steps=20, ctrl=("random", 3, 1.0)),
    "chain64": dict(model="chain64", B=2, steps=10, ctrl=("random", 5, 1.0), nefcmax=96, nconmax=24, lanes=64),
    "tree": dict(model="tree", B=2, steps=10, ctrl=("random", 5, 1.0), nefcmax=96, nconmax=24, lanes=64),
}


def compiled_model(name):
    from mujoco_template_amd import mjcf
    from tests.conftest import MODELS
    from tests.large_models import LARGE_MODELS

    if name in MODELS:
        return mjcf.compile_xml_path(MODELS[name])
    if name == "both_sides":
        return mjcf.compile_xml_string(BOTH_SIDES_XML)
    return mjcf.compile_xml_string(LARGE_MODELS[name]())


def start_state(case, cm):
    """(qpos, qvel) [B, .] float64 of a case: keyframes and qpos0 for the humanoid, a flat drop for the drone, the cart next to its
    upper limit, the large models in floor contact (tests.large_models.initial_state)."""
    from oracle import mjo
    from tests.large_models import initial_state

    c = CASES[case]
    B = c["B"]
    q = np.tile(np.array(cm.qpos0, dtype=np.float64), (B, 1))
    v = np.zeros((B, cm.nv))
    if c["model"] == "humanoid":
        od = mjo.OracleData(mjo.OracleModel(cm))
        for e, key in enumerate((-1, -1, 0, 0, 1, 1, 2, 3)):     # qpos0, squat, stand_on_left_leg, prone, supine
            if key >= 0:
                od.reset_keyframe(key)
                q[e] = od.qpos
        v[1::2] = np.random.default_rng(11).normal(size=(B // 2, cm.nv)) * 0.2
        hip, knee = (cm.jnt_qposadr[cm.names[3].index(n)] for n in ("hip_y_right", "knee_right"))
        q[1::4, hip] = -1.2; q[1::4, knee] = 0.0                 # hamstring_right = 0.5 hip_y - 0.5 knee = -0.6, below its range [-0.3, 2]
    elif case == "drone2_flipped":
        q[:, 2] = 0.03 + 0.005 * np.arange(B)
        q[:, 3:7] = (0, 1, 0, 0)
    elif c["model"] == "drone2":
        q[:, 2] = 0.1
        q[:, 0] = 0.01 * np.arange(B)
    elif c["model"] == "cartpole":
        q[:, 0] = 1.9 + 0.02 * np.arange(B)
        v[:, 0] = 1.0
    elif c["model"] == "both_sides":
        q[:, 0] = (0.0, 0.004)
    else:
        rng = np.random.default_rng(cm.nv)
        for e in range(B):
            q[e], v[e] = initial_state(cm, c["model"], rng)
    return q, v


def _bits(a):
    return np.ascontiguousarray(a.astype(np.float32)).view(np.uint32)


def _dump(sim, cm, tag, out):
    sim.debug_forward()
    cn = sim.counters()
    nefc = cn["nefc"]
    for k in ROW_ARRAYS:
        a = sim.debug_get(k).reshape(sim.batch, sim.nefcmax, -1)
        for e in range(sim.batch):
            a[e, nefc[e]:] = 0
        out[f"{tag}_{k}"] = _bits(a.reshape(sim.batch, -1))
    t = sim.debug_get("efc_type").copy()
    for e in range(sim.batch):
        t[e, nefc[e]:] = 0
    out[f"{tag}_efc_type"] = t
    out[f"{tag}_counters"] = np.stack([cn[k] for k in cn], axis=1).astype(np.int32)


def run_case(case, variant, dm=None):
    """The arrays of one case under one kernel variant (None where the model has no two-wave kernel), keyed as in the fixture."""
    from mujoco_template_amd._capi import CTRL_KEEP, CTRL_RANDOM, CTRL_ZERO, BatchSim, DeviceModel

    c = CASES[case]
    cm = compiled_model(c["model"])
    dm = dm or DeviceModel(cm)
    caps = dict(nefcmax=c.get("nefcmax", 0), nconmax=c.get("nconmax", 0), lanes=c.get("lanes", 0))
    if variant == "two" and dm.step2_spec_source(**caps) is None:
        return None
    prev = os.environ.get("MJB_TWO_WAVE")
    os.environ["MJB_TWO_WAVE"] = "1" if variant == "two" else "0"   # read by the data object's first stepping launch
    try:
        sim = BatchSim(dm, c["B"], dtype="float32", specialize=variant != "generic", **caps)
        q, v = start_state(case, cm)
        sim.set("qpos", q); sim.set("qvel", v)
        out = {}
        _dump(sim, cm, "start", out)
        sim.set("qpos", q); sim.set("qvel", v)
        kind = c["ctrl"][0]
        if kind == "random":
            sim.rollout(c["steps"], CTRL_RANDOM, seed=c["ctrl"][1], ctrl_scale=c["ctrl"][2])
        elif kind == "zero":
            sim.rollout(c["steps"], CTRL_ZERO)
        else:
            sim.set("ctrl", np.full((c["B"], cm.nu), c["ctrl"][1]))
            sim.rollout(c["steps"], CTRL_KEEP)
        if variant == "two":
            assert sim.schedule_info()["waves_per_env"] == 2
        cn = sim.counters()
        out["roll_counters"] = np.stack([cn[k] for k in cn], axis=1).astype(np.int32)
        out["qpos"] = _bits(sim.get("qpos")); out["qvel"] = _bits(sim.get("qvel"))
        _dump(sim, cm, "end", out)
    finally:
        if prev is None:
            os.environ.pop("MJB_TWO_WAVE", None)
        else:
            os.environ["MJB_TWO_WAVE"] = prev
    return {f"{case}/{k}": a for k, a in out.items()}


def main():
    fixture = {}
    for case in CASES:
        ref = run_case(case, "generic")
        for variant in VARIANTS[1:]:
            got = run_case(case, variant)
            if got is None:
                continue
            for k, a in ref.items():
                if not np.array_equal(a, got[k]):
                    raise SystemExit(f"{k}: the {variant} kernel differs from the generic one; nothing written")
        fixture.update(ref)
        cn = ref[f"{case}/end_counters"]
        types = sorted(set((ref[f"{case}/end_efc_type"] & 0xff)[ref[f"{case}/end_efc_pos"] != 0].tolist()))
        print(case, "nefc", cn[:, 1].tolist(), "ncon", cn[:, 0].tolist(), "dropped", ref[f"{case}/roll_counters"][:, 3:5].sum(0).tolist(), "types", types)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(out, **fixture)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
