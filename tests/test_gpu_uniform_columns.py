"""Uniform record columns baked as constants (UniformCols / MJB_REC): the specialised fp32 kernels
(one wave, and two waves where the model has them) against the generic kernel, byte for byte, on the small models of
tests/uniform_columns_models.py - all columns uniform, then one column at a time made non-uniform, so that a constant substituted
for a column that is NOT one (or a wrong value for one that is) moves a bit.  fp32, batch 4, 30 single steps with random controls;
qpos, qvel, qacc after every step, the dumped rows (efc_J, efc_aref, efc_D) at the start and the end, and the counters of every
step.  Each case asserts from those counters that the rows it is for were active in every environment.  A model has a two-wave
kernel only at 64 lanes per environment, which these small models do not get by default: the cases with non-uniform columns run
once more at lanes=64 (TWO_WAVE_LANES), and there the two-wave comparison is required to have happened."""
import os

import numpy as np
import pytest

from mujoco_template_amd import mjcf
from mujoco_template_amd._capi import CTRL_RANDOM, BatchSim, DeviceModel
from tests import uniform_columns_models as ucm

pytestmark = pytest.mark.gpu

B, STEPS = 4, 30
TWO_WAVE_LANES = 64
ROWS = ("efc_J", "efc_aref", "efc_D")


def _dump(sim, out, tag):
    sim.debug_forward()
    nefc = sim.counters()["nefc"]
    for k in ROWS:
        a = sim.debug_get(k).reshape(sim.batch, sim.nefcmax, -1).copy()
        for e in range(sim.batch):
            a[e, nefc[e]:] = 0                                     # rows at and above nefc are never written
        out[f"{tag}_{k}"] = a
    out[f"{tag}_nefc"] = nefc.copy()


def _run(dm, q, v, variant, **caps):
    """Everything one kernel variant computes for a case, or None where the model has no two-wave kernel."""
    if variant == "two" and dm.step2_spec_source(**caps) is None:
        return None
    prev = os.environ.get("MJB_TWO_WAVE")
    os.environ["MJB_TWO_WAVE"] = "1" if variant == "two" else "0"  # read by the data object's first stepping launch
    try:
        sim = BatchSim(dm, q.shape[0], dtype="float32", specialize=variant != "generic", **caps)
        assert sim.specialized == (variant != "generic")
        out = {"lanes": np.array(sim.lanes)}
        sim.set("qpos", q); sim.set("qvel", v)
        _dump(sim, out, "start")
        sim.set("qpos", q); sim.set("qvel", v)
        cnt = []
        for s in range(STEPS):
            sim.rollout(1, CTRL_RANDOM, seed=5, step0=s, ctrl_scale=1.0)
            c = sim.counters()
            cnt.append(np.stack([c[k] for k in ("ncon", "nefc", "con_dropped", "efc_dropped")], axis=1))
            for k in ("qpos", "qvel", "qacc"):
                out[f"{k}_{s}"] = sim.get(k)
        if variant == "two":
            assert sim.schedule_info()["waves_per_env"] == 2
        out["counters"] = np.stack(cnt)                            # [step, env, (ncon, nefc, con_dropped, efc_dropped)]
        _dump(sim, out, "end")
        return sim, out
    finally:
        if prev is None:
            os.environ.pop("MJB_TWO_WAVE", None)
        else:
            os.environ["MJB_TWO_WAVE"] = prev


def _compare(xml, start, *, batch=B, two_wave=False, **caps):
    cm = mjcf.compile_xml_string(xml)
    dm = DeviceModel(cm)
    q, v = start(batch, cm)
    _, ref = _run(dm, q, v, "generic", **caps)
    assert all(np.isfinite(ref[f"qpos_{STEPS - 1}"]).ravel())
    compared = []
    for variant in ("spec", "two"):
        got = _run(dm, q, v, variant, **caps)
        if got is None:
            continue
        compared.append(variant)
        for k, a in ref.items():
            b = got[1][k]
            assert a.dtype == b.dtype and a.shape == b.shape, (variant, k)
            assert a.tobytes() == b.tobytes(), f"{variant} {k}: {int((a != b).sum())} of {a.size} values differ"
    assert compared == (["spec", "two"] if two_wave else ["spec"])   # the two-wave kernel exists exactly at 64 lanes per environment
    return cm, dm, q, v, ref


def _fd_bits(dm, q, v):
    """(A, B) of transition_fd at the first two start states: specialised against generic float64 finite-difference kernel."""
    res = []
    for spec in (False, True):
        sim = BatchSim(dm, 2, dtype="float32", specialize=False)
        sim.set("qpos", q[:2]); sim.set("qvel", v[:2])
        if spec:
            sim.specialize_fd()                                    # (specialize=False keeps the first transition_fd from doing it)
        A, Bm = sim.transition_fd()
        assert sim.fd_specialized == spec
        res.append((np.array(A), np.array(Bm)))
    for a, b in zip(res[0], res[1]):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case,lanes", [(c, 0) for c in ucm.ARM_CASES] + [(c, TWO_WAVE_LANES) for c in ("uniform", "solimp_mid_power", "ctrlrange", "second_body_rotated")])
def test_arm_limit_rows(case, lanes):
    """Two limited hinges: identical limit parameters, control ranges and body frames (every column uniform), then the second joint's
    solimp mid / power, its control range, and one or the other body frame changed.  lanes=64: the two-wave kernel too."""
    cm, dm, q, v, ref = _compare(ucm.ARM_CASES[case], lambda n, cm: ucm.arm_start(n), two_wave=lanes == TWO_WAVE_LANES, lanes=lanes)
    assert not lanes or int(ref["lanes"]) == lanes
    nefc = ref["counters"][:, :, 1]
    assert ((nefc > 0).mean(axis=0) > 0).all() and (ref["start_nefc"] > 0).all()      # limit rows in every environment
    assert ref["counters"][:, :, 0].sum() == 0                                         # (no contacts in this model)
    if case in ("uniform", "solimp_mid_power") and not lanes:
        _fd_bits(dm, q, v)


@pytest.mark.parametrize("case,lanes", [(c, 0) for c in ucm.SPHERE_CASES] + [(c, TWO_WAVE_LANES) for c in ucm.SPHERE_CASES])
def test_sphere_contact_rows(case, lanes):
    """Two spheres on a plane: equal margins and frictions, then one sphere's changed (pair_kb, pair_friction, pair_cull columns).
    lanes=64: the two-wave kernel too."""
    cm, dm, q, v, ref = _compare(ucm.SPHERE_CASES[case], ucm.spheres_start, two_wave=lanes == TWO_WAVE_LANES, lanes=lanes)
    ncon = ref["counters"][:, :, 0]
    assert ((ncon > 0).mean(axis=0) > 0).all() and (ref["start_nefc"] > 0).all()
    assert (ncon[0] >= 3).all()                                                        # both plane pairs and the sphere pair at the first step


def test_more_survivors_than_lanes():
    """Five spheres in a row at 8 lanes per environment: 9 pairs pass the broad phase, so the survivor list is flushed inside the
    loop and again at its end (the narrow phase with folded geom / pair columns runs at both places).  Contacts, counts and drops
    equal the generic kernel's, also with a contact cap that drops some."""
    cm, dm, q, v, ref = _compare(ucm.crowd_xml(), ucm.crowd_start, **ucm.CROWD_CAPS)
    assert int(ref["lanes"]) == 8
    assert (ref["counters"][0, :, 0] > 8).all()                                        # more contacts (hence survivors) than lanes
    assert ref["counters"][:, :, 2:].sum() == 0
    cm, dm, q, v, ref = _compare(ucm.crowd_xml(), ucm.crowd_start, **ucm.CROWD_CAPS_DROP)
    assert (ref["counters"][:, :, 2].sum(axis=0) > 0).all()                            # contacts dropped in every environment
