"""The feature scenes of tests/feature_models.py on the CPU: both MJCF compilers agree on them, the kernel source (host emulation,
float64) follows the oracle through each of them, hand-derived anchors pin what kernel and oracle compute for each feature (so that a
misreading they share cannot hide behind their parity), the specialised kernel of each scene cross-compiles, and every honoured
attribute of the MJCF schema demonstrably reaches the simulation."""
import shutil

import numpy as np
import pytest

from mujoco_template_amd import mjcf
from oracle import mjo
from tests import pymjcf
from tests.feature_models import NOT_PHYSICS, PERTURB, SCENES, attrs_in_xml, perturbed
from tests.hostemu.emu import EmuEnv

NAMES = list(SCENES)
FWD_FIELDS = ("xpos", "xipos", "subtree_com", "cdof", "cinert", "cvel", "qM", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "qacc_smooth",
              "qfrc_constraint", "qacc")


def _compiled(name):
    return mjcf.compile_xml_string(SCENES[name].xml)


def _start_state(cm, od, seed):
    rng = np.random.default_rng(seed)
    q = od.integrate_pos(cm.qpos0, rng.normal(size=cm.nv) * 0.05, 1.0)
    return q, rng.normal(size=cm.nv) * 0.2


# ---------------------------------------------------------------------------------------------------------------------------------
# compilers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_native_compiler_matches_the_python_restatement(name):
    """As tests/test_mjcf.py::test_native_compiler_matches_the_python_restatement, on every feature scene."""
    a, b = pymjcf.compile_xml_string(SCENES[name].xml), _compiled(name)
    for k in ("nq", "nv", "nu", "na", "nbody", "njnt", "ngeom", "nsite", "ntendon", "nwrap", "nsensor", "nsensordata", "nkey", "npair", "nexclude",
              "integrator", "iterations", "ls_iterations", "disableactuator", "name"):
        assert getattr(a, k) == getattr(b, k), k
    for k in ("timestep", "density", "viscosity", "impratio", "tolerance", "meaninertia"):
        assert getattr(a, k) == pytest.approx(getattr(b, k), rel=1e-13), k
    assert np.array_equal(a.gravity, b.gravity) and a.names == b.names and set(a.arrays) == set(b.arrays)
    for k in a.arrays:
        x, y = np.asarray(a.arrays[k], dtype=float), np.asarray(b.arrays[k], dtype=float)
        assert x.shape == y.shape, k
        if k in ("body_iquat", "body_inertia") or x.size == 0:
            continue
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(x).max()), k
    for bb in range(a.nbody):
        ia = mjcf.quat_to_mat(a.body_iquat[bb]) @ np.diag(a.body_inertia[bb]) @ mjcf.quat_to_mat(a.body_iquat[bb]).T
        ib = mjcf.quat_to_mat(b.body_iquat[bb]) @ np.diag(b.body_inertia[bb]) @ mjcf.quat_to_mat(b.body_iquat[bb]).T
        assert np.abs(ia - ib).max() <= 1e-12 * max(1e-30, np.abs(ia).max()), bb


@pytest.mark.parametrize("compiler", [mjcf, pymjcf], ids=["native", "python"])
def test_impratio_other_than_one_is_rejected_by_both_compilers(compiler):
    """<option impratio> is not implemented (kernel and oracle use impratio = 1): any other value is an error naming it, 1 compiles."""
    xml = SCENES["contact_mix"].xml
    with pytest.raises(mjcf.MjcfError if compiler is mjcf else pymjcf.MjcfError, match="impratio"):
        compiler.compile_xml_string(xml.replace('<option timestep="0.003"/>', '<option timestep="0.003" impratio="10"/>'))
    m = compiler.compile_xml_string(xml.replace('<option timestep="0.003"/>', '<option timestep="0.003" impratio="1.0"/>'))
    assert m.impratio == 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel source (host emulation, float64) against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [16, 64])
@pytest.mark.parametrize("name", NAMES)
def test_hostemu_forward_and_free_running_match_oracle(name, G):
    cm = _compiled(name)
    od = mjo.OracleData(mjo.OracleModel(cm))
    e = EmuEnv(cm, G=G, use_double=True)
    q, v = _start_state(cm, od, 1)
    u = od.random_ctrl(3, 0, 0, SCENES[name].ctrl_scale)
    od.qpos[:] = q; od.qvel[:] = v; od.ctrl[:] = u
    e.qpos[:] = q; e.qvel[:] = v; e.ctrl[:cm.nu] = u
    od.forward(); e.forward()
    for k in FWD_FIELDS:
        a, b = getattr(e, k), getattr(od, k)
        scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
        assert np.abs(a[:b.size] - b).max() <= 1e-11 * scale, k
    assert (e.counters[0], e.counters[1]) == (od.counters()["ncon"], od.counters()["nefc"])
    if cm.nsensordata:
        assert np.abs(e.sensordata[:cm.nsensordata] - od.sensordata).max() <= 1e-11 * max(1.0, np.abs(od.sensordata).max())
    rows = 0
    for s in range(60):
        u = od.random_ctrl(3, 0, s, SCENES[name].ctrl_scale)
        od.ctrl[:] = u; e.ctrl[:cm.nu] = u
        od.step(); e.step()
        c = od.counters()
        assert (e.counters[0], e.counters[1], e.counters[2]) == (c["ncon"], c["nefc"], c["solver_niter"]), s
        rows = max(rows, c["nefc"])
    assert np.abs(e.qpos - od.qpos).max() <= 1e-10
    assert rows > 0                                          # every scene has constraint rows in the rollout


def test_hostemu_follows_run_time_solver_options():
    """iterations / tolerance / disableactuator changed after compilation: the emulated kernel reads them as the oracle does."""
    from tests.feature_models import SOLVER_OPTS

    cm = _compiled(SOLVER_OPTS["scene"])
    cm.iterations, cm.tolerance, cm.disableactuator = SOLVER_OPTS["iterations"], SOLVER_OPTS["tolerance"], SOLVER_OPTS["disableactuator"]
    om = mjo.OracleModel(cm)
    od, e = mjo.OracleData(om), EmuEnv(cm, G=16, use_double=True)
    q, v = _start_state(cm, od, 2)
    od.qpos[:] = q; od.qvel[:] = v; e.qpos[:] = q; e.qvel[:] = v
    niter = []
    for s in range(60):
        u = od.random_ctrl(4, 0, s, 1.0)
        od.ctrl[:] = u; e.ctrl[:cm.nu] = u
        od.step(); e.step()
        niter.append(od.counters()["solver_niter"])
        assert e.counters[2] == niter[-1]
    assert max(niter) == SOLVER_OPTS["iterations"]
    assert np.abs(e.qpos - od.qpos).max() <= 1e-10


# ---------------------------------------------------------------------------------------------------------------------------------
# hand-derived anchors (MuJoCo's documented formulas), checked in the oracle AND the emulated kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _both(cm, q, v, u, G=16):
    od = mjo.OracleData(mjo.OracleModel(cm))
    e = EmuEnv(cm, G=G, use_double=True)
    od.qpos[:] = q; od.qvel[:] = v; od.ctrl[:] = u
    e.qpos[:] = q; e.qvel[:] = v; e.ctrl[:cm.nu] = u
    od.forward(); e.forward()
    return od, e


def test_servo_arm_actuator_forces_by_hand():
    """position: kp (ctrl - q) - kv qdot; general affine: g ctrl + b0 + b1 q + b2 qdot; motor: gear * clamp(ctrl, forcerange), the ctrl
    clamped to ctrlrange first.  One actuator per joint, so qfrc_actuator is the joint's force times its gear."""
    cm = _compiled("servo_arm")
    q, v = np.array([0.1, -0.3, 0.4]), np.array([0.7, -1.1, 0.5])
    for u, wrist in (([0.3, 0.4, 0.9], 2 * 0.6), ([-2.0, -1.0, -0.5], 2 * -0.4), ([0.1, 2.0, 0.1], 2 * 0.1)):
        u = np.array(u)
        od, e = _both(cm, q, v, u)
        uc = np.clip(u, [-1.5, -0.8, -1], [0.5, 1, 1])
        want = [30 * (uc[0] - q[0]) - 3 * v[0], 4 * uc[1] + 0.5 - 2.5 * q[1] - 0.4 * v[1], wrist]
        assert od.qfrc_actuator == pytest.approx(want, rel=1e-13, abs=1e-13)
        assert e.qfrc_actuator[:3] == pytest.approx(want, rel=1e-13, abs=1e-13)


def test_servo_arm_springs_and_ref_by_hand():
    """qpos0 = ref; passive force = -stiffness (q - springref) - damping qdot, with the class defaults resolved."""
    cm = _compiled("servo_arm")
    assert cm.qpos0 == pytest.approx([0.3, -0.2, 0.0])
    q, v = np.array([0.1, -0.3, 0.4]), np.array([0.7, -1.1, 0.5])
    od, e = _both(cm, q, v, np.zeros(3))
    want = [-6 * (q[0] - 0.6) - 0.4 * v[0], -0.25 * v[1], -0.25 * v[2]]
    assert od.qfrc_passive == pytest.approx(want, rel=1e-13, abs=1e-13)
    assert e.qfrc_passive[:3] == pytest.approx(want, rel=1e-13, abs=1e-13)


def test_servo_arm_joint_limit_rows_by_hand():
    """Shoulder past its upper limit and elbow inside the margin of its lower one: efc_pos = upper - q (J = -1) and q - lower (J = +1)."""
    cm = _compiled("servo_arm")
    q = np.array([0.36, -0.49, 0.0])
    od, e = _both(cm, q, np.zeros(3), np.zeros(3))
    assert od.counters()["nefc"] == 2 and e.counters[1] == 2
    for J, pos in ((od.efc_J.reshape(2, 3), od.efc_pos), (e.efc_J[:6].reshape(2, 3), e.efc_pos[:2])):
        assert J == pytest.approx(np.array([[-1, 0, 0], [0, 1, 0]]))
        assert pos == pytest.approx([0.35 - 0.36, -0.49 + 0.5], abs=1e-15)


@pytest.mark.parametrize("name,kind", [("servo_arm", 0), ("tendon_limits", 1)])
def test_limits_are_reached_on_both_sides_in_the_rollout(name, kind):
    """The scenes' joint / tendon limits are not decoration: within the 120-step rollout of the GPU tests rows of both signs appear."""
    cm = _compiled(name)
    od = mjo.OracleData(mjo.OracleModel(cm))
    signs = set()
    for s in range(120):
        od.ctrl[:] = od.random_ctrl(0, 0, s, SCENES[name].ctrl_scale)
        od.step()
        n = od.counters()["nefc"]
        J = od.efc_J.reshape(n, cm.nv)
        signs.update(int(np.sign(J[i][np.abs(J[i]).argmax()])) for i in range(n) if od.efc_type()[i] == kind)
    assert signs == {-1, 1}


def test_tendon_limit_rows_by_hand():
    """Fixed tendon L = 1.5 x - 0.7 theta (degrees converted), range [-0.12, 0.1], margin 0.03: below the lower limit the row has
    efc_pos = L - lower and J = dL/dq = (1.5, -0.7); above the upper one efc_pos = upper - L and J = (-1.5, 0.7)."""
    cm = _compiled("tendon_limits")
    assert cm.tendon_margin[0] == pytest.approx(0.03)
    for q, side in ((np.array([-0.05, 0.1]), -1), (np.array([0.08, 0.02]), 1)):
        L = 1.5 * q[0] - 0.7 * q[1]
        od, e = _both(cm, q, np.zeros(2), np.zeros(2))
        assert od.counters()["nefc"] == 1 and e.counters[1] == 1
        want_J = np.array([1.5, -0.7]) * (1 if side < 0 else -1)
        want_pos = (L + 0.12) if side < 0 else (0.1 - L)
        assert od.efc_J == pytest.approx(want_J, rel=1e-14) and e.efc_J[:2] == pytest.approx(want_J, rel=1e-14)
        assert od.efc_pos[0] == pytest.approx(want_pos, abs=1e-15) and e.efc_pos[0] == pytest.approx(want_pos, abs=1e-15)
        assert od.ten_length[0] == pytest.approx(L, abs=1e-15)


def test_contact_parameter_mixing_by_hand():
    """mj_contactParam at equal priority: mix = solmix1 / (solmix1 + solmix2) weights solref and solimp; friction and condim take the
    maximum; margin and gap the maximum.  Pinned on the compiled pairs, then on the rows: a scene whose geoms carry the pre-mixed
    parameters directly gives the same constraint rows (efc_D, efc_aref) in the oracle and in the emulated kernel."""
    cm = _compiled("contact_mix")
    floor, box, ball, rod = (cm.name2id(mjcf.OBJ_GEOM, n) for n in ("floor", "box_geom", "ball_geom", "rod_geom"))
    default_solimp = np.array([0.9, 0.95, 0.001, 0.5, 2.0])
    geoms = {floor: (1.0, [0.02, 1], [0.9, 0.95, 0.001, 0.5, 2], [0.6, 0.004, 0.0002], 1, 0, 0),
             box: (3.0, [0.01, 0.7], [0.8, 0.99, 0.003, 0.3, 2], [0.9, 0.01, 0.0001], 3, 0, 0),
             ball: (0.5, [0.03, 1.3], default_solimp, [1, 0.005, 0.0001], 1, 0, 0),
             rod: (2.0, [0.02, 1], [0.85, 0.97, 0.002, 0.5, 2], [0.3, 0.005, 0.0001], 3, 0.02, 0.012)}
    assert cm.npair == 3
    for p in range(cm.npair):
        g1, g2 = int(cm.pair_geom1[p]), int(cm.pair_geom2[p])
        assert g1 == floor
        s1, s2 = geoms[g1], geoms[g2]
        mix = s1[0] / (s1[0] + s2[0])
        assert cm.pair_solref[p] == pytest.approx(mix * np.array(s1[1]) + (1 - mix) * np.array(s2[1]), rel=1e-14)
        assert cm.pair_solimp[p] == pytest.approx(mix * np.array(s1[2]) + (1 - mix) * np.array(s2[2]), rel=1e-14)
        fr = np.maximum(s1[3], s2[3])
        assert cm.pair_friction[p] == pytest.approx([fr[0], fr[0], fr[1], fr[2], fr[2]], rel=1e-14)
        assert cm.pair_condim[p] == max(s1[4], s2[4]) == (1 if g2 == ball else 3)
        assert (cm.pair_margin[p], cm.pair_gap[p]) == (max(s1[5], s2[5]), max(s1[6], s2[6]))
    # the rows: the rod's floor contact (mix 1/3 between floor and rod), against the same contact with the parameters pre-mixed
    mix = 1.0 / 3.0
    sr = mix * np.array([0.02, 1]) + (1 - mix) * np.array([0.02, 1])
    si = mix * np.array([0.9, 0.95, 0.001, 0.5, 2]) + (1 - mix) * np.array([0.85, 0.97, 0.002, 0.5, 2])
    txt = lambda x: " ".join(repr(float(y)) for y in x)                  # noqa: E731
    pre = SCENES["contact_mix"].xml.replace('solimp="0.85 0.97 0.002 0.5 2" solmix="2"', f'solref="{txt(sr)}" solimp="{txt(si)}" solmix="1"')
    pre = pre.replace('solref="0.02 1"\n          solimp="0.9 0.95 0.001 0.5 2" solmix="1"', f'solref="{txt(sr)}"\n          solimp="{txt(si)}" solmix="1"')
    assert pre.count(txt(si)) == 2
    cp = mjcf.compile_xml_string(pre)
    q, v = cm.qpos0.copy(), np.zeros(cm.nv)
    (oa, ea), (ob, eb) = _both(cm, q, v, np.zeros(0)), _both(cp, q, v, np.zeros(0))
    n = oa.counters()["nefc"]
    assert n == 4 and ob.counters()["nefc"] == 4 and ea.counters[1] == eb.counters[1] == 4
    for a, b in ((oa.efc_D, ob.efc_D), (ea.efc_D[:n], eb.efc_D[:n]), (oa.efc_aref, ob.efc_aref), (ea.efc_aref[:n], eb.efc_aref[:n])):
        assert a == pytest.approx(b, rel=1e-12)
    assert ea.efc_D[:n] == pytest.approx(oa.efc_D, rel=1e-12)


def test_contact_in_the_gap_band_counts_but_has_no_rows():
    """margin 0.02, gap 0.012: a contact at distance d is generated for d < margin and is a constraint only for d < margin - gap.  The
    rod's lower end cap (d = 0.004) gives four pyramidal rows, its upper end cap (d = 0.014, in the band) is counted in ncon and gives
    none."""
    cm = _compiled("contact_mix")
    od, e = _both(cm, cm.qpos0.copy(), np.zeros(cm.nv), np.zeros(0))
    c = od.contacts()
    assert od.counters()["ncon"] == e.counters[0] == 2
    d = np.sort(c["dist"])
    assert d[0] < 0.02 - 0.012 <= d[1] < 0.02
    assert d == pytest.approx([0.004, 0.014], abs=2e-4)
    assert od.counters()["nefc"] == e.counters[1] == 4
    assert od.efc_pos == pytest.approx([d[0]] * 4, abs=1e-15)
    assert e.efc_pos[:4] == pytest.approx([d[0]] * 4, abs=1e-15)


def test_site_wrench_transmission_by_hand():
    """Site transmission with a 6-component gear: the actuator moment is J_site^T (R_site gear), i.e. the generalised force of a wrench
    gear[:3] (force) and gear[3:] (torque) expressed in the site frame and applied at the site."""
    cm = _compiled("site_wrench")
    od, e = _both(cm, cm.qpos0.copy(), np.zeros(cm.nv), np.array([0.7, 0.0]))
    sid = cm.name2id(mjcf.OBJ_SITE, "hub")
    R = od.site_xmat.reshape(-1, 3, 3)[sid]
    Jp, Jr = od.jac(0, sid)                                      # mjo_jac kind 0: a site
    gear = np.array([1, 0.5, 0.3, 0.02, -0.03, 0.05])
    want = 2 * 0.7 * (Jp.T @ (R @ gear[:3]) + Jr.T @ (R @ gear[3:]))
    assert od.qfrc_actuator == pytest.approx(want, rel=1e-12, abs=1e-14)
    assert e.qfrc_actuator[:cm.nv] == pytest.approx(want, rel=1e-12, abs=1e-14)


# ---------------------------------------------------------------------------------------------------------------------------------
# the specialised kernel source of each scene cross-compiles
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_specialised_kernel_source_compiles(name):
    from mujoco_template_amd._capi import DeviceModel, compile_spec

    if shutil.which("hipcc") is None and shutil.which("/opt/rocm/bin/hipcc") is None:
        pytest.skip("hipcc is not installed")
    dm = DeviceModel(_compiled(name))
    assert compile_spec(dm.spec_source()).endswith(".hsaco")


# ---------------------------------------------------------------------------------------------------------------------------------
# no inert attributes
# ---------------------------------------------------------------------------------------------------------------------------------
def _honoured():
    return {(tag, a) for tag, (hon, _ign) in pymjcf._SCHEMA_ATTRS.items() for a in hon}


def test_every_honoured_attribute_is_claimed_or_listed():
    """Each honoured (tag, attribute) of the schema is exercised by a feature scene or stated as not physics (NOT_PHYSICS, with reasons);
    a scene claims only what its XML actually writes."""
    honoured = _honoured()
    claimed = set()
    for s in SCENES.values():
        written = attrs_in_xml(s.xml)
        assert s.claims <= written, (s.name, sorted(s.claims - written))
        claimed |= s.claims
    assert NOT_PHYSICS <= honoured, sorted(NOT_PHYSICS - honoured)
    missing = honoured - claimed - NOT_PHYSICS
    assert not missing, sorted(missing)


def test_every_physics_attribute_has_a_perturbation_row():
    physics = _honoured() - NOT_PHYSICS
    rows = {(r[0], r[1]) for r in PERTURB}
    assert physics <= rows, sorted(physics - rows)
    assert rows <= physics, sorted(rows - physics)


def _trajectory(xml, steps=50, scale=1.0):
    cm = mjcf.compile_xml_string(xml)
    od = mjo.OracleData(mjo.OracleModel(cm))
    qs, ss = [], []
    for s in range(steps):
        od.ctrl[:] = od.random_ctrl(5, 0, s, scale)
        od.step()
        qs.append(od.qpos.copy())
        ss.append(od.sensordata.copy())
    return np.array(qs), np.array(ss)


@pytest.mark.parametrize("row", PERTURB, ids=[f"{r[0]}.{r[1]}@{r[2]}" for r in PERTURB])
def test_perturbing_an_attribute_changes_the_oracle_trajectory(row):
    """Each row changes one attribute of one scene; both compilers accept the result and the oracle's 50-step trajectory (qpos, or the
    sensor readings for a sensor attribute) changes.  An attribute that is parsed and stored but never read fails here."""
    tag, attr, scene = row[:3]
    xml = perturbed(row)
    assert (tag, attr) in attrs_in_xml(xml) or (tag, attr) in attrs_in_xml(SCENES[scene].xml)
    pymjcf.compile_xml_string(xml)
    q0, s0 = _trajectory(SCENES[scene].xml, scale=SCENES[scene].ctrl_scale)
    q1, s1 = _trajectory(xml, scale=SCENES[scene].ctrl_scale)
    if q0.shape != q1.shape:                                   # the row changed the model's dimensions (a joint's type)
        return
    changed = np.abs(q1 - q0).max() > 1e-9 or (s0.shape == s1.shape and s0.size and np.abs(s1 - s0).max() > 1e-9) or s0.shape != s1.shape
    assert changed, f"{tag} {attr} on {scene}: the trajectory did not change"
