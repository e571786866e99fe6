"""A catalogue of small MJCF scenes, one per group of accepted features, and the perturbation rows that show every honoured physics
attribute reaches the simulation.  Data and helpers only: tests/test_feature_models.py (CPU) and tests/test_gpu_feature_models.py (GPU)
run them.

Each scene records the ``(tag, attribute)`` pairs of ``tests.pymjcf._SCHEMA_ATTRS`` it exercises, the scale of its random controls and
whether it has contacts.  The shipped models and the scenes of tests/conftest.py are not repeated here."""
from __future__ import annotations

from dataclasses import dataclass

# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
# A three-hinge arm hanging from the world: a position servo with kp and kv, a general actuator with a fully affine bias, a motor
# whose force clamp is active, joint ref / springref / stiffness / damping (the implicit-damping Euler path) / armature, joint limits
# with margin, solreflimit and solimplimit that the start state and the rollout press on both sides.
SERVO_ARM = """<mujoco model="servo_arm">
  <compiler angle="radian" autolimits="true"/>
  <option timestep="0.004" integrator="Euler" iterations="30" tolerance="1e-9"/>
  <default>
    <joint type="hinge" armature="0.02"/>
    <geom type="capsule" size="0.035" contype="0" conaffinity="0" density="900"/>
    <default class="limb"><joint damping="0.25"/></default>
  </default>
  <worldbody>
    <body name="upper" pos="0 0 1" euler="0 0 0.4" childclass="limb">
      <joint name="shoulder" pos="0 0 0.01" axis="0 1 0" ref="0.3" springref="0.6" stiffness="6" damping="0.4" range="-0.12 0.35"
             margin="0.06" solreflimit="0.03 0.9" solimplimit="0.85 0.97 0.002 0.4 2"/>
      <geom fromto="0 0 0 0.3 0 0"/>
      <body name="fore" pos="0.3 0 0">
        <joint name="elbow" axis="0 1 0" ref="-0.2" range="-0.5 0.3" margin="0.02" solreflimit="0.015 1.2" solimplimit="0.8 0.99 0.004 0.6 2"/>
        <geom fromto="0 0 0 0.25 0 0" size="0.03"/>
        <body name="hand" pos="0.25 0 0">
          <joint name="wrist" class="limb" axis="0 0 1"/>
          <geom type="sphere" size="0.05" pos="0.08 0.02 0" mass="0.3"/>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator>
    <position name="servo" joint="shoulder" kp="30" kv="3" ctrllimited="true" ctrlrange="-1.5 0.5"/>
    <general name="affine" joint="elbow" gainprm="4" biastype="affine" biasprm="0.5 -2.5 -0.4" ctrllimited="true" ctrlrange="-0.8 1"/>
    <motor name="clamped" joint="wrist" gear="2" ctrllimited="true" ctrlrange="-1 1" forcelimited="true" forcerange="-0.4 0.6"/>
  </actuator>
</mujoco>
"""

# A slide and a hinge coupled by a limited fixed tendon with non-unit coefficients (one negative), a margin and its own solref /
# solimp; both tendon limits are reached in the rollout.
TENDON_LIMITS = """<mujoco model="tendon_limits">
  <option timestep="0.005" gravity="0 0 -9.81"/>
  <worldbody>
    <body name="cart" pos="0 0 0.5">
      <joint name="slider" type="slide" axis="1 0 0" damping="0.5" stiffness="20" springref="-0.2"/>
      <geom type="box" size="0.1 0.05 0.05" contype="0" conaffinity="0" mass="1.5"/>
      <body name="pole" pos="0 0 0" xyaxes="1 0 0 0 0 1">
        <joint name="hinge" type="hinge" axis="0 0 1" damping="0.05" stiffness="2" springref="-25"/>
        <geom type="capsule" size="0.02" fromto="0 0 0 0 -0.4 0" contype="0" conaffinity="0" density="700"/>
      </body>
    </body>
  </worldbody>
  <tendon>
    <fixed name="coupling" limited="true" range="-0.12 0.1" margin="0.03" solreflimit="0.02 1.1" solimplimit="0.9 0.96 0.003 0.5 2">
      <joint joint="slider" coef="1.5"/>
      <joint joint="hinge" coef="-0.7"/>
    </fixed>
  </tendon>
  <actuator>
    <motor name="push" joint="slider" gear="3" ctrllimited="true" ctrlrange="-1 1"/>
    <motor name="twist" joint="hinge" gear="0.4"/>
  </actuator>
</mujoco>
"""

# A box, a sphere and a capsule dropped on a plane.  Every pair mixes different solref / solimp / solmix and friction (maximum).  The
# floor is condim 1: against the condim-1 sphere its contacts are frictionless, against the condim-3 box and capsule pyramidal.  The
# capsule carries margin and gap and starts with one end cap in the band between margin - gap and margin: that contact is counted in
# ncon and produces no constraint rows.  The sphere starts overlapping the capsule, and an <exclude> keeps that pair out.  contype /
# conaffinity keep the box apart from both (box-sphere and box-capsule are outside the collision subset) and let the box meet the
# floor through one bit only.
CONTACT_MIX = """<mujoco model="contact_mix">
  <option timestep="0.003"/>
  <worldbody>
    <geom name="floor" type="plane" size="3 3 0.1" contype="1" conaffinity="6" condim="1" friction="0.6 0.004 0.0002" solref="0.02 1"
          solimp="0.9 0.95 0.001 0.5 2" solmix="1"/>
    <body name="box" pos="0 0 0.1" quat="0.9914449 0 0 0.1305262">
      <freejoint name="box_free"/>
      <geom name="box_geom" type="box" size="0.1 0.08 0.06" contype="2" conaffinity="0" condim="3" friction="0.9 0.01 0.0001" solref="0.01 0.7"
            solimp="0.8 0.99 0.003 0.3 2" solmix="3" density="600" euler="0.04 -0.03 0"/>
    </body>
    <body name="ball" pos="0.8 0.1 0.12">
      <freejoint/>
      <geom name="ball_geom" type="sphere" size="0.07" contype="4" conaffinity="5" condim="1" solref="0.03 1.3" solmix="0.5" mass="0.4"/>
    </body>
    <body name="rod" pos="0.8 0 0.059" axisangle="0 0 1 0.3">
      <freejoint/>
      <geom name="rod_geom" type="capsule" size="0.05 0.2" contype="4" conaffinity="5" zaxis="1 0 0.025" margin="0.02" gap="0.012"
            friction="0.3 0.005 0.0001" solimp="0.85 0.97 0.002 0.5 2" solmix="2"/>
    </body>
  </worldbody>
  <contact><exclude name="no_ball_rod" body1="ball" body2="rod"/></contact>
</mujoco>
"""

# RK4 with a floor contact, joint limits and joint damping: a two-link leg whose foot lands on the floor.
RK4_CONTACT = """<mujoco model="rk4_contact">
  <option timestep="0.004" integrator="RK4"/>
  <worldbody>
    <geom name="floor" type="plane" size="2 2 0.1"/>
    <body name="thigh" pos="0 0 0.5">
      <joint name="hip" type="hinge" axis="0 1 0" damping="0.3" limited="true" range="-40 30" margin="0.01"/>
      <geom type="capsule" size="0.04" fromto="0 0 0 0 0 -0.25" contype="0" conaffinity="0"/>
      <body name="shin" pos="0 0 -0.25">
        <joint name="knee" type="hinge" axis="0 1 0" damping="0.2" stiffness="2" limited="true" range="-5 25"/>
        <joint name="lift" type="slide" axis="0 0 1" damping="1.5" limited="true" range="-0.1 0.05"/>
        <geom type="capsule" size="0.035" fromto="0 0 0 0.05 0 -0.22"/>
      </body>
    </body>
  </worldbody>
  <actuator>
    <motor joint="hip" gear="4" ctrllimited="true" ctrlrange="-1 1"/>
    <position joint="knee" kp="8" ctrlrange="-0.5 1.5" ctrllimited="true"/>
  </actuator>
  <sensor><jointpos name="knee_angle" joint="knee"/></sensor>
</mujoco>
"""

# A free body pushed through a site transmission with a full 6-component gear, under a tilted gravity and a fluid (density,
# viscosity); accelerometer / gyro / framequat on a rotated site while the body rests on the floor.  Two actuator groups: the
# run-time option tests disable group 1.
SITE_WRENCH = """<mujoco model="site_wrench">
  <option timestep="0.004" gravity="0.8 -0.3 -7.5" density="1.2" viscosity="0.05"/>
  <worldbody>
    <geom name="floor" type="plane" size="3 3 0.1" friction="0.8 0.005 0.0001"/>
    <body name="puck" pos="0 0 0.06">
      <freejoint name="puck_free"/>
      <geom name="puck_geom" type="box" size="0.12 0.09 0.05" density="500"/>
      <geom name="mast" type="capsule" size="0.02" fromto="0 0 0.05 0 0 0.2" density="300"/>
      <site name="hub" pos="0.03 -0.02 0.04" euler="10 -20 30"/>
      <site name="imu" pos="-0.04 0.02 0.05" quat="0.9659258 0 0.258819 0"/>
    </body>
  </worldbody>
  <actuator>
    <general name="wrench" site="hub" gear="1 0.5 0.3 0.02 -0.03 0.05" gainprm="2" ctrllimited="true" ctrlrange="-1 1" group="0"/>
    <motor name="lifter" site="hub" gear="0 0 1 0 0.01 0" ctrllimited="true" ctrlrange="0 1" group="1"/>
  </actuator>
  <sensor>
    <accelerometer name="acc" site="imu"/>
    <gyro name="gyro" site="imu"/>
    <framequat name="orient" objtype="site" objname="imu"/>
  </sensor>
</mujoco>
"""


@dataclass(frozen=True)
class Scene:
    name: str
    xml: str
    claims: frozenset          # (schema tag, attribute) pairs of tests.pymjcf._SCHEMA_ATTRS the scene exercises
    ctrl_scale: float          # scale of the random controls (mjo random_ctrl / CTRL_RANDOM)
    contacts: bool             # contacts occur in the rollout


def _claims(*spec: str) -> frozenset:
    """``"joint: ref springref"`` -> {("joint", "ref"), ("joint", "springref")}."""
    out = set()
    for s in spec:
        tag, attrs = s.split(":")
        out.update((tag.strip(), a) for a in attrs.split())
    return frozenset(out)


SCENES = {s.name: s for s in (
    Scene("servo_arm", SERVO_ARM, _claims(
        "compiler: angle autolimits", "option: timestep integrator iterations tolerance", "body: pos euler childclass",
        "joint: type pos axis range damping stiffness armature margin ref springref solreflimit solimplimit",
        "geom: type size fromto pos density mass",
        "position: joint kp kv ctrllimited ctrlrange", "general: joint gainprm biastype biasprm ctrllimited ctrlrange",
        "motor: joint gear ctrllimited ctrlrange forcelimited forcerange"), 1.0, False),
    Scene("tendon_limits", TENDON_LIMITS, _claims(
        "option: gravity", "body: xyaxes",
        "fixed: limited range margin solreflimit solimplimit", "tendon/joint: coef"), 1.0, False),
    Scene("contact_mix", CONTACT_MIX, _claims(
        "body: quat axisangle", "geom: friction solref solimp solmix condim margin gap euler zaxis contype conaffinity",
        "exclude: body1 body2"), 1.0, True),
    Scene("rk4_contact", RK4_CONTACT, _claims("option: integrator", "joint: limited", "jointpos: joint"), 1.0, True),
    Scene("site_wrench", SITE_WRENCH, _claims(
        "option: gravity density viscosity", "site: pos euler quat", "general: site gear", "motor: site",
        "accelerometer: site", "gyro: site", "framequat: objname"), 1.0, True),
)}

# run-time options exercised on a baked model: set_solver / set_disableactuator after the model object exists
SOLVER_OPTS = dict(scene="site_wrench", iterations=2, tolerance=1e-3, disableactuator=1 << 1)

# ---------------------------------------------------------------------------------------------------------------------------------
# coverage: honoured attributes no scene needs to perturb, with the reason
# ---------------------------------------------------------------------------------------------------------------------------------
NOT_PHYSICS = {
    # names and references by name: they select objects, the object's own attributes carry the physics
    ("mujoco", "model"), ("body", "name"), ("joint", "name"), ("freejoint", "name"), ("geom", "name"), ("site", "name"), ("fixed", "name"),
    ("motor", "name"), ("position", "name"), ("general", "name"), ("jointpos", "name"), ("gyro", "name"), ("accelerometer", "name"),
    ("framequat", "name"), ("exclude", "name"), ("key", "name"), ("tendon/joint", "joint"),
    # default classes: a class only decides which defaults apply (the resolved attributes are claimed)
    ("joint", "class"), ("geom", "class"), ("site", "class"), ("fixed", "class"), ("motor", "class"), ("position", "class"), ("general", "class"),
    # actuator groups act only through the run-time opt.disableactuator mask (the GPU run-time option test)
    ("motor", "group"), ("position", "group"), ("general", "group"),
    # accepted at a single value only (anything else is an MjcfError): cone pyramidal, solver Newton, jacobian dense / auto,
    # general dyntype none / gaintype fixed, framequat objtype site, one geom priority per contact pair
    ("option", "cone"), ("option", "solver"), ("option", "jacobian"), ("general", "dyntype"), ("general", "gaintype"), ("framequat", "objtype"),
    ("geom", "priority"),
    # keyframes are read by reset(key) only (tests/test_gpu_parity.py, the humanoid's keyframes); <include> is textual
    ("key", "qpos"), ("key", "qvel"), ("key", "ctrl"), ("key", "time"), ("include", "file"),
    # orientations the scenes do not need: the same quaternion helper as the claimed ones (body / geom / site)
    ("body", "zaxis"), ("geom", "quat"), ("geom", "axisangle"), ("geom", "xyaxes"), ("site", "axisangle"), ("site", "xyaxes"), ("site", "zaxis"),
    # <position> / <motor> share the actuator record with <general>: gear / site are claimed there, force limits on <motor>
    ("position", "gear"), ("position", "site"), ("position", "forcelimited"), ("position", "forcerange"),
    ("general", "forcelimited"), ("general", "forcerange"),
}

# ---------------------------------------------------------------------------------------------------------------------------------
# perturbation rows: (tag, attribute, scene, text in the scene, replacement).  Each replaces ONE occurrence and must change the
# oracle's 50-step trajectory or its sensor readings.
# ---------------------------------------------------------------------------------------------------------------------------------
PERTURB = [
    ("compiler", "angle", "servo_arm", 'angle="radian"', 'angle="degree"'),
    ("compiler", "autolimits", "servo_arm", 'autolimits="true"', 'autolimits="false"'),
    ("option", "timestep", "servo_arm", 'timestep="0.004"', 'timestep="0.0035"'),
    ("option", "integrator", "servo_arm", 'integrator="Euler"', 'integrator="RK4"'),
    ("option", "integrator", "rk4_contact", 'integrator="RK4"', 'integrator="Euler"'),
    ("option", "iterations", "contact_mix", '<option timestep="0.003"/>', '<option timestep="0.003" iterations="1"/>'),
    ("option", "tolerance", "contact_mix", '<option timestep="0.003"/>', '<option timestep="0.003" tolerance="0.5"/>'),
    ("option", "gravity", "tendon_limits", 'gravity="0 0 -9.81"', 'gravity="0 0 -9"'),
    ("option", "density", "site_wrench", 'density="1.2"', 'density="50"'),
    ("option", "viscosity", "site_wrench", 'viscosity="0.05"', 'viscosity="2"'),
    ("body", "pos", "servo_arm", 'name="fore" pos="0.3 0 0"', 'name="fore" pos="0.3 0 0.02"'),
    ("body", "euler", "servo_arm", 'euler="0 0 0.4"', 'euler="0.3 0 0.4"'),
    ("body", "childclass", "servo_arm", 'childclass="limb"', ''),
    ("body", "xyaxes", "tendon_limits", 'xyaxes="1 0 0 0 0 1"', 'xyaxes="1 0 0 0 0.2 1"'),
    ("body", "quat", "contact_mix", 'quat="0.9914449 0 0 0.1305262"', 'quat="0.9914449 0.1305262 0 0"'),
    ("body", "axisangle", "contact_mix", 'axisangle="0 0 1 0.3"', 'axisangle="0 1 0 0.3"'),
    ("joint", "type", "rk4_contact", 'name="lift" type="slide"', 'name="lift" type="hinge"'),
    ("joint", "pos", "servo_arm", 'pos="0 0 0.01"', 'pos="0 0 0.05"'),
    ("joint", "axis", "servo_arm", 'name="wrist" class="limb" axis="0 0 1"', 'name="wrist" class="limb" axis="1 0 0"'),
    ("joint", "range", "servo_arm", 'range="-0.12 0.35"', 'range="-0.2 0.35"'),
    ("joint", "limited", "rk4_contact", 'stiffness="2" limited="true"', 'stiffness="2" limited="false"'),
    ("joint", "damping", "servo_arm", 'damping="0.4"', 'damping="0.9"'),
    ("joint", "stiffness", "servo_arm", 'stiffness="6"', 'stiffness="9"'),
    ("joint", "armature", "servo_arm", 'armature="0.02"', 'armature="0.2"'),
    ("joint", "margin", "servo_arm", 'margin="0.06"', 'margin="0.02"'),
    ("joint", "ref", "servo_arm", 'ref="0.3"', 'ref="0.1"'),
    ("joint", "springref", "servo_arm", 'springref="0.6"', 'springref="0.2"'),
    ("joint", "solreflimit", "servo_arm", 'solreflimit="0.03 0.9"', 'solreflimit="0.06 0.9"'),
    ("joint", "solimplimit", "servo_arm", 'solimplimit="0.8 0.99 0.004 0.6 2"', 'solimplimit="0.6 0.99 0.004 0.6 2"'),
    ("geom", "type", "contact_mix", 'name="ball_geom" type="sphere"', 'name="ball_geom" type="capsule"'),
    ("geom", "size", "servo_arm", 'size="0.03"', 'size="0.06"'),
    ("geom", "fromto", "servo_arm", 'fromto="0 0 0 0.3 0 0"', 'fromto="0 0 0 0.3 0 0.05"'),
    ("geom", "pos", "servo_arm", 'pos="0.08 0.02 0"', 'pos="0.12 0.02 0"'),
    ("geom", "density", "servo_arm", 'density="900"', 'density="1500"'),
    ("geom", "mass", "servo_arm", 'mass="0.3"', 'mass="0.5"'),
    ("geom", "euler", "contact_mix", 'euler="0.04 -0.03 0"', 'euler="0.1 -0.03 0"'),
    ("geom", "zaxis", "contact_mix", 'zaxis="1 0 0.025"', 'zaxis="1 0 0.2"'),
    ("geom", "contype", "contact_mix", 'contype="2" conaffinity="0"', 'contype="0" conaffinity="0"'),
    ("geom", "conaffinity", "contact_mix", 'conaffinity="6"', 'conaffinity="4"'),
    ("geom", "friction", "contact_mix", 'friction="0.9 0.01 0.0001"', 'friction="0.2 0.01 0.0001"'),
    ("geom", "solref", "contact_mix", 'solref="0.01 0.7"', 'solref="0.005 0.7"'),
    ("geom", "solimp", "contact_mix", 'solimp="0.8 0.99 0.003 0.3 2"', 'solimp="0.6 0.99 0.003 0.3 2"'),
    ("geom", "solmix", "contact_mix", 'solmix="3"', 'solmix="0.3"'),
    ("geom", "condim", "contact_mix", 'condim="3"', 'condim="1"'),
    ("geom", "margin", "contact_mix", 'margin="0.02"', 'margin="0.03"'),
    ("geom", "gap", "contact_mix", 'gap="0.012"', 'gap="0"'),
    ("site", "pos", "site_wrench", 'pos="0.03 -0.02 0.04"', 'pos="0.08 -0.02 0.04"'),
    ("site", "euler", "site_wrench", 'euler="10 -20 30"', 'euler="10 -20 60"'),
    ("site", "quat", "site_wrench", 'quat="0.9659258 0 0.258819 0"', 'quat="1 0 0 0"'),
    ("fixed", "limited", "tendon_limits", '<fixed name="coupling" limited="true"', '<fixed name="coupling" limited="false"'),
    ("fixed", "range", "tendon_limits", 'range="-0.12 0.1"', 'range="-0.12 0.05"'),
    ("fixed", "margin", "tendon_limits", 'margin="0.03"', 'margin="0.005"'),
    ("fixed", "solreflimit", "tendon_limits", 'solreflimit="0.02 1.1"', 'solreflimit="0.05 1.1"'),
    ("fixed", "solimplimit", "tendon_limits", 'solimplimit="0.9 0.96 0.003 0.5 2"', 'solimplimit="0.7 0.96 0.003 0.5 2"'),
    ("tendon/joint", "coef", "tendon_limits", 'coef="-0.7"', 'coef="-1"'),
    ("tendon/joint", "coef", "tendon_limits", 'coef="1.5"', 'coef="1"'),
    ("motor", "joint", "servo_arm", 'joint="wrist" gear="2"', 'joint="elbow" gear="2"'),
    ("motor", "gear", "servo_arm", 'gear="2"', 'gear="1.5"'),
    ("motor", "ctrllimited", "site_wrench", 'ctrllimited="true" ctrlrange="0 1"', 'ctrllimited="false" ctrlrange="0 1"'),
    ("motor", "ctrlrange", "servo_arm", 'ctrlrange="-1 1" forcelimited', 'ctrlrange="-0.5 1" forcelimited'),
    ("motor", "forcelimited", "servo_arm", 'forcelimited="true"', 'forcelimited="false"'),
    ("motor", "forcerange", "servo_arm", 'forcerange="-0.4 0.6"', 'forcerange="-0.4 0.3"'),
    ("motor", "site", "site_wrench", 'site="hub" gear="0 0 1', 'site="imu" gear="0 0 1'),
    ("position", "joint", "rk4_contact", '<position joint="knee"', '<position joint="hip"'),
    ("position", "kp", "servo_arm", 'kp="30"', 'kp="20"'),
    ("position", "kv", "servo_arm", 'kv="3"', 'kv="0"'),
    ("position", "ctrllimited", "rk4_contact", 'ctrlrange="-0.5 1.5" ctrllimited="true"', 'ctrlrange="-0.5 1.5" ctrllimited="false"'),
    ("position", "ctrlrange", "servo_arm", 'ctrlrange="-1.5 0.5"', 'ctrlrange="-1 0.5"'),
    ("general", "joint", "servo_arm", '<general name="affine" joint="elbow"', '<general name="affine" joint="wrist"'),
    ("general", "site", "site_wrench", '<general name="wrench" site="hub"', '<general name="wrench" site="imu"'),
    ("general", "gear", "site_wrench", 'gear="1 0.5 0.3 0.02 -0.03 0.05"', 'gear="1 0.5 0.3 0.02 -0.03 0.2"'),
    ("general", "gainprm", "servo_arm", 'gainprm="4"', 'gainprm="2"'),
    ("general", "biastype", "servo_arm", 'biastype="affine"', 'biastype="none"'),
    ("general", "biasprm", "servo_arm", 'biasprm="0.5 -2.5 -0.4"', 'biasprm="0.5 -2.5 0"'),
    ("general", "biasprm", "servo_arm", 'biasprm="0.5 -2.5 -0.4"', 'biasprm="0 -2.5 -0.4"'),
    ("general", "ctrllimited", "servo_arm", 'ctrllimited="true" ctrlrange="-0.8 1"', 'ctrllimited="false" ctrlrange="-0.8 1"'),
    ("general", "ctrlrange", "servo_arm", 'ctrlrange="-0.8 1"', 'ctrlrange="-0.8 0.3"'),
    ("jointpos", "joint", "rk4_contact", 'joint="knee"/>', 'joint="hip"/>'),
    ("gyro", "site", "site_wrench", '<gyro name="gyro" site="imu"/>', '<gyro name="gyro" site="hub"/>'),
    ("accelerometer", "site", "site_wrench", '<accelerometer name="acc" site="imu"/>', '<accelerometer name="acc" site="hub"/>'),
    ("framequat", "objname", "site_wrench", 'objname="imu"', 'objname="hub"'),
    ("exclude", "body1", "contact_mix", 'body1="ball" body2="rod"', 'body1="box" body2="rod"'),
    ("exclude", "body2", "contact_mix", 'body1="ball" body2="rod"', 'body1="ball" body2="box"'),
]


def perturbed(row) -> str:
    """The scene's XML with the row's replacement applied (the text must occur exactly once)."""
    tag, attr, scene, old, new = row
    xml = SCENES[scene].xml
    assert xml.count(old) == 1, (tag, attr, scene, old)
    return xml.replace(old, new)


def attrs_in_xml(xml: str) -> set:
    """Every (schema tag, attribute) written in the XML (a <joint> inside <tendon> is "tendon/joint")."""
    import xml.etree.ElementTree as ET

    out = set()

    def walk(e, where):
        key = "tendon/joint" if (e.tag == "joint" and where == "tendon") else e.tag
        out.update((key, a) for a in e.attrib)
        for c in e:
            walk(c, "tendon" if e.tag in ("tendon", "fixed") else e.tag)

    walk(ET.fromstring(xml), "")
    return out

