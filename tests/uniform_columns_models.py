"""Small models for the uniform-column tests (tests/test_uniform_columns_host.py, tests/test_gpu_uniform_columns.py): the smallest
shapes at which a wrongly folded record column can show.  Every model has at least two records in the tables it is about, since a
column of one record is never a constant of the specialised kernel."""
import numpy as np

LIMIT = 'solreflimit="0.02 1" solimplimit="0.9 0.95 0.001 0.5 2"'


def arm_xml(*, limit2=LIMIT, ctrlrange2="-1 1", quat1="1 0 0 0", quat2="1 0 0 0", ctrlrange1="-1 1"):
    """Two limited hinges in a chain with identical limit parameters, damping and control ranges: every column of lim_f, dof_frec,
    actuator_ctrlrange, actuator_gainprm and body_quat that the defaults fill is uniform.  The keyword arguments break one of them."""
    return f"""<mujoco><compiler angle="radian"/><option timestep="0.004"/><worldbody>
  <body pos="0 0 1" quat="{quat1}"><joint name="j1" type="hinge" axis="0 1 0" limited="true" range="-0.5 0.5" margin="0.01" damping="0.1" {LIMIT}/>
    <geom type="capsule" size="0.03" fromto="0 0 0 0.3 0 0" contype="0" conaffinity="0"/>
    <body pos="0.3 0 0" quat="{quat2}"><joint name="j2" type="hinge" axis="0 1 0" limited="true" range="-0.5 0.5" margin="0.01" damping="0.1" {limit2}/>
      <geom type="capsule" size="0.03" fromto="0 0 0 0.3 0 0" contype="0" conaffinity="0"/></body></body>
</worldbody><actuator><motor joint="j1" gear="1" ctrllimited="true" ctrlrange="{ctrlrange1}"/>
  <motor joint="j2" gear="1" ctrllimited="true" ctrlrange="{ctrlrange2}"/></actuator></mujoco>"""


ROT = "0.9238795325 0 0.3826834324 0"       # 45 degrees about y

ARM_CASES = {
    "uniform": arm_xml(),
    "solimp_mid_power": arm_xml(limit2='solreflimit="0.02 1" solimplimit="0.9 0.95 0.001 0.3 1"'),
    "ctrlrange": arm_xml(ctrlrange2="-0.25 0.5"),
    "second_body_rotated": arm_xml(quat2=ROT),
    "first_body_rotated": arm_xml(quat1=ROT),
}


def arm_start(B):
    """Both joints past a limit (upper for even environments, lower for odd ones), moving further in: limit rows from the first step."""
    q = np.empty((B, 2)); v = np.empty((B, 2))
    for e in range(B):
        s = 1.0 if e % 2 == 0 else -1.0
        q[e] = (s * (0.55 + 0.01 * e), -s * (0.6 + 0.02 * e))
        v[e] = (s * 0.5, -s * 0.3)
    return q, v


def spheres_xml(*, margin2="0.02", friction2="1 0.005 0.0001", n=2):
    """n free spheres over a plane (and each other): n plane pairs and n (n - 1) / 2 sphere pairs with one margin and one friction,
    unless the second sphere's are changed."""
    bodies = ""
    for i in range(n):
        extra = f'margin="{margin2}" friction="{friction2}"' if i == 1 else 'margin="0.02"'
        bodies += f'<body pos="{0.25 * i} 0 0.1"><freejoint/><geom type="sphere" size="0.1" {extra}/></body>\n'
    return f"""<mujoco><option timestep="0.004"/><worldbody><geom name="floor" type="plane" size="0 0 1" margin="0.02"/>
{bodies}</worldbody></mujoco>"""


SPHERE_CASES = {
    "uniform": spheres_xml(),
    "margin_friction": spheres_xml(margin2="0.05", friction2="1.5 0.005 0.0001"),
}


def spheres_start(B, cm, *, spacing=0.25, n=2):
    """Resting height with a small penetration, neighbours closer than two radii apart for some of them: plane and sphere contacts
    from the first step."""
    q = np.tile(np.array(cm.qpos0, dtype=np.float64), (B, 1))
    v = np.zeros((B, cm.nv))
    for e in range(B):
        for i in range(n):
            q[e, 7 * i] = (spacing - 0.06 - 0.005 * e) * i           # 0.19 .. apart: overlapping spheres (radius 0.1)
            q[e, 7 * i + 2] = 0.098 - 0.001 * e
            v[e, 6 * i + 2] = -0.1
    return q, v


# more broad-phase survivors than lanes: 5 spheres in a tight row on the floor at G = 8 lanes - 5 plane pairs + 10 sphere pairs (two
# chunks of candidates), of which the 5 plane pairs and the 4 pairs of neighbours survive the bounding test: 9 survivors against 8
# slots, so the survivor list is flushed inside the loop and again at its end.  CROWD_CAPS keep 8 environments' LDS under the limit.
CROWD_CAPS = dict(lanes=8, nconmax=12, nefcmax=48)
CROWD_CAPS_DROP = dict(lanes=8, nconmax=6, nefcmax=24)            # ... and with fewer contact slots than contacts
CROWD_N = 5


def crowd_xml():
    return spheres_xml(n=CROWD_N)


def crowd_start(B, cm):
    return spheres_start(B, cm, spacing=0.25, n=CROWD_N)
