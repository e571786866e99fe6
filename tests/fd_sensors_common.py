"""Shared by the sensor-Jacobian tests: the test-local models and the expected ``C = d sensordata / d x``, ``D = d sensordata / d u``.

The oracle has no sensor derivatives.  The expectation is the definition, as a numpy loop over ``oracle.mjo.OracleData``: for every
column restore (qpos, qvel, ctrl, qacc_warmstart), perturb (``integrate_pos`` for a dq column, the ctrlrange rule of ``B`` for a ctrl
column), ``step(1)``, read ``sensordata``; then difference the sensor vectors as they are - centred where both sides are valid,
one-sided where one is, 0 where none.
"""
import numpy as np

from oracle import mjo
from tests.conftest import MODELS


def cartpole_sensors_xml() -> str:
    """models/cartpole.xml plus jointpos sensors on both joints."""
    xml = open(MODELS["cartpole"]).read()
    return xml.replace("</mujoco>", '  <sensor>\n    <jointpos name="slider_pos" joint="slider"/>\n    <jointpos name="hinge_pos" joint="hinge"/>\n'
                                    "  </sensor>\n</mujoco>")


# An RK4 hinge with a jointpos and a gyro: a step leaves the sensors of RK4's FOURTH forward pass in sensordata (mj_step), so the
# jointpos row of C is not the unit row here (it is 1 + O(h^2) over dq and ~h over dv): this model decides where the kernel's store sits.
RK4_HINGE = """<mujoco model="rk4_hinge">
  <option timestep="0.005" integrator="RK4"/>
  <worldbody>
    <body name="arm" pos="0 0 1">
      <joint name="pivot" type="hinge" axis="0 1 0" damping="0.1"/>
      <geom type="capsule" size="0.03" fromto="0 0 0 0.3 0 0"/>
      <site name="imu" pos="0.3 0 0" euler="0 0 20"/>
    </body>
  </worldbody>
  <actuator><motor joint="pivot" gear="2" ctrllimited="true" ctrlrange="-1 1"/></actuator>
  <sensor>
    <jointpos name="angle" joint="pivot"/>
    <gyro name="rate" site="imu"/>
  </sensor>
</mujoco>
"""


def oracle_sensor_fd(om, cm, qpos, qvel, ctrl, warmstart, eps=1e-6, centered=True):
    """(C [ns, 2nv], D [ns, nu]) of ONE environment about (qpos, qvel, ctrl, warmstart)."""
    od = mjo.OracleData(om)
    nv, nu, ns = cm.nv, cm.nu, cm.nsensordata
    q0, v0, u0, w0 = (np.array(x, dtype=np.float64) for x in (qpos, qvel, ctrl, warmstart))
    lim = np.asarray(cm.arrays["actuator_ctrllimited"]).astype(bool).reshape(-1) if nu else np.zeros(0, dtype=bool)
    rng = np.reshape(np.asarray(cm.arrays["actuator_ctrlrange"], dtype=np.float64), (-1, 2)) if nu else np.zeros((0, 2))

    def run(q, v, u):
        od.qpos[:] = q; od.qvel[:] = v; od.qacc_warmstart[:] = w0; od.time = 0.0
        if nu:
            od.ctrl[:] = u
        od.step(1)
        return np.array(od.sensordata, dtype=np.float64)

    s0 = run(q0, v0, u0)
    out = np.zeros((ns, 2 * nv + nu))
    for k in range(2 * nv + nu):
        side = {}
        for sgn in (1.0, -1.0) if centered else (1.0,):
            q, v, u = q0.copy(), v0.copy(), u0.copy()
            if k < nv:
                e = np.zeros(nv); e[k] = 1.0
                q = od.integrate_pos(q0, e, sgn * eps)
            elif k < 2 * nv:
                v[k - nv] += sgn * eps
            else:
                a = k - 2 * nv
                val = u0[a] + sgn * eps
                if lim[a] and (val < rng[a, 0] or val > rng[a, 1]):
                    continue                                     # the nudge would leave ctrlrange: one-sided
                u[a] = val
            side[sgn] = run(q, v, u)
        if 1.0 in side and -1.0 in side:
            out[:, k] = (side[1.0] - side[-1.0]) / (2 * eps)
        elif 1.0 in side:
            out[:, k] = (side[1.0] - s0) / eps
        elif -1.0 in side:
            out[:, k] = (s0 - side[-1.0]) / eps
    return out[:, :2 * nv], out[:, 2 * nv:]
