"""Test data of the step-invariant tests (tests/test_gpu_step_invariants.py, tests/test_step_invariants_hostemu.py); no reference model.

  GUARD_XML   a weight on a vertical slide and a rod on a hinge, both hanging from the world, one motor each, under a gravity of
              3e5 m/s^2: 8 lanes per environment, so one pass of random controls serves 8 / 2 = 4 steps.  A falling weight is the
              one state that can sit AT the bad-state bound (|x| <= 1e10, exactly representable in fp32) and be carried past it by
              one ordinary step: a pure translation has no velocity-dependent forces, its acceleration is gravity (far below the
              bound, so the acceleration guard stays quiet), and 0.01 s of it is 3000 m/s - three fp32 ulps (1024) of the bound.  So
              with the weight's velocity at -1e10 the first step runs from a good state, and the qvel guard fires at the top of the
              SECOND step: the second step of a pass.
"""
import numpy as np

GUARD_XML = """<mujoco model="guard"><option timestep="0.01" gravity="0 0 -3e5"/>
  <default><joint damping="0" armature="0.01"/><geom type="sphere" size="0.05" density="1000" contype="0" conaffinity="0"/></default>
  <worldbody>
    <body name="weight" pos="0 0 1"><joint name="fall" type="slide" axis="0 0 1"/><geom/></body>
    <body name="rod" pos="1 0 1"><joint name="swing" type="hinge" axis="0 1 0"/><geom pos="0 0 -0.001"/></body>
  </worldbody>
  <actuator><motor name="mf" joint="fall" ctrllimited="true" ctrlrange="-1 1"/><motor name="ms" joint="swing" ctrllimited="true" ctrlrange="-0.5 2"/></actuator>
</mujoco>"""

BAD_BOUND = 1e10                    # group_bad: |x| <= 1e10 is a good value


def poisoned_state(batch, victim):
    """(qpos, qvel) [batch, 2]: small values everywhere, the victim's weight falling at the bound."""
    rng = np.random.default_rng(12)
    q = rng.normal(size=(batch, 2)) * 0.001
    v = rng.normal(size=(batch, 2)) * 0.5
    v[victim, 0] = -BAD_BOUND
    return q, v
