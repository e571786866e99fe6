"""Synthetic models with 33 to 64 dofs: the range where the step kernel leaves its nv <= 32 register paths (MFMA sweep / Cholesky,
reg_factor32, the split J^T f) for the register-tiled Cholesky on an 8x8 lane grid (tile_factor) with chol_solve, and where the
64-bit dof masks fill up to bit 63.  Test data only; none of them is a reference model.

  chain_xml(n)   tests.conftest.chain_xml: a serial hinge chain with joint limits whose last four links touch the floor
  tree_xml()     a branching tree of 45 dofs: a sliding / pitching base with six limbs of hinges and slides, damping (the implicit
                 M + h diag(damping) factor), armature, stiffness with springref, a limited fixed tendon, position actuators
  two_free_xml() two free bodies plus 52 hinges = 64 dofs; the second free body is the last one, so its joint owns dofs 58..63
"""
import numpy as np

from tests.conftest import chain_xml  # noqa: F401  (re-exported: the chains of 33..64 links are built by the same generator)

CHAIN_SIZES = (33, 40, 57, 64)


def pitched_chain_qpos(n, rng=None, noise=0.01, z_tip=0.02):
    """qpos of chain_xml(n) pitched down about the first hinge, with the last four links bent back to horizontal so that they lie
    1 cm deep in the floor (link radius 0.03): two contacts per link, 32 contact rows.  The random part only turns the vertical
    (odd) hinges: noise on the pitch hinges adds up along a long chain and lifts the tip off the floor."""
    j = n - 4 if (n - 4) % 2 == 0 else n - 3                 # the last pitch (y-axis) hinge before the tip
    th = np.arcsin((0.3 - z_tip) / (0.1 * j))
    q = np.zeros(n)
    if rng is not None:
        q[1::2] += rng.normal(size=n // 2) * noise
    q[0] += th
    q[j] -= th
    return q


def tree_xml(limbs=6, links=7):
    """Base with a slide along x, a slide along z and a pitch hinge (3 dofs), then `limbs` limbs of `links` joints each, splayed out
    around the base and bent towards the floor so that every foot can touch it.  Every third joint of a limb is a slide along the
    limb; the others are hinges about alternating axes.  nv = 3 + limbs * links (45 by default)."""
    s = ['<mujoco model="tree"><option timestep="0.004"/>',
         '<default><joint armature="0.05" damping="0.4" limited="true" range="-40 40"/>',
         '<geom type="capsule" size="0.025" contype="1" conaffinity="0" density="600"/></default>',
         '<worldbody><geom name="floor" type="plane" size="5 5 0.1" contype="1" conaffinity="1"/>',
         '<body name="base" pos="0 0 0.22">',
         '<joint name="bx" type="slide" axis="1 0 0" limited="false" damping="1"/>',
         '<joint name="bz" type="slide" axis="0 0 1" limited="false" damping="1"/>',
         '<joint name="by" type="hinge" axis="0 1 0" limited="false" damping="0.5"/>',
         '<geom type="box" size="0.12 0.12 0.04" contype="0"/>']
    for l in range(limbs):
        yaw = 360.0 * l / limbs
        c, sn = np.cos(np.radians(yaw)), np.sin(np.radians(yaw))
        s.append(f'<body name="l{l}" pos="{0.12 * c:.6f} {0.12 * sn:.6f} 0" euler="0 0 {yaw:.3f}">')
        for k in range(links):
            pos = "0 0 0" if k == 0 else "0.07 0 -0.03"
            if k % 3 == 2:
                jt = f'<joint name="l{l}j{k}" type="slide" axis="1 0 0" range="-0.03 0.03" stiffness="40" springref="0.01"/>'
            else:
                ax = "0 1 0" if k % 2 == 0 else "0 0 1"
                extra = ' stiffness="2" springref="5"' if k == 1 else ""
                jt = f'<joint name="l{l}j{k}" type="hinge" axis="{ax}"{extra}/>'
            ct = 1 if k == links - 1 else 0
            s.append(f'<body name="l{l}b{k}" pos="{pos}">{jt}<geom fromto="0 0 0 0.07 0 -0.03" contype="{ct}"/>')
        s.append("</body>" * (links + 1))
    s.append("</body></worldbody>")
    s.append('<tendon><fixed name="couple" limited="true" range="-0.05 0.05"><joint joint="l0j0" coef="1"/><joint joint="l3j0" coef="-1"/></fixed></tendon>')
    s.append("<actuator>")
    for l in range(limbs):
        s.append(f'<position name="p{l}" joint="l{l}j0" kp="20" ctrllimited="true" ctrlrange="-0.5 0.5"/>')
        s.append(f'<motor name="m{l}" joint="l{l}j3" gear="1" ctrllimited="true" ctrlrange="-1 1"/>')
    s.append('<motor name="mb" joint="bx" gear="5" ctrllimited="true" ctrlrange="-1 1"/>')
    s.append("</actuator></mujoco>")
    return "\n".join(s)


def two_free_xml(limbs=4, links=13):
    """A free torso with `limbs` hinge limbs of `links` joints (6 + 52 dofs), then a free box that rests on the floor: its free joint
    is the last joint of the model, so dof 63 (the top bit of every 64-bit dof mask) belongs to it."""
    s = ['<mujoco model="two-free"><option timestep="0.004"/>',
         '<default><joint type="hinge" armature="0.02" damping="0.2" limited="true" range="-30 30"/>',
         '<geom type="capsule" size="0.02" contype="1" conaffinity="0" density="500"/></default>',
         '<worldbody><geom name="floor" type="plane" size="5 5 0.1" contype="1" conaffinity="1"/>',
         '<body name="torso" pos="0 0 0.5"><freejoint name="torso"/><geom type="sphere" size="0.08" contype="0"/>']
    for l in range(limbs):
        yaw = 360.0 * l / limbs
        s.append(f'<body name="a{l}" pos="0 0 0" euler="0 0 {yaw:.3f}">')
        for k in range(links):
            pos = "0.08 0 0" if k == 0 else "0.045 0 -0.03"
            ax = "0 1 0" if k % 2 == 0 else "1 0 0"
            ct = 1 if k == links - 1 else 0
            s.append(f'<body name="a{l}b{k}" pos="{pos}"><joint name="a{l}j{k}" axis="{ax}"/><geom fromto="0 0 0 0.045 0 -0.03" contype="{ct}"/>')
        s.append("</body>" * (links + 1))
    s.append('</body><body name="box" pos="0.9 0 0.055"><freejoint name="box"/><geom type="box" size="0.06 0.06 0.06" contype="1"/></body>')
    s.append("</worldbody><actuator>")
    for l in range(limbs):
        s.append(f'<motor name="m{l}" joint="a{l}j0" gear="1" ctrllimited="true" ctrlrange="-1 1"/>')
    s.append("</actuator></mujoco>")
    return "\n".join(s)


LARGE_MODELS = {f"chain{n}": (lambda n=n: chain_xml(n)) for n in CHAIN_SIZES}
LARGE_MODELS.update({"tree": tree_xml, "two_free": two_free_xml})


def initial_state(cm, name, rng):
    """(qpos, qvel) in floor contact: pitched chains, the tree with its feet 5 mm in the floor, the torso above a box 5 mm in the floor."""
    if name.startswith("chain"):
        q = pitched_chain_qpos(cm.nv, rng)
    else:
        q = np.array(cm.qpos0, dtype=np.float64)
        hinge = np.ones(cm.nq, dtype=bool)
        if name == "two_free":
            hinge[:7] = False; hinge[-7:] = False                # the two free joints keep their qpos0 (positions, unit quaternions)
        q[hinge] += rng.normal(size=int(hinge.sum())) * 0.02
        if name == "tree":
            q[3] += 0.04; q[24] -= 0.04                           # l0j0 - l3j0 beyond the tendon's range: its limit row is active
    return q, rng.normal(size=cm.nv) * 0.1
