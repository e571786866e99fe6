"""Records tests/golden/dare_humanoid.npz: A [54, 54], B [54, 21], Q [54, 54], R [21, 21] (float64) of the tutorial's humanoid balance
design - DeepMind's LQR tutorial on models/humanoid.xml, built with the project's float64 oracle on the CPU exactly as
tests/test_oracle_anchors.py::test_oracle_humanoid_keeps_its_one_leg_balance_under_the_tutorial_lqr builds it (inverse-dynamics height
sweep, set-point ctrl0, the oracle's transition_fd, COM-over-foot Jacobian cost).  tests/dare_common.py::humanoid_case reads it.

    python tests/golden/make_dare_humanoid.py [OUT]      # no GPU; a minute of CPU

The design is the hard case of mjb_lqr_dare: open-loop spectral radius 1.056, and a closed loop that keeps unit-modulus modes (the
unweighted root dofs are marginal), on which the plain Riccati recursion has not converged after 20 000 steps.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "dare_humanoid.npz")


def design():
    from mujoco_template_amd import mj
    from mujoco_template_amd.mjcf import compile_xml_path
    from oracle import mjo

    cm = compile_xml_path(os.path.join(ROOT, "models", "humanoid.xml"))
    d = mjo.OracleData(mjo.OracleModel(cm))
    nv, nu = cm.nv, cm.nu
    model = mj.MjModel(cm)
    offs = np.linspace(-1e-3, 1e-3, 2001)
    fz = np.zeros_like(offs)
    for i, o in enumerate(offs):
        d.reset_keyframe(1); d.forward(); d.qacc[:] = 0; d.qpos[2] += o; d.inverse(); fz[i] = d.qfrc_inverse[2]
    best = float(offs[np.argmin(np.abs(fz))])
    d.reset_keyframe(1); d.forward(); d.qacc[:] = 0; d.qpos[2] += best; d.inverse()
    qfrc0 = d.qfrc_inverse.copy()
    ctrl0 = (qfrc0[None] @ np.linalg.pinv(np.array(d.actuator_moment).reshape(nu, nv))).ravel()
    d.qvel[:] = 0; d.ctrl[:] = ctrl0; d.forward()
    A, B = d.transition_fd(1e-6, True)
    jd = d.jac(3, model.body("torso").id)[0] - d.jac(2, model.body("foot_left").id)[0]
    joint = [model.joint(j).name for j in range(cm.njnt)]
    bal = np.array(sorted(int(cm.arrays["jnt_dofadr"][j]) for j, n in enumerate(joint) if "z" not in n and
                          ("abdomen" in n or ("left" in n and any(t in n for t in ("hip", "knee", "ankle"))))))
    other = np.setdiff1d(np.arange(6, nv), bal)
    Qj = np.eye(nv); Qj[:6, :6] = 0; Qj[bal, bal] = 3.0; Qj[other, other] = 0.3
    Q = np.zeros((2 * nv, 2 * nv)); Q[:nv, :nv] = 1000.0 * jd.T @ jd + Qj
    Q = 0.5 * (Q + Q.T)
    return np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64), Q, np.eye(nu)


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    A, B, Q, R = design()
    assert A.shape == (54, 54) and B.shape == (54, 21)
    np.savez_compressed(out, A=A, B=B, Q=Q, R=R)
    print(f"{out}: {os.path.getsize(out)} bytes, open-loop spectral radius {np.abs(np.linalg.eigvals(A)).max():.4f}")
