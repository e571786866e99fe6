"""Output feedback end to end on the GPU: the cart-pole with jointpos sensors on both joints, balanced from its two sensor readings.

``linearize_rollout(T = 1, sensor_derivatives=True)`` at the upright set-point -> ``solve_dare`` (control gain K) -> ``solve_kalman``
(predictor gain L) -> 300 steps of ``u = -K xhat``, ``xhat+ = A xhat + B u + L (y - C xhat - D u)`` in torch on ``DeviceData``, with
``xhat0 = 0`` and ``y`` the sensordata each step leaves (the sensors of its forward pass: those of the state before the step).

The weights were checked on the CPU first, with the oracle's finite differences, scipy's Riccati solutions and the oracle's ``step``:
rho(A - B K) = 0.975, rho(A - L C) = 0.904, |hinge| after 300 steps 6e-4 of its initial value for offsets 0.02 .. 0.05 rad.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.fd_sensors_common import cartpole_sensors_xml  # noqa: E402

Q, R = np.diag([100.0, 100.0, 1.0, 1.0]), np.eye(1) * 1e-4
W, V = np.diag([1e-2, 1e-2, 1.0, 1.0]), np.eye(2) * 1e-4


def test_cartpole_balances_from_its_sensors():
    import torch

    import mujoco_template_amd as mt
    from mujoco_template_amd import DeviceData, mj

    mm = mj.MjModel.from_xml_string(cartpole_sensors_xml())
    Bn, nsteps = 4, 300
    data = mj.MjData(mm, batch=Bn, dtype="float64")
    sim = data.sim
    opt = dict(dtype=torch.float64, device="cuda")
    x_up = torch.zeros((Bn, 5), **opt)                                            # time | slider, hinge | their velocities: upright, at rest
    _, _, A, Bm, C, D = mt.linearize_rollout(mm, data, torch.zeros((Bn, 1, 1), **opt), initial_state=x_up, sensor_derivatives=True)
    A, Bm, C, D = (x[:, 0].contiguous() for x in (A, Bm, C, D))
    ctrl_sol = mt.solve_dare(data, A, Bm, torch.as_tensor(Q, **opt), torch.as_tensor(R, **opt))
    est_sol = mt.solve_kalman(data, A, C, torch.as_tensor(W, **opt), torch.as_tensor(V, **opt))
    K, L = ctrl_sol.K, est_sol.L
    assert ctrl_sol.status.cpu().tolist() == [0] * Bn and est_sol.status.cpu().tolist() == [0] * Bn
    rho_k = mt.closed_loop_poles(data, A, Bm, K).rho
    rho_l = mt.closed_loop_poles(data, A.mT, C.mT, L.mT).rho
    print(f"rho(A - B K) {rho_k.cpu().tolist()}  rho(A - L C) {rho_l.cpu().tolist()}")
    assert bool((rho_k < 0.98).all()) and bool((rho_l < 0.98).all())

    hinge0 = torch.tensor([0.02, 0.03, 0.04, 0.05], **opt)
    dev = DeviceData(data)
    sim.use_torch_stream()
    dev.qpos.zero_(); dev.qvel.zero_(); dev.qacc_warmstart.zero_()
    dev.qpos[:, 1] = hinge0
    xhat = torch.zeros((Bn, 4, 1), **opt)
    err0 = (xhat[..., 0] - torch.cat([dev.qpos, dev.qvel], dim=1)).abs().amax(dim=1)
    for _ in range(nsteps):
        u = -(K @ xhat)                                                           # [B, 1, 1]
        dev.ctrl.copy_(u[..., 0])
        sim.step(1)
        y = dev.sensordata[..., None]                                             # the sensors of this step's forward pass
        xhat = A @ xhat + Bm @ u + L @ (y - C @ xhat - D @ u)
    torch.cuda.synchronize()
    x = torch.cat([dev.qpos, dev.qvel], dim=1)
    hinge, err = dev.qpos[:, 1].abs(), (xhat[..., 0] - x).abs().amax(dim=1)
    print(f"|hinge| {hinge.cpu().tolist()} of {hinge0.cpu().tolist()};  |xhat - dx| {err.cpu().tolist()} of {err0.cpu().tolist()}")
    assert bool((hinge < 0.1 * hinge0).all()) and bool((err < 0.1 * err0).all())
