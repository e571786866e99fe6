"""Timing of the batched finite-difference linearisation (mjd_transitionFD, float64 on device) and Jacobians.

``--points``: ``transition_fd_points`` without and with the sensor Jacobians (a sensors column), and ``solve_kalman`` beside ``solve_dare``."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mujoco_template_amd.mjcf import compile_xml_path
from mujoco_template_amd._capi import BatchSim, DeviceModel, CTRL_RANDOM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for name, B, scale in () if "--points" in sys.argv else (("cartpole", 512, 0.01), ("cartpole", 4096, 0.01), ("drone2/scene", 2048, 0.3), ("humanoid", 64, 1.0), ("humanoid", 512, 1.0)):
    cm = compile_xml_path(os.path.join(ROOT, f"models/{name}.xml"))
    sim = BatchSim(DeviceModel(cm), B, dtype="float64")
    sim.rollout(100, CTRL_RANDOM, seed=1, ctrl_scale=scale); sim.sync()
    sim.transition_fd(1e-6, True)
    t = time.time(); n = 5
    for _ in range(n):
        A, Bm = sim.transition_fd(1e-6, True, copy=False)          # the call the Python front makes (mjd_transitionFD copies once, into the caller's arrays)
    dt = (time.time() - t) / n
    t = time.time()
    for _ in range(n):
        sim.transition_fd(1e-6, True, copy=True)
    dtc = (time.time() - t) / n
    ncol = 1 + 2 * (2 * cm.nv + cm.nu)
    print(f"{name:14s} B={B:5d}: transition_fd {dt*1e3:8.2f} ms per call = {B/dt:.3e} linearisations/s = {B*ncol/dt:.3e} perturbed env-steps/s (float64, {ncol} columns; {dtc*1e3:.2f} ms with a host copy of A/B), A {A.shape} B {Bm.shape}", flush=True)


# ---- transition_fd_points with and without the sensor Jacobians (C, D), and solve_kalman beside solve_dare ------------------------------
# HIP events around windows of back-to-back calls, each window at least 30 ms; the median and the spread (min .. max) of the windows.
def _windows(torch, call, nwin=7, min_ms=30.0):
    call(); torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); call(); t1.record(); torch.cuda.synchronize()
    reps = max(2, int(min_ms / max(t0.elapsed_time(t1), 1e-3)) + 1)
    out = []
    for _ in range(nwin):
        t0.record()
        for _ in range(reps):
            call()
        t1.record(); torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / reps)
    out.sort()
    return out[len(out) // 2], out[0], out[-1], reps


def points_timing():
    import inspect

    import torch

    import mujoco_template_amd as mt

    has_sensors = "sensors" in inspect.signature(BatchSim.transition_fd_points).parameters
    print(f"{'model':14s} {'points':>6s} {'plain ms (min .. max)':>28s} {'sensors ms (min .. max)':>28s} {'sensors / plain':>16s}")
    for name, B, scale in (("drone2/scene", 4096, 0.3), ("humanoid", 512, 1.0)):
        cm = compile_xml_path(os.path.join(ROOT, f"models/{name}.xml"))
        sim = BatchSim(DeviceModel(cm), B, dtype="float64")
        sim.rollout(100, CTRL_RANDOM, seed=1, ctrl_scale=scale); sim.sync()
        sim.use_torch_stream()
        q, v, u, w = (sim.torch_view(k) for k in ("qpos", "qvel", "ctrl", "qacc_warmstart"))
        plain_out = sim.transition_fd_points(q, v, u, w)
        p = _windows(torch, lambda: sim.transition_fd_points(q, v, u, w, out=plain_out))
        row = f"{name:14s} {B:6d} {p[0]:10.3f} ({p[1]:.3f} .. {p[2]:.3f})"
        if has_sensors and cm.nsensordata > 0:
            sens_out = sim.transition_fd_points(q, v, u, w, sensors=True)
            s = _windows(torch, lambda: sim.transition_fd_points(q, v, u, w, out=sens_out, sensors=True))
            row += f" {s[0]:10.3f} ({s[1]:.3f} .. {s[2]:.3f}) {s[0] / p[0]:16.3f}"
        else:
            row += f" {'-':>28s} {'-':>16s}"
        print(row, flush=True)
    if hasattr(mt, "solve_kalman"):
        nx, ny, nb = 12, 10, 4096
        rng = np.random.default_rng(0)
        M = rng.normal(size=(nb, nx, nx))
        A = M * (rng.uniform(0.9, 1.05, nb) / np.abs(np.linalg.eigvals(M)).max(axis=1))[:, None, None]
        C = rng.normal(size=(nb, ny, nx))
        dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")    # noqa: E731
        At, Ct, W, V = dev(A), dev(C), dev(np.eye(nx)), dev(np.eye(ny))
        Atr, Ctr = At.mT.contiguous(), Ct.mT.contiguous()
        sim = BatchSim(DeviceModel(compile_xml_path(os.path.join(ROOT, "models/cartpole.xml"))), 1, dtype="float64")
        d = _windows(torch, lambda: mt.solve_dare(sim, Atr, Ctr, W, V))
        k = _windows(torch, lambda: mt.solve_kalman(sim, At, Ct, W, V))
        print(f"solve_dare ({nx}, {ny}) x {nb}: {d[0]:.3f} ms ({d[1]:.3f} .. {d[2]:.3f});  solve_kalman (the two transposes included): "
              f"{k[0]:.3f} ms ({k[1]:.3f} .. {k[2]:.3f})", flush=True)


if "--points" in sys.argv:
    points_timing()
