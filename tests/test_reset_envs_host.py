"""Per-environment reset without a GPU: the device function behind ``k_reset_envs`` (``mjb_device.hpp`` ``reset_env_state``) compiled for
the host (``tests/reset_envs_host.cpp``, g++ -DMJB_HOST_EMU) against a numpy reference - Philox4x32-10 draws (the algorithm of
``controllers.philox_uniform``, counter word 3 = 1 for qpos, 2 for qvel) and ``DeviceModel.integrate_pos`` - plus the decision rule
for device-array controllers."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from mujoco_template_amd import ConfigError, ControllerCapabilities, LinearFeedbackController, RandomCtrlController, ZeroController
from mujoco_template_amd.control import device_ctrl_mode_of, uses_device_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "mujoco_template_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("reset_envs") / "libreset_envs_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "reset_envs_host.cpp")])
    lib = ctypes.CDLL(so)
    vp, ci, cu, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_double
    for fn in (lib.reset_envs_f64, lib.reset_envs_f32):
        fn.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, cu, cd, cd, cu, vp, vp, vp, vp, vp, vp, vp]
        fn.restype = ci
    return lib


def philox_u(seed: int, c0, c1, c2, c3) -> np.ndarray:
    """u in [0, 1): Philox4x32-10 keyed (seed, 0x5EED), counter (c0, c1, c2, c3), first word >> 8 / 2^24 (controllers.philox_uniform)."""
    mask = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & mask for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = seed & 0xFFFFFFFF, 0x5EED
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & mask, p1 & mask,
                          ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & mask, p0 & mask)
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return (c0 >> np.uint64(8)).astype(np.float64) / 16777216.0


def reference(dm, cm, key: int, seed: int, qn: float, qv: float, genv: np.ndarray, episode: np.ndarray):
    """numpy + mj_integratePos: the float64 state of each (global env, episode)."""
    B = genv.size
    base_q = np.asarray(cm.arrays["qpos0"], dtype=np.float64) if key < 0 else np.reshape(cm.arrays["key_qpos"], (-1, cm.nq))[key]
    base_v = np.zeros(cm.nv) if key < 0 else np.reshape(cm.arrays["key_qvel"], (-1, cm.nv))[key]
    base_c = np.zeros(cm.nu) if key < 0 else np.reshape(cm.arrays["key_ctrl"], (-1, cm.nu))[key]
    i = np.arange(cm.nv)[None, :]
    qpos = np.ascontiguousarray(np.tile(base_q, (B, 1)))
    if qn != 0:
        dq = qn * (2.0 * philox_u(seed, genv[:, None], episode[:, None], i, 1) - 1.0)
        dm.integrate_pos(qpos, np.ascontiguousarray(dq), 1.0)
    qvel = base_v[None, :] + (qv * (2.0 * philox_u(seed, genv[:, None], episode[:, None], i, 2) - 1.0) if qv != 0 else 0.0)
    return qpos, np.broadcast_to(qvel, (B, cm.nv)).copy(), np.tile(base_c, (B, 1))


def run(lib, cm, dtype, key, seed, qn, qv, env0, mask, episode, B):
    a = cm.arrays
    ints = [np.ascontiguousarray(a[k], dtype=np.int32) for k in ("jnt_type", "jnt_qposadr", "jnt_dofadr")]
    if key < 0:
        bq, bv, bc = np.ascontiguousarray(a["qpos0"], dtype=np.float64), None, None
    else:
        bq = np.ascontiguousarray(np.reshape(a["key_qpos"], (-1, cm.nq))[key])
        bv = np.ascontiguousarray(np.reshape(a["key_qvel"], (-1, cm.nv))[key])
        bc = np.ascontiguousarray(np.reshape(a["key_ctrl"], (-1, cm.nu))[key])
    npdt = np.float64 if dtype == "float64" else np.float32
    out = [np.full((B, n), np.nan, dtype=npdt) for n in (cm.nq, cm.nv, max(cm.nu, 1), cm.nv, cm.nv)]
    fn = lib.reset_envs_f64 if dtype == "float64" else lib.reset_envs_f32
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    rc = fn(B, cm.nq, cm.nv, cm.nu, cm.njnt, *[x.ctypes.data for x in ints], bq.ctypes.data, None if bv is None else bv.ctypes.data,
            None if bc is None else bc.ctypes.data, seed, qn, qv, env0, None if m is None else m.ctypes.data, episode.ctypes.data,
            *[o.ctypes.data for o in out])
    assert rc == 0
    return out


def check_close(got, ref, dtype, what):
    if dtype == "float64":
        np.testing.assert_allclose(got, ref, rtol=1e-15, atol=0, err_msg=what)
    else:
        r32 = ref.astype(np.float32)
        ulp = np.spacing(np.abs(r32))
        assert np.all(np.abs(got.astype(np.float64) - r32.astype(np.float64)) <= ulp), what


def quat_addrs(cm):
    return [int(cm.arrays["jnt_qposadr"][j]) + 3 for j in range(cm.njnt) if int(cm.arrays["jnt_type"][j]) == 0]


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "humanoid"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_reset_noise_matches_numpy_reference(harness, compiled, name, dtype):
    from mujoco_template_amd._capi import DeviceModel

    cm = compiled(name)
    dm = DeviceModel(cm)
    B, seed, qn, qv = 8, 1234, 0.3, 0.7
    for key in ([-1, 0] if cm.nkey else [-1]):
        episode = np.array([0, 1, 2, 3, 0, 5, 7, 1], dtype=np.uint32)
        ep0 = episode.copy()
        q, v, c, acc, ws = run(harness, cm, dtype, key, seed, qn, qv, 0, None, episode, B)
        rq, rv, rc = reference(dm, cm, key, seed, qn, qv, np.arange(B), ep0)
        check_close(q, rq, dtype, f"{name} {dtype} key {key}: qpos")
        check_close(v, rv, dtype, f"{name} {dtype} key {key}: qvel")
        if cm.nu:
            check_close(c, rc, dtype, f"{name} {dtype} key {key}: ctrl")
        assert np.all(acc == 0) and np.all(ws == 0)
        assert np.array_equal(episode, ep0 + 1)
        assert not np.array_equal(q, np.tile(q[0], (B, 1))) or cm.nv == 0       # the environments drew different noise
        for qa in quat_addrs(cm):
            n = np.linalg.norm(q[:, qa:qa + 4].astype(np.float64), axis=1)
            assert np.all(np.abs(n - 1) <= (1e-15 if dtype == "float64" else 1e-7)), n


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_reset_without_noise_is_the_base_state(harness, compiled, dtype):
    cm = compiled("humanoid")
    B = 4
    episode = np.zeros(B, dtype=np.uint32)
    q, v, c, acc, ws = run(harness, cm, dtype, -1, 7, 0.0, 0.0, 0, None, episode, B)
    npdt = np.float64 if dtype == "float64" else np.float32
    assert np.array_equal(q, np.tile(np.asarray(cm.arrays["qpos0"]).astype(npdt), (B, 1)))
    assert np.all(v == 0) and np.all(c == 0) and np.all(acc == 0) and np.all(ws == 0)


def test_mask_episode_and_shard_invariance(harness, compiled):
    cm = compiled("humanoid")
    B, k = 6, 4
    # only the masked environments are written; their episode numbers advance, the others' stay
    episode = np.zeros(B, dtype=np.uint32)
    mask = np.array([1, 0, 0, 1, 0, 1], dtype=np.uint8)
    q, *_ = run(harness, cm, "float64", -1, 3, 0.2, 0.2, 0, mask, episode, B)
    assert np.array_equal(episode, mask.astype(np.uint32))
    assert np.all(np.isnan(q[mask == 0])) and np.all(np.isfinite(q[mask == 1]))
    # a second reset of the same environment draws fresh noise (episode 1 instead of 0)
    q2, *_ = run(harness, cm, "float64", -1, 3, 0.2, 0.2, 0, mask, episode, B)
    assert not np.array_equal(q2[0], q[0]) and np.array_equal(episode, 2 * mask.astype(np.uint32))
    # noise is keyed by the GLOBAL environment index: (env0 = k, env 0) == (env0 = 0, env k)
    a, av, *_ = run(harness, cm, "float64", -1, 3, 0.2, 0.2, k, None, np.zeros(1, dtype=np.uint32), 1)
    b, bv, *_ = run(harness, cm, "float64", -1, 3, 0.2, 0.2, 0, None, np.zeros(k + 1, dtype=np.uint32), k + 1)
    assert np.array_equal(a[0], b[k]) and np.array_equal(av[0], bv[k])


class _TorchPolicy:
    device_arrays = True

    def __init__(self, caps=None):
        self.capabilities = caps or ControllerCapabilities()

    def prepare(self, model, data):
        pass

    def __call__(self, model, data, t):
        pass


def test_uses_device_arrays_decision_rule():
    for ctl in (None, ZeroController(), RandomCtrlController(seed=1), LinearFeedbackController(K=np.zeros((1, 2)), ctrl0=np.zeros(1), qpos_goal=np.zeros(1))):
        assert uses_device_arrays(ctl) is False
    assert uses_device_arrays(_TorchPolicy()) is True
    assert device_ctrl_mode_of(_TorchPolicy()) is None
    with pytest.raises(ConfigError):
        uses_device_arrays(_TorchPolicy(ControllerCapabilities(needs_linearization=True)))
    with pytest.raises(ConfigError):
        uses_device_arrays(_TorchPolicy(ControllerCapabilities(needs_jacobians=("site:tip",))))
    truthy = _TorchPolicy()
    truthy.device_arrays = 1                                   # only the explicit True opts in
    assert uses_device_arrays(truthy) is False
