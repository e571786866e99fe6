"""Device-resident control loop on the GPU: per-environment reset / forward (``mjb_reset_envs`` / ``mjb_forward_envs``), torch controllers
on ``DeviceData``, ``reset_done``, stream ordering.  Bitwise comparisons everywhere except the reset noise, which is held to the
float64 numpy reference of tests/test_reset_envs_host.py."""

from __future__ import annotations

import numpy as np
import pytest

from tests.conftest import MODELS
from tests.test_reset_envs_host import check_close, quat_addrs, reference

pytestmark = pytest.mark.gpu

STATE = ("qpos", "qvel", "ctrl", "qacc", "qacc_warmstart", "time")
DERIVED = ("xpos", "xquat", "xipos", "site_xpos", "geom_xpos", "subtree_com", "sensordata")
CASES = [(m, d) for m in ("cartpole", "humanoid") for d in ("float32", "float64")]


def _table(nu, n, seed=0, batch=None):
    rng = np.random.default_rng(seed)
    shape = (n, nu) if batch is None else (n, batch, nu)
    return rng.uniform(-1, 1, shape).astype(np.float32).astype(np.float64)      # fp32-representable


def _snapshot(sim):
    out = {k: sim.get(k) for k in STATE + DERIVED}
    cn = sim.counters()
    out["counters"] = np.stack([cn[k] for k in sorted(cn)], axis=1)
    return out


def _sim(compiled, name, dtype, B):
    from mujoco_template_amd._capi import BatchSim, DeviceModel

    return BatchSim(DeviceModel(compiled(name)), B, dtype=dtype)


def _feed(sim, table, count):
    """ctrl of environment e = table[count[e]] (each environment counts from its own last reset)."""
    sim.set("ctrl", table[count % len(table)])


@pytest.mark.parametrize("name,dtype", CASES)
def test_masked_reset_is_surgical(compiled, name, dtype):
    import torch

    B, T1, T2 = 64, 30, 20
    cm = compiled(name)
    table = _table(cm.nu, T1 + T2)
    a, fresh, never = (_sim(compiled, name, dtype, B) for _ in range(3))       # same creation arguments: the same kernel variants
    for s in (a, fresh, never):
        s.reset(); s.forward()
    count = np.zeros(B, dtype=np.int64)
    for _ in range(T1):
        _feed(a, table, count); a.step(1); count += 1
        _feed(never, table, count - 1); never.step(1)
    before, flags_before = _snapshot(a), a.engine_flags()
    ep_before = a.get("episode")
    mask = torch.zeros(B, dtype=torch.bool, device=f"cuda:{a.device}")
    mask[::3] = True
    m = mask.cpu().numpy()
    a.reset_envs(mask)
    a.forward_envs(mask)
    after, ref = _snapshot(a), _snapshot(fresh)
    for k in after:
        assert np.array_equal(after[k][~m], before[k][~m]), f"{k}: an unmasked environment changed"
        assert np.array_equal(after[k][m], ref[k][m]), f"{k}: a reset environment differs from a freshly reset twin"
    assert a.engine_flags() == flags_before
    ep = a.get("episode")[:, 0]
    assert np.array_equal(ep, ep_before[:, 0] + m)
    count[m] = 0
    for s in range(T2):
        _feed(a, table, count); a.step(1); count += 1
        _feed(never, table, np.full(B, T1 + s)); never.step(1)
        _feed(fresh, table, np.full(B, s)); fresh.step(1)
    got, tn, tf = _snapshot(a), _snapshot(never), _snapshot(fresh)
    for k in STATE + DERIVED:
        assert np.array_equal(got[k][~m], tn[k][~m]), f"{k}: never-reset environments differ from the never-reset twin"
        assert np.array_equal(got[k][m], tf[k][m]), f"{k}: reset environments differ from the freshly reset twin"


@pytest.mark.parametrize("name,dtype", CASES)
def test_reset_noise_matches_reference(compiled, name, dtype):
    from mujoco_template_amd._capi import DeviceModel

    B, seed, qn, qv = 16, 77, 0.2, 0.5
    cm = compiled(name)
    dm = DeviceModel(cm)
    sim = _sim(compiled, name, dtype, B)
    sim.reset_envs(None, seed=seed, qpos_noise=qn, qvel_noise=qv)
    q, v = sim.get("qpos"), sim.get("qvel")
    rq, rv, _ = reference(dm, cm, -1, seed, qn, qv, np.arange(B), np.zeros(B, dtype=np.int64))
    npdt = np.float64 if dtype == "float64" else np.float32
    check_close(q.astype(npdt), rq, dtype, "qpos")
    check_close(v.astype(npdt), rv, dtype, "qvel")
    for qa in quat_addrs(cm):
        n = np.linalg.norm(q[:, qa:qa + 4], axis=1)
        assert np.all(np.abs(n - 1) <= (1e-15 if dtype == "float64" else 1e-7))
    assert np.array_equal(sim.get("episode")[:, 0], np.ones(B))
    sim.reset_envs([0, 5], seed=seed, qpos_noise=qn, qvel_noise=qv)          # a second reset draws fresh noise
    q2 = sim.get("qpos")
    assert np.array_equal(sim.get("episode")[:, 0], np.array([2 if e in (0, 5) else 1 for e in range(B)]))
    assert not np.array_equal(q2[0], q[0]) and np.array_equal(q2[1], q[1])
    rq2, _, _ = reference(dm, cm, -1, seed, qn, qv, np.array([0, 5]), np.array([1, 1]))
    check_close(q2[[0, 5]].astype(npdt), rq2, dtype, "qpos, episode 1")


class TorchTable:
    """ctrl = table[k] on the device, k = control calls since prepare (device_arrays controller)."""

    device_arrays = True

    def __init__(self, table):
        from mujoco_template_amd import ControllerCapabilities

        self.capabilities = ControllerCapabilities()
        self.table, self.k, self._dev = table, 0, None

    def prepare(self, model, data):
        self.k = 0

    def __call__(self, model, data, t):
        import torch

        if self._dev is None:
            self._dev = torch.as_tensor(self.table, device=data.device, dtype=data.ctrl.dtype)
        row = self._dev[self.k % self._dev.shape[0]]
        data.ctrl.copy_(row if row.dim() == 2 else row.expand_as(data.ctrl))
        self.k += 1


class HostTable:
    """The same law as a reference-style host controller (numpy, writes data.ctrl in place)."""

    def __init__(self, table):
        from mujoco_template_amd import ControllerCapabilities

        self.capabilities = ControllerCapabilities()
        self.table, self.k = table, 0

    def prepare(self, model, data):
        self.k = 0

    def __call__(self, model, data, t):
        data.ctrl[...] = self.table[self.k % len(self.table)]
        self.k += 1


@pytest.mark.parametrize("name,dtype", CASES)
@pytest.mark.parametrize("decimation", [1, 2])
def test_torch_controller_equals_host_controller(compiled, name, dtype, decimation):
    import mujoco_template_amd as mt

    B, T = 64, 50
    table = _table(compiled(name).nu, T)
    dev = mt.Env.from_xml_path(MODELS[name], controller=TorchTable(table), batch=B, dtype=dtype, control_decimation=decimation)
    host = mt.Env.from_xml_path(MODELS[name], controller=HostTable(table), batch=B, dtype=dtype, control_decimation=decimation)
    for _ in range(T):
        r = dev.step()
        host.step()
    assert r.done.dtype.is_floating_point is False and tuple(r.done.shape) == (B,)
    assert np.array_equal(np.array(dev.data.qpos), np.array(host.data.qpos))
    assert np.array_equal(np.array(dev.data.qvel), np.array(host.data.qvel))
    assert np.array_equal(np.array(dev.data.time), np.array(host.data.time))


def test_device_loop_makes_no_host_copies(monkeypatch):
    import mujoco_template_amd as mt
    from mujoco_template_amd._capi import BatchSim

    env = mt.Env.from_xml_path(MODELS["humanoid"], controller=TorchTable(_table(21, 8)), batch=256, dtype="float32",
                               reward_fn=lambda m, d, o: -d.qvel.square().sum(1), done_fn=lambda m, d, o: d.qpos[:, 2] < 0.8)

    def boom(*a, **k):
        raise AssertionError("host copy inside the device-resident loop")

    monkeypatch.setattr(BatchSim, "sync_to_host", boom)
    monkeypatch.setattr(BatchSim, "get", boom)
    for _ in range(20):
        r = env.step()
    monkeypatch.undo()
    assert tuple(r.obs.shape) == (256, env.model.nq + env.model.nv) and tuple(r.reward.shape) == (256,) and r.done.dtype.is_floating_point is False


def test_reset_done_restarts_done_environments():
    import torch

    import mujoco_template_amd as mt

    B, T = 64, 200
    table = _table(1, T, seed=3, batch=B) * 3.0
    done_fn = lambda m, d, o: d.qpos[:, 1].abs() > 0.2                         # noqa: E731  pole angle of the cart-pole
    kw = dict(batch=B, dtype="float32", done_fn=done_fn)
    auto = mt.Env.from_xml_path(MODELS["cartpole"], controller=TorchTable(table), reset_done=True, **kw)
    plain = mt.Env.from_xml_path(MODELS["cartpole"], controller=TorchTable(table), **kw)
    fresh = mt.Env.from_xml_path(MODELS["cartpole"], controller=TorchTable(table), **kw)
    first = fresh.observe_device().clone()
    ever = torch.zeros(B, dtype=torch.bool, device=first.device)
    ndone = 0
    for _ in range(T):
        ra, rp = auto.step(), plain.step()
        d = ra.done
        assert torch.equal(ra.info["final_observation"][~ever], rp.obs[~ever])      # pre-reset observation
        assert torch.equal(ra.obs[d], first[d])                                     # first observation of the new episode
        keep = ~ever & ~d
        assert torch.equal(ra.obs[keep], rp.obs[keep])                              # untouched environments: as without reset_done
        ndone += int(d.sum())
        ever |= d
    assert ndone > 0
    assert int(auto.device_data.episode.sum()) == ndone


@pytest.mark.parametrize("name", ["cartpole", "humanoid"])
def test_non_default_stream_gives_the_same_result(compiled, name):
    import torch

    import mujoco_template_amd as mt

    B, T = 128, 20
    table = _table(compiled(name).nu, T, seed=9)
    env0 = mt.Env.from_xml_path(MODELS[name], controller=TorchTable(table), batch=B, dtype="float32")
    env1 = mt.Env.from_xml_path(MODELS[name], controller=TorchTable(table), batch=B, dtype="float32")
    for _ in range(T):
        env0.step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(T):
            env1.step()
        q1 = env1.device_data.qpos.clone()
    torch.cuda.synchronize()
    assert torch.equal(env0.device_data.qpos, q1)
    assert torch.equal(env0.device_data.qvel, env1.device_data.qvel)
