"""Open-loop rollouts from a control tensor (``mjb_rollout_ctrl``, ``BatchSim.rollout_ctrl``, ``Env.rollout(ctrl=)``, ``rollout()``) on
the GPU: bitwise equal to the same controls written before each ``step(1)`` under every launch shape (static map, ticket mode,
two-wave kernel, specialised and generic kernels), ring semantics, broadcasting, parity with the oracle, and the host-side rejections
that keep a bad pointer from ever reaching the device."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mujoco_template_amd import ConfigError, Env, RandomCtrlController, mj, rollout  # noqa: E402
from mujoco_template_amd._capi import CTRL_KEEP, BatchSim, DeviceModel, load_library  # noqa: E402
from mujoco_template_amd import mjcf  # noqa: E402
from oracle import mjo  # noqa: E402
from tests.conftest import MODELS, measured  # noqa: E402

STATE = ("qpos", "qvel", "qacc", "qacc_warmstart", "ctrl", "time", "sensordata")
RING_FLAGS = 1 | 2 | 8 | 16                     # qpos | qvel | sensordata | time
FP32_TRAJ_TOL = {"cartpole": 3.3e-7, "drone2": 1.4e-6}  # fp32 vs float64 oracle, 50 smooth steps: 3x measured (1.1e-7, 4.6e-7)
CTRL_SCALE = {"cartpole": 0.005, "drone2": 1.0, "humanoid": 1.0}   # cart-pole: +-1 of its +-200 range keeps the cart off its joint limits


@pytest.fixture(scope="module")
def world():
    cache = {}

    def get(name):
        if name not in cache:
            cm = mjcf.compile_xml_path(MODELS[name])
            cache[name] = (cm, mjo.OracleModel(cm), DeviceModel(cm))
        return cache[name]

    return get


def _tdt(dtype):
    import torch

    return torch.float32 if dtype == "float32" else torch.float64


def _start(sim, cm, om, seed=0):
    """A distinct, fp32-representable start state per environment (plus a forward pass for the derived arrays)."""
    od = mjo.OracleData(om)
    rng = np.random.default_rng(seed)
    q = np.stack([od.integrate_pos(cm.qpos0, rng.normal(size=cm.nv) * 0.05, 1.0) for _ in range(sim.batch)])
    v = rng.normal(size=(sim.batch, cm.nv)) * 0.2
    sim.set("qpos", q.astype(np.float32).astype(np.float64))
    sim.set("qvel", v.astype(np.float32).astype(np.float64))
    sim.forward()
    sim.sync()


def _table(cm, B, T, dtype, seed=1, scale=1.0):
    """[B, T, nu] controls inside ``scale`` x the ctrl range (about its middle), fp32-representable, on the GPU in the data's dtype."""
    import torch

    lo, hi = np.full(cm.nu, -1.0), np.full(cm.nu, 1.0)
    rg = np.reshape(np.asarray(cm.arrays["actuator_ctrlrange"], dtype=np.float64), (-1, 2))
    lim = np.asarray(cm.arrays["actuator_ctrllimited"]).astype(bool)
    lo[lim], hi[lim] = rg[lim, 0], rg[lim, 1]
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * scale
    lo, hi = mid - half, mid + half
    u = np.random.default_rng(seed).uniform(lo, hi, size=(B, T, cm.nu)).astype(np.float32)
    return torch.from_numpy(u).to(device="cuda", dtype=_tdt(dtype))


def _snapshot(sim):
    cn = sim.counters()
    return [sim.get(k) for k in STATE] + [cn[k] for k in ("ncon", "nefc", "solver_niter")]


def _fused(sim, tab, T):
    import torch

    spec = sim.make_obs_spec(RING_FLAGS)
    ring = torch.full((T, sim.batch, spec.dim), float("nan"), device="cuda", dtype=tab.dtype)
    sim.rollout_ctrl(T, tab, obs_spec=spec, obs_out_ptr=ring.data_ptr(), obs_every=1)
    sim.sync()
    return ring.cpu().numpy(), _snapshot(sim)


def _stepwise(sim, tab, T):
    """T x (write ctrl on the device, step(1)); the state after each step as a ring row (qpos | qvel | sensordata | time)."""
    import torch

    sim.use_torch_stream()
    ctrl, rows = sim.torch_view("ctrl"), []
    for t in range(T):
        ctrl.copy_(tab[:, t])
        sim.step(1)
        rows.append(torch.cat([sim.torch_view("qpos"), sim.torch_view("qvel"), sim.torch_view("sensordata"),
                               sim.torch_view("time").to(tab.dtype)], dim=1).clone())
    sim.sync()
    return torch.stack(rows).cpu().numpy(), _snapshot(sim)


SHAPES = [(n, "float32", s) for n in ("cartpole", "humanoid", "drone2") for s in ("static", "tickets")]
SHAPES += [("humanoid", "float32", "two_wave")]                   # the two-wave kernel takes one-wave-per-environment models only
SHAPES += [(n, "float64", "static") for n in ("cartpole", "humanoid", "drone2")]


@pytest.mark.parametrize("name,dtype,shape", SHAPES)
def test_rollout_ctrl_equals_stepwise(world, name, dtype, shape, monkeypatch):
    """rollout_ctrl(T = 50) == 50 x (write ctrl, step(1)): every state array, the counters and the ring, bit for bit; ring row t is the
    state after step t (sensordata of that step's forward pass); the last row equals the data arrays."""
    cm, om, dm = world(name)
    B, T = 256, 50
    monkeypatch.setenv("MJB_CHUNK_STEPS", "7" if shape == "tickets" else "0")
    monkeypatch.setenv("MJB_TWO_WAVE", "1" if shape == "two_wave" else "0")
    tab = _table(cm, B, T, dtype)
    res = {}
    for how in ("fused", "stepwise"):
        sim = BatchSim(dm, B, dtype=dtype)
        _start(sim, cm, om)
        res[how] = (_fused if how == "fused" else _stepwise)(sim, tab, T)
        if how == "fused":
            info = sim.schedule_info()
            assert info["launch_steps"] == T
            assert info["map"] == ("tickets" if shape == "tickets" else "static")
            assert info["waves_per_env"] == (2 if shape == "two_wave" else 1)
            sim.sync_to_host()
            assert int(sim.host_view("engine_flags")[0]) & 8 == 0
    (ring_f, st_f), (ring_s, st_s) = res["fused"], res["stepwise"]
    assert np.array_equal(ring_f, ring_s), "ring rows differ from the state after each step"
    for k, a, b in zip(STATE + ("ncon", "nefc", "solver_niter"), st_f, st_s):
        assert np.array_equal(a, b), k
    nq, nv, ns = cm.nq, cm.nv, cm.nsensordata
    last = ring_f[-1]
    assert np.array_equal(last[:, :nq], st_f[0]) and np.array_equal(last[:, nq:nq + nv], st_f[1])
    assert np.array_equal(last[:, nq + nv:nq + nv + ns], st_f[6][:, :ns])
    assert np.array_equal(st_f[4], tab[:, -1].double().cpu().numpy())       # data.ctrl holds the last applied control
    assert np.isfinite(ring_f).all()


@pytest.mark.parametrize("name", ["cartpole", "humanoid", "drone2"])
def test_specialised_kernel_equals_generic(world, name):
    cm, om, dm = world(name)
    B, T = 128, 30
    tab = _table(cm, B, T, "float32", seed=4)
    res = {}
    for spec in (True, False):
        sim = BatchSim(dm, B, dtype="float32", specialize=spec)
        assert sim.specialized == spec
        _start(sim, cm, om, seed=2)
        res[spec] = _fused(sim, tab, T)
    assert np.array_equal(res[True][0], res[False][0])
    for a, b in zip(res[True][1], res[False][1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_broadcast_sequences_equal_the_materialised_tensor(world, dtype):
    """[T, nu] (env stride 0) and an expand-ed [B, T, nu] (stride 0, no copy) == the materialised [B, T, nu] tensor, bitwise."""
    cm, om, dm = world("humanoid")
    B, T = 64, 20
    seq = _table(cm, 1, T, dtype, seed=5)[0]                                  # [T, nu]
    res = []
    for tab in (seq, seq.unsqueeze(0).expand(B, T, cm.nu), seq.unsqueeze(0).repeat(B, 1, 1).contiguous()):
        sim = BatchSim(dm, B, dtype=dtype)
        _start(sim, cm, om, seed=3)
        res.append(_fused(sim, tab, T))
    assert res[1][0].shape == res[2][0].shape
    for r in res[:2]:
        assert np.array_equal(r[0], res[2][0])
        for a, b in zip(r[1], res[2][1]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name,T,dtype", [("cartpole", 50, "float64"), ("drone2", 50, "float64"), ("humanoid", 20, "float64"),
                                          ("cartpole", 50, "float32"), ("drone2", 50, "float32")])
def test_trajectory_tracks_the_oracle(world, name, T, dtype):
    """The recorded trajectory against the oracle stepped with the same (fp32-representable) ctrl table: float64 within the suite's
    float64 bounds, fp32 within the free-running bound through measured() - on the smooth models only: contact-rich fp32 trajectories
    are chaotic against the float64 oracle, and the bitwise tests above cover the fp32 humanoid."""
    cm, om, dm = world(name)
    B = 4
    sim = BatchSim(dm, B, dtype=dtype)
    _start(sim, cm, om, seed=6)
    q0, v0 = sim.get("qpos"), sim.get("qvel")
    tab = _table(cm, B, T, dtype, seed=7, scale=CTRL_SCALE[name])
    ring, _ = _fused(sim, tab, T)
    u = tab.double().cpu().numpy()
    nq, nv = cm.nq, cm.nv
    err_q = err_v = 0.0
    for e in range(B):
        od = mjo.OracleData(om)
        od.qpos[:] = q0[e]; od.qvel[:] = v0[e]
        for t in range(T):
            od.ctrl[:] = u[e, t]
            od.step()
            err_q = max(err_q, float(np.abs(ring[t, e, :nq] - od.qpos).max()))
            err_v = max(err_v, float(np.abs(ring[t, e, nq:nq + nv] - od.qvel).max()))
    if dtype == "float64":
        assert err_q <= 1e-9 and err_v <= 1e-7, (err_q, err_v)
    else:
        measured(f"rollout_ctrl/{name}/fp32_qpos_{T}_steps_max", err_q, FP32_TRAJ_TOL[name])


def _hip_runtime():
    """The HIP runtime already in the process (torch's; the library shares it)."""
    with open("/proc/self/maps") as fh:
        paths = {line.split()[-1] for line in fh if "libamdhip64" in line}
    lib = ctypes.CDLL(sorted(paths)[0])
    lib.hipMemGetAddressRange.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    lib.hipMemGetAddressRange.restype = ctypes.c_int
    return lib


def test_rejections_leave_state_and_flags_untouched(world):
    import torch

    cm, om, dm = world("cartpole")
    B, T, nu = 16, 10, cm.nu
    sim = BatchSim(dm, B, dtype="float32")
    _start(sim, cm, om)
    L = load_library()
    before = _snapshot(sim)
    sim.sync_to_host()
    flags0 = float(sim.host_view("engine_flags")[0])
    tab = _table(cm, B, T, "float32")

    def raw(ptr, nstep=T, ss=nu, es=T * nu):
        return L.mjb_rollout_ctrl(sim.ptr, nstep, ctypes.c_void_p(ptr), ss, es, None, None, 0)

    host = np.zeros((B, T, nu), dtype=np.float32)                             # pageable host memory
    assert raw(host.ctypes.data) == -1
    with pytest.raises(ConfigError):
        sim.rollout_ctrl(T, host)
    assert raw(tab.data_ptr(), ss=-1) == -1 and raw(tab.data_ptr(), es=-nu) == -1
    assert raw(0) == -1                                                       # NULL with nu > 0
    with pytest.raises(ConfigError):
        sim.rollout_ctrl(T + 1, tab)                                          # fewer steps than nstep: the front checks the shape
    with pytest.raises(ConfigError):
        sim.rollout_ctrl(T, tab.double())                                     # wrong dtype
    with pytest.raises(ConfigError):
        sim.rollout_ctrl(T, tab.cpu())                                        # wrong device
    with pytest.raises(ConfigError):
        sim.rollout(T, 4)                                                     # the sequence mode is not reachable through mjb_rollout
    assert L.mjb_rollout(sim.ptr, T, 4, 0, 0, 1.0, None, None, 0) == -1
    # the C bound: an extent one element past the end of the allocation hipMemGetAddressRange reports is refused, the last element is not
    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    assert _hip_runtime().hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(tab.data_ptr())) == 0
    n_ok = (base.value + size.value - tab.data_ptr()) // 4                     # float32 elements from the table to the end of its block
    assert n_ok >= T * B * nu
    assert raw(tab.data_ptr(), nstep=2, ss=n_ok - nu + 1, es=0) == -1
    assert raw(tab.data_ptr(), nstep=1, ss=0, es=(n_ok - nu) // (B - 1) + 1) == -1
    after = _snapshot(sim)
    sim.sync_to_host()
    assert float(sim.host_view("engine_flags")[0]) == flags0
    for k, a, b in zip(STATE, before, after):
        assert np.array_equal(a, b), k
    assert raw(tab.data_ptr(), nstep=2, ss=n_ok - nu, es=0) == 0              # the highest element is the block's last one: accepted
    sim.sync()
    torch.cuda.synchronize()


def test_env_rollout_with_ctrl_is_open_loop(world):
    """Env.rollout(ctrl=) ignores the environment's controller and returns the obs ring as the controller path does."""
    cm, om, dm = world("cartpole")
    B, T = 32, 25
    tab = _table(cm, B, T, "float32", seed=8)
    env = Env.from_xml_path(MODELS["cartpole"], controller=RandomCtrlController(seed=1), batch=B, dtype="float32")
    start = {k: env.data.sim.get(k) for k in STATE[:-1]}
    obs = env.rollout(T, ctrl=tab, obs_every=5)
    assert tuple(obs.shape[:2]) == (T // 5, B)
    sim = BatchSim(dm, B, dtype="float32")
    for k, v in start.items():
        sim.set(k, v)
    sim.rollout_ctrl(T, tab)
    sim.sync()
    assert np.array_equal(np.array(env.data.qpos), sim.get("qpos"))
    assert np.array_equal(np.array(env.data.ctrl), tab[:, -1].cpu().numpy())
    with pytest.raises(ConfigError):
        env.rollout(T, ctrl=tab[:, :T - 1])


def _mj(name, B, dtype):
    model = mj.MjModel.from_xml_path(MODELS[name])
    return model, mj.MjData(model, batch=B, dtype=dtype)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_rollout_function_shapes_rows_and_initial_state(world, dtype):
    import torch

    cm, om, dm = world("drone2")
    B, T = 8, 30
    nq, nv, nx, ns = cm.nq, cm.nv, 1 + cm.nq + cm.nv, cm.nsensordata
    model, data = _mj("drone2", B, dtype)
    rng = np.random.default_rng(9)
    od = mjo.OracleData(om)
    x0 = np.stack([np.concatenate([[0.25], od.integrate_pos(cm.qpos0, rng.normal(size=nv) * 0.1, 1.0), rng.normal(size=nv) * 0.3])
                   for _ in range(B)]).astype(np.float32).astype(np.float64)
    x0[:, 3] += 1.0                                                              # in the air
    tab = _table(cm, B, T, dtype, seed=10)
    state, sens = rollout(model, data, tab, initial_state=x0)
    assert tuple(state.shape) == (B, T, nx) and tuple(sens.shape) == (B, T, ns)
    assert state.dtype == _tdt(dtype) and state.device.type == "cuda"
    # row t = the state after step t: the same controls through BatchSim step by step from the same start
    sim = BatchSim(dm, B, dtype=dtype)
    sim.set("qpos", x0[:, 1:1 + nq]); sim.set("qvel", x0[:, 1 + nq:]); sim.set("time", x0[:, :1]); sim.set("qacc_warmstart", np.zeros((B, nv)))
    ring, st = _stepwise(sim, tab, T)
    s, d = state.cpu().numpy(), sens.cpu().numpy()
    assert np.array_equal(s[..., 1:1 + nq], ring[..., :nq].transpose(1, 0, 2))
    assert np.array_equal(s[..., 1 + nq:], ring[..., nq:nq + nv].transpose(1, 0, 2))
    assert np.array_equal(d, ring[..., nq + nv:nq + nv + ns].transpose(1, 0, 2))
    assert np.array_equal(s[..., 0], ring[..., -1].T)                          # time rounded to the data dtype
    assert np.allclose(s[:, -1, 0], 0.25 + T * model.opt.timestep, rtol=1e-6)
    # data ends in the final state, time in float64
    assert np.array_equal(np.asarray(data.qpos), st[0]) and np.array_equal(np.asarray(data.time), st[5][:, 0])
    # broadcast initial state == the same state tiled per environment
    s1, _ = rollout(model, data, tab, initial_state=torch.from_numpy(x0[0]))
    s2, _ = rollout(model, data, tab, initial_state=np.tile(x0[0], (B, 1)))
    assert torch.equal(s1, s2)


def test_rollout_function_warmstart_and_control_none(world):
    import torch

    cm, om, dm = world("humanoid")
    B, T, nv = 16, 12, cm.nv
    model, data = _mj("humanoid", B, "float32")
    mj.mj_forward(model, data)
    x0 = np.concatenate([np.zeros((B, 1)), np.asarray(data.qpos), np.asarray(data.qvel)], axis=1)
    tab = _table(cm, B, T, "float32", seed=12)
    # zeroed warm start by default: a rollout does not depend on what qacc_warmstart held before
    a, _ = rollout(model, data, tab, initial_state=x0)
    data.sim.torch_view("qacc_warmstart").fill_(3.0)
    b, _ = rollout(model, data, tab, initial_state=x0)
    assert torch.equal(a, b)
    # initial_warmstart given == that warm start set by hand before the same rollout_ctrl
    w = torch.randn(B, nv, device="cuda") * 0.1
    c, _ = rollout(model, data, tab, initial_state=x0, initial_warmstart=w)
    sim = BatchSim(dm, B, dtype="float32")
    sim.set("qpos", x0[:, 1:1 + cm.nq]); sim.set("qvel", x0[:, 1 + cm.nq:]); sim.set("qacc_warmstart", w.double().cpu().numpy())
    sim.rollout_ctrl(T, tab)
    sim.sync()
    assert np.array_equal(c[:, -1, 1:1 + cm.nq].cpu().numpy(), sim.get("qpos"))
    # control=None: nstep steps on data.ctrl == mjb_rollout(KEEP) with the same ring
    data.ctrl[:] = 0.1
    s, _ = rollout(model, data, None, initial_state=x0, nstep=T)
    sim2 = BatchSim(dm, B, dtype="float32")
    sim2.set("qpos", x0[:, 1:1 + cm.nq]); sim2.set("qvel", x0[:, 1 + cm.nq:]); sim2.set("ctrl", np.full((B, cm.nu), 0.1))
    spec = sim2.make_obs_spec(RING_FLAGS)
    ring = torch.empty((T, B, spec.dim), device="cuda")
    sim2.rollout(T, CTRL_KEEP, obs_spec=spec, obs_out_ptr=ring.data_ptr(), obs_every=1)
    sim2.sync()
    assert torch.equal(s[..., 1:], ring[..., :cm.nq + nv].permute(1, 0, 2))
    with pytest.raises(ConfigError):
        rollout(model, data, None)
    with pytest.raises(ConfigError):
        rollout(model, data, tab, initial_state=np.zeros(3))
