"""Per-environment model parameters (``BatchSim.set_env_params``, ``Env.set_model_params``) on the GPU: batching a field with the
model's own values changes nothing, every environment matches the float64 oracle run on a copy of the model carrying that
environment's values (tests/model_params_oracle.py), through every kernel and work map, and the parameters' life cycle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mujoco_template_amd import mjcf  # noqa: E402
from mujoco_template_amd._capi import CTRL_RANDOM, ENV_PARAM_FIELDS, BatchSim, DeviceModel  # noqa: E402
from oracle import mjo  # noqa: E402
from tests.conftest import MODELS, measured  # noqa: E402
from tests.model_params_oracle import env_oracle, row  # noqa: E402

STATE = ("qpos", "qvel", "qacc", "qacc_warmstart", "ctrl", "time", "sensordata", "xpos", "subtree_com")
# fp32, one teacher-forced humanoid step vs the oracle (relative to max(1, |qvel|)), over the environments with the oracle's contact and
# row counts; measured 1.15e-5 (B = 64, one wave) and 2.89e-5 (B = 512, two waves).  A contact at its activation threshold can flip
# under the fp32 rounding of the state (B = 512: one environment of 512, 2 contacts against the oracle's 3, while float64 data match
# all 512 to 7e-13): such environments are counted, and must stay rare.
TEACHER_TOL32 = {"step": 2e-5, "two_wave": 5e-5}
MAX_FLIPS = 0.02
FD_TOL = {"float64": 2.5e-10, "float32": 2.5e-10}    # cart-pole FD vs the oracle's FD (tests/test_gpu_parity.py FD_TOL["cartpole"])


@pytest.fixture(scope="module")
def world():
    cache = {}

    def get(name):
        if name not in cache:
            cm = mjcf.compile_xml_path(MODELS[name])
            cache[name] = (cm, mjo.OracleModel(cm), DeviceModel(cm))
        return cache[name]

    return get


def own_values(cm) -> dict:
    return {k: (np.array(cm.gravity, dtype=np.float64) if k == "gravity" else np.array(cm.arrays[k], dtype=np.float64)) for k in ENV_PARAM_FIELDS}


def random_params(cm, B, seed, fields=ENV_PARAM_FIELDS, fp32=False) -> dict:
    """The issue's ranges: mass / inertia / armature / gear / gains / bias +-20 %, damping x[0.5, 2], sliding friction in [0.5, 1.5],
    gravity z in [-11, -8.5]."""
    rng = np.random.default_rng(seed)
    own = own_values(cm)
    out = {}
    for k in fields:
        v = np.broadcast_to(own[k], (B, *own[k].shape)).copy()
        if k == "dof_damping":
            v = v * rng.uniform(0.5, 2.0, v.shape) if np.any(v > 0) else rng.uniform(0.05, 0.5, v.shape)
        elif k == "geom_friction":
            v[..., 0] = rng.uniform(0.5, 1.5, v.shape[:-1])
        elif k == "gravity":
            v[:, 2] = rng.uniform(-11.0, -8.5, B)
        else:
            v = v * rng.uniform(0.8, 1.2, v.shape)
        out[k] = v.astype(np.float32).astype(np.float64) if fp32 else v
    return out


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _snapshot(sim):
    out = {k: sim.get(k) for k in STATE}
    cn = sim.counters()
    out["counters"] = np.stack([cn[k] for k in ("ncon", "nefc", "solver_niter")], axis=1)
    return out


def _standing(sim, cm):
    key = cm.name2id(mjcf.OBJ_KEY, "stand_on_left_leg")
    sim.reset(key)
    sim.forward()
    return key


# ---- 1. identity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_identity_generic_kernel_is_bitwise(world, dtype):
    """Every field batched with the model's own values: the generic kernel's results are bitwise those of the unbatched data, through
    a random-ctrl rollout and through step()."""
    cm, om, dm = world("humanoid")
    B = 64
    sims = [BatchSim(dm, B, dtype=dtype, specialize=False) for _ in range(2)]
    sims[1].set_env_params(**own_values(cm))
    assert sims[1].env_param_fields() == ENV_PARAM_FIELDS
    for s in sims:
        _standing(s, cm)
        s.rollout(20, CTRL_RANDOM, seed=11, ctrl_scale=0.5)
        s.step(5)
    a, b = (_snapshot(s) for s in sims)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_identity_specialised_kernel(world):
    """The same through the fp32 specialised kernel (built for all nine fields vs none): bitwise as well (measured: the rows hold the
    values the baked tables hold, and the arithmetic is the same)."""
    cm, om, dm = world("humanoid")
    B = 2048
    sims = [BatchSim(dm, B, dtype="float32", specialize=True) for _ in range(2)]
    sims[1].set_env_params(**own_values(cm))
    assert sims[0].specialized and sims[1].specialized
    assert "#define MJB_SPEC_PARAMS 511" in sims[1].spec_source()
    for s in sims:
        _standing(s, cm)
        s.rollout(5, CTRL_RANDOM, seed=11, ctrl_scale=0.5)
    a, b = (_snapshot(s) for s in sims)
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, _rel(b[k], a[k]))


# ---- 2. parity with the oracle ------------------------------------------------------------------------------------------------------
def test_parity_humanoid_float64_free_running(world):
    """B = 64 standing humanoids, every field randomised per environment, 30 free-running random-ctrl steps: each environment
    matches its own oracle to 1e-9 relative with the same contact and row counts."""
    cm, om, dm = world("humanoid")
    B, T, seed = 64, 30, 5
    prm = random_params(cm, B, 21)
    sim = BatchSim(dm, B, dtype="float64")
    sim.set_env_params(**prm)
    key = _standing(sim, cm)
    sim.rollout(T, CTRL_RANDOM, seed=seed, ctrl_scale=0.5)
    q, v, cn = sim.get("qpos"), sim.get("qvel"), sim.counters()
    worst, ncon = 0.0, []
    for e in range(B):
        od = mjo.OracleData(env_oracle(cm, **row(prm, e)))
        od.reset_keyframe(key)
        od.rollout_random(T, seed=seed, env=e, scale=0.5)
        worst = max(worst, _rel(q[e], od.qpos), _rel(v[e], od.qvel))
        oc = od.counters()
        assert (int(cn["ncon"][e]), int(cn["nefc"][e])) == (oc["ncon"], oc["nefc"]), e
        ncon.append(oc["ncon"])
    assert max(ncon) > 0, "contacts must be live"
    assert worst <= 1e-9, worst


def test_parameters_change_the_trajectory(world):
    """Two environments in the same state with the same (zero) controls but different parameters end in different states."""
    cm, om, dm = world("humanoid")
    sim = BatchSim(dm, 2, dtype="float64")
    prm = random_params(cm, 2, 3)
    sim.set_env_params(**prm)
    _standing(sim, cm)
    sim.set("ctrl", np.zeros((2, cm.nu)))
    sim.step(10)
    q = sim.get("qpos")
    assert not np.array_equal(q[0], q[1])


def _teacher_forced(sim, cm, prm, B):
    """One step from the same fp32-representable state on both sides; returns the worst relative qvel error over the environments
    with the oracle's contact / row counts, and the number of the others."""
    key = cm.name2id(mjcf.OBJ_KEY, "stand_on_left_leg")
    rng = np.random.default_rng(8)
    ods = []
    for e in range(B):
        od = mjo.OracleData(env_oracle(cm, **row(prm, e)))
        od.reset_keyframe(key)
        od.rollout_random(3 + e % 5, seed=2, env=e, scale=0.3)
        od.ctrl[:] = rng.uniform(-0.5, 0.5, cm.nu)
        ods.append(od)
    state = {k: np.stack([getattr(od, k) for od in ods]).astype(np.float32).astype(np.float64) for k in ("qpos", "qvel", "ctrl", "qacc_warmstart")}
    for k, val in state.items():
        sim.set(k, val)
    sim.step(1)
    v, cn = sim.get("qvel"), sim.counters()
    worst, flips = 0.0, 0
    for e, od in enumerate(ods):
        for k, val in state.items():
            getattr(od, k)[:] = val[e]
        od.step()
        oc = od.counters()
        if (int(cn["ncon"][e]), int(cn["nefc"][e])) != (oc["ncon"], oc["nefc"]):
            flips += 1
            continue
        worst = max(worst, _rel(v[e], od.qvel))
    assert flips <= MAX_FLIPS * B, flips
    return worst, flips


def test_parity_humanoid_float32_teacher_forced(world, monkeypatch):
    """fp32, one step of the (specialised, all fields) one-wave step kernel from the oracle's state."""
    cm, om, dm = world("humanoid")
    B = 64
    monkeypatch.setenv("MJB_TWO_WAVE", "0")
    prm = random_params(cm, B, 22, fp32=True)
    sim = BatchSim(dm, B, dtype="float32")
    sim.set_env_params(**prm)
    assert sim.specialized
    worst, flips = _teacher_forced(sim, cm, prm, B)
    assert sim.schedule_info()["waves_per_env"] == 1
    measured("model_params/teacher_forced_fp32", worst, TEACHER_TOL32["step"], f"(relative qvel after one step; {flips} contact flips)")


# ---- 3. work maps -------------------------------------------------------------------------------------------------------------------
def test_ticket_map_equals_static_map(world, monkeypatch):
    cm, om, dm = world("humanoid")
    B, T = 4096, 40
    prm = random_params(cm, B, 23, fp32=True)
    out, maps = [], []
    for chunk in ("0", "7"):
        monkeypatch.setenv("MJB_CHUNK_STEPS", chunk)
        sim = BatchSim(dm, B, dtype="float32")
        sim.set_env_params(**prm)
        _standing(sim, cm)
        sim.rollout(T, CTRL_RANDOM, seed=4, ctrl_scale=0.5)
        maps.append(sim.schedule_info()["map"])
        out.append(_snapshot(sim))
    assert maps == ["static", "tickets"]
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


def test_two_wave_kernel_matches_oracle(world, monkeypatch):
    cm, om, dm = world("humanoid")
    B = 512
    monkeypatch.setenv("MJB_TWO_WAVE", "1")
    prm = random_params(cm, B, 24, fp32=True)
    sim = BatchSim(dm, B, dtype="float32")
    sim.set_env_params(**prm)
    worst, flips = _teacher_forced(sim, cm, prm, B)
    assert sim.schedule_info()["waves_per_env"] == 2
    measured("model_params/teacher_forced_fp32_two_wave", worst, TEACHER_TOL32["two_wave"], f"(relative qvel after one step; {flips} contact flips)")


# ---- 4. finite differences ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_transition_fd_matches_oracle(world, dtype):
    """Per-environment mass, damping and gain (the other fields batched with the model's values): float64 data through the
    specialised FD kernel, float32 data through the generic one (which reads the float64 masters)."""
    cm, om, dm = world("cartpole")
    B = 32
    prm = own_values(cm)
    prm = {k: np.broadcast_to(v, (B, *v.shape)).copy() for k, v in prm.items()}
    prm.update(random_params(cm, B, 25, fields=("body_mass", "dof_damping", "actuator_gainprm"), fp32=dtype == "float32"))
    od0 = mjo.OracleData(om)
    rng = np.random.default_rng(7)
    q = np.stack([od0.integrate_pos(cm.qpos0, rng.normal(size=cm.nv) * 0.02, 1.0) for _ in range(B)])
    v, u = rng.normal(size=(B, cm.nv)) * 0.1, rng.uniform(-0.5, 0.5, (B, cm.nu))
    sim = BatchSim(dm, B, dtype=dtype, specialize=None if dtype == "float64" else False)
    sim.set_env_params(**prm)
    sim.set("qpos", q); sim.set("qvel", v); sim.set("ctrl", u)
    A, Bm = sim.transition_fd(1e-6, True)
    assert sim.fd_specialized == (dtype == "float64")
    qd, vd, ud = sim.get("qpos"), sim.get("qvel"), sim.get("ctrl")
    worst = 0.0
    for e in range(B):
        od = mjo.OracleData(env_oracle(cm, **row(prm, e)))
        od.qpos[:] = qd[e]; od.qvel[:] = vd[e]; od.ctrl[:] = ud[e]
        Ao, Bo = od.transition_fd(1e-6, True)
        worst = max(worst, np.abs(A[e] - Ao).max() / max(1.0, np.abs(Ao).max()), np.abs(Bm[e] - Bo).max() / max(1.0, np.abs(Bo).max()))
    measured(f"model_params/transition_fd/cartpole/{dtype}", worst, FD_TOL[dtype], "(relative to the largest entry of A / B)")
    assert not np.allclose(A[0], A[1])                        # the parameters reach the linearisation


# ---- 5. inverse dynamics ------------------------------------------------------------------------------------------------------------
def test_inverse_matches_oracle(world):
    cm, om, dm = world("humanoid")
    B = 16
    prm = random_params(cm, B, 26)
    od0 = mjo.OracleData(om)
    rng = np.random.default_rng(9)
    q = np.stack([od0.integrate_pos(cm.qpos0, rng.normal(size=cm.nv) * 0.1, 1.0) for _ in range(B)])
    v, a = rng.normal(size=(B, cm.nv)) * 0.3, rng.normal(size=(B, cm.nv))
    sim = BatchSim(dm, B, dtype="float64")
    sim.set_env_params(**prm)
    sim.set("qpos", q); sim.set("qvel", v); sim.set("qacc", a)
    sim.inverse()
    f, mom = sim.get("qfrc_inverse"), sim.get("actuator_moment")
    for e in range(B):
        od = mjo.OracleData(env_oracle(cm, **row(prm, e)))
        od.qpos[:] = q[e]; od.qvel[:] = v[e]; od.qacc[:] = a[e]
        od.inverse()
        assert _rel(f[e], od.qfrc_inverse) <= 1e-9, e
        assert _rel(mom[e], od.actuator_moment.reshape(-1)) <= 1e-9, e


# ---- 6. damping on a model without damping ------------------------------------------------------------------------------------------
DAMPLESS_XML = """<mujoco><option timestep="0.005"/><worldbody><geom type="plane" size="5 5 .1"/>
  <body pos="0 0 1"><joint name="a" type="hinge" axis="0 1 0"/><geom type="capsule" fromto="0 0 0 .4 0 0" size=".04"/>
    <body pos=".4 0 0"><joint name="b" type="hinge" axis="0 1 0"/><geom type="capsule" fromto="0 0 0 .4 0 0" size=".04"/></body></body>
  </worldbody><actuator><motor joint="a" gear="3"/></actuator></mujoco>"""


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_damping_on_a_model_without_damping(dtype):
    cm = mjcf.compile_xml_string(DAMPLESS_XML)
    assert not np.any(np.asarray(cm.arrays["dof_damping"]) > 0)
    dm = DeviceModel(cm)
    B, T = 8, 40
    prm = {"dof_damping": np.random.default_rng(4).uniform(0.5, 3.0, (B, cm.nv)).astype(np.float32).astype(np.float64)}
    sim = BatchSim(dm, B, dtype=dtype, specialize=False)
    plain = BatchSim(dm, B, dtype=dtype, specialize=False)
    sim.set_env_params(**prm)
    for s in (sim, plain):
        s.set("qvel", np.full((B, cm.nv), 2.0))
        s.rollout(T, CTRL_RANDOM, seed=1)
    q = sim.get("qpos")
    assert not np.allclose(q, plain.get("qpos"))
    for e in range(B):
        od = mjo.OracleData(env_oracle(cm, **row(prm, e)))
        od.qvel[:] = 2.0
        od.rollout_random(T, seed=1, env=e)
        assert _rel(q[e], od.qpos) <= (1e-9 if dtype == "float64" else 1e-4), e


# ---- 7. life cycle ------------------------------------------------------------------------------------------------------------------
def test_masked_set_reset_and_clear(world):
    import torch

    cm, om, dm = world("cartpole")
    B = 16
    sim = BatchSim(dm, B, dtype="float32", specialize=False)
    never = BatchSim(dm, B, dtype="float32", specialize=False)
    own = own_values(cm)
    full = random_params(cm, B, 30, fp32=True)
    mask = torch.zeros(B, dtype=torch.bool, device=f"cuda:{sim.device}")
    mask[::3] = True
    sim.use_torch_stream()
    sim.set_env_params(envs=mask, body_mass=torch.as_tensor(full["body_mass"], device=mask.device))
    got = sim.env_params("body_mass")
    m = mask.cpu().numpy()
    assert np.array_equal(got[m], full["body_mass"][m])
    assert np.array_equal(got[~m], np.broadcast_to(own["body_mass"], got[~m].shape))
    sim.set_env_params(envs=[1], gravity=np.array([0.0, 0.0, -3.0]))
    g = sim.env_params("gravity")
    assert np.array_equal(g[1], [0, 0, -3.0]) and np.array_equal(np.delete(g, 1, axis=0), np.broadcast_to(own["gravity"], (B - 1, 3)))
    assert np.array_equal(never.env_params("gravity"), np.broadcast_to(own["gravity"], (B, 3)))
    sim.reset_envs(mask)
    sim.reset()
    assert np.array_equal(sim.env_params("body_mass"), got)
    assert np.array_equal(sim.env_params("gravity"), g)
    sim.clear_env_params()
    assert sim.env_param_mask() == 0
    for s in (sim, never):
        s.reset()
        s.rollout(30, CTRL_RANDOM, seed=2)
    a, b = _snapshot(sim), _snapshot(never)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_rejections(world):
    import torch

    from mujoco_template_amd import ConfigError

    cm, om, dm = world("cartpole")
    sim = BatchSim(dm, 4, dtype="float32", specialize=False)
    with pytest.raises(ConfigError):
        sim.set_env_params(geom_size=np.zeros(3))
    with pytest.raises(ConfigError):
        sim.set_env_params(gravity=np.array([0.0, np.nan, -9.81]))
    with pytest.raises(ConfigError):
        sim.set_env_params(body_mass=np.ones((3, cm.nbody)))
    bad = torch.ones((4, cm.nbody), device="cpu")
    with pytest.raises(ConfigError):
        sim.set_env_params(body_mass=bad)
    assert sim.env_param_mask() == 0
    import ctypes

    from mujoco_template_amd._capi import _check, load_library

    src = np.ones((4, cm.nbody))
    host_mask = np.ones(4, dtype=np.uint8)
    with pytest.raises(ConfigError):            # env_mask in pageable host memory
        _check(load_library().mjb_set_env_param(sim.ptr, b"body_mass", src.ctypes.data, 1, 0, host_mask.ctypes.data))
    with pytest.raises(ConfigError):            # a host block passed as device memory
        _check(load_library().mjb_set_env_param(sim.ptr, b"body_mass", src.ctypes.data, 1, 1, None))
    assert sim.env_param_mask() == 0


def test_reset_done_loop_resamples_parameters():
    """A reset_done loop that re-samples body_mass and gravity of the environments reset by each step (mask taken on the device):
    200 steps; the environments never reset keep their first parameters."""
    import torch

    import mujoco_template_amd as mt
    from tests.test_gpu_device_loop import TorchTable

    B, T = 64, 200
    table = np.random.default_rng(3).uniform(-1, 1, (T, B, 1)) * 3.0
    table[:, B // 2:] = 0.0                                    # the upper half holds the pole at rest upright: never done
    env = mt.Env.from_xml_path(MODELS["cartpole"], controller=TorchTable(table), reset_done=True, batch=B, dtype="float32",
                               done_fn=lambda m, d, o: d.qpos[:, 1].abs() > 0.2, specialize=False)
    dev = torch.device("cuda:0")
    cm = mjcf.compile_xml_path(MODELS["cartpole"])
    base_mass = torch.as_tensor(np.asarray(cm.arrays["body_mass"]), device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    env.set_model_params(body_mass=base_mass * (0.8 + 0.4 * torch.rand((B, cm.nbody), generator=gen, device=dev, dtype=torch.float64)))
    first = env.model_params("body_mass")
    ever = torch.zeros(B, dtype=torch.bool, device=dev)
    for _ in range(T):
        r = env.step()
        mass = base_mass * (0.8 + 0.4 * torch.rand((B, cm.nbody), generator=gen, device=dev, dtype=torch.float64))
        grav = torch.tensor([0.0, 0.0, -9.81], device=dev, dtype=torch.float64).repeat(B, 1)
        grav[:, 2] -= torch.rand(B, generator=gen, device=dev, dtype=torch.float64)
        env.set_model_params(envs=r.done, body_mass=mass, gravity=grav)
        ever |= r.done
    assert 0 < int(ever.sum()) <= B // 2
    after = env.model_params("body_mass")
    keep = ~ever.cpu().numpy()
    assert np.array_equal(after[keep], first[keep])
    assert not np.array_equal(after[~keep], first[~keep])
    g = env.model_params("gravity")
    assert np.array_equal(g[keep], np.broadcast_to(cm.gravity, g[keep].shape))
    assert np.isfinite(np.array(env.data.qpos)).all()
