"""The sensor half of ``mjd_transitionFD`` on the GPU: ``C = d sensordata / d[dq; dv]`` and ``D = d sensordata / d ctrl`` from the
per-column sensor vectors of the finite-difference kernel (``mjb_transition_fd_sensors`` / ``mjb_transition_fd_points_sensors``,
``BatchSim.transition_fd(sensors=True)``, ``transition_fd_points(sensors=True)``, ``linearize_rollout(sensor_derivatives=True)``,
``mj.mjd_transitionFD(..., C, D)``).

The expected values are a numpy loop over the float64 oracle's ``step`` (tests/fd_sensors_common.py); the anchors need no oracle;
``A`` and ``B`` of a sensor call are bitwise those of the plain call.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mujoco_template_amd import linearize_rollout, mj, mjcf  # noqa: E402
from mujoco_template_amd._capi import load_library  # noqa: E402
from oracle import mjo  # noqa: E402
from tests.conftest import MODELS, measured  # noqa: E402
from tests.fd_sensors_common import RK4_HINGE, cartpole_sensors_xml, oracle_sensor_fd  # noqa: E402
from tests.feature_models import RK4_CONTACT, SITE_WRENCH  # noqa: E402

EPS = 1e-6
DTYPES = ("float64", "float32")
NAMES = ("site_wrench", "knee", "drone2", "cartpole_sensors", "rk4_hinge")
FIELDS = ("qpos", "qvel", "ctrl", "qacc_warmstart")

# Device C, D against the oracle loop, relative to max(1, max|C|) and max(1, max|D|), worst over the environments and over the centred
# and the forward difference; each bound <= 3x the value measured on an MI355X (measured values in the comments; float64 and float32 data
# gave the same figures).  The errors are single roundings of a sensor value divided by the difference step, not accuracy lost:
#  * drone2, site_wrench (max|C| = 1 apart from the resting puck, so the figure is absolute): 1.776e-9 = 2^-49 / 1e-6 - ONE ulp of an
#    accelerometer reading of magnitude 8 .. 16 (drone2: |g| = 9.81) by which the two implementations of a step disagree,
#    over the forward difference's eps; the centred difference shows the same ulp over 2 eps, 8.88e-10.  That is 18x FD_TOL (1e-10,
#    tests/test_gpu_parity.py), whose state entries are of magnitude <= 2 and always centred: the quantum is 8x larger and the step half.
#    The resting puck (env 1, max|C| = 2.1e3 in the accelerometer rows over the contact) measures 1.2e-11 relative in C and 1.8e-9 in D,
#    below FD_CONTACT_TOL (3e-9): its contact solve is not what sets the bound.
#  * rk4_hinge: 4.4e-10 = 2^-51 / 1e-6, roundings of readings of magnitude about 1; knee: 2.8e-11 = 2^-55 / 1e-6, of an angle of magnitude 0.1.
#  * cartpole_sensors: 0.  Euler: jointpos of the perturbed point is q +- eps itself, and both sides do the same two IEEE operations.
FD_SENS_TOL = {
    ("site_wrench", "float64"): 5.2e-9, ("site_wrench", "float32"): 5.3e-9,            # measured 1.72e-9 / 1.78e-9
    ("knee", "float64"): 8.3e-11, ("knee", "float32"): 8.3e-11,                        # measured 2.8e-11 / 2.8e-11
    ("drone2", "float64"): 5.3e-9, ("drone2", "float32"): 5.3e-9,                      # measured 1.78e-9 / 1.78e-9
    ("cartpole_sensors", "float64"): 0.0, ("cartpole_sensors", "float32"): 0.0,        # measured 0 / 0 (bit for bit)
    ("rk4_hinge", "float64"): 1.3e-9, ("rk4_hinge", "float32"): 1.3e-9,                # measured 4.4e-10 / 4.4e-10
}


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _xml(name):
    return {"site_wrench": SITE_WRENCH, "knee": RK4_CONTACT, "cartpole_sensors": cartpole_sensors_xml(), "rk4_hinge": RK4_HINGE}.get(name)


@pytest.fixture(scope="module")
def world():
    cache = {}

    def get(name):
        if name not in cache:
            xml = _xml(name)
            cm = mjcf.compile_xml_path(MODELS[name]) if xml is None else mjcf.compile_xml_string(xml)
            mm = mj.MjModel.from_xml_path(MODELS[name]) if xml is None else mj.MjModel.from_xml_string(xml)
            cache[name] = (cm, mjo.OracleModel(cm), mm)
        return cache[name]

    return get


def _prepare(name, cm, mm, dtype):
    """A data object of the issue's shape for this model, left at the states the Jacobians are taken at (fp32-representable)."""
    rng = np.random.default_rng(11)
    if name == "site_wrench":
        # B = 3: [0] airborne, [1] resting on the floor with its rolled-out warm start, [2] airborne with ctrl[1] at its lower bound 0
        data = mj.MjData(mm, batch=3, dtype=dtype)
        sim = data.sim
        sim.set("ctrl", np.array([[0.3, 0.4], [0.2, 0.5], [-0.5, 0.0]]))
        sim.step(150)
        sim.sync()
        q, v = sim.get("qpos"), sim.get("qvel")
        for e, (z, ang) in ((0, (0.5, 0.3)), (2, (0.7, -0.2))):
            q[e] = _f32([0.1 * e, -0.05, z, np.cos(ang / 2), 0.0, np.sin(ang / 2) * 0.6, np.sin(ang / 2) * 0.8])
            v[e] = _f32(rng.normal(size=6) * 0.3)
        sim.set("qpos", q); sim.set("qvel", v)
    elif name == "knee":
        # joint limits active: the knee beyond its upper (25 deg) and lower (-5 deg) limit, the slide beyond its upper limit (0.05)
        data = mj.MjData(mm, batch=2, dtype=dtype)
        sim = data.sim
        sim.set("qpos", _f32([[0.1, 0.45, 0.0], [-0.2, -0.1, 0.06]]))
        sim.set("qvel", _f32(rng.normal(size=(2, 3)) * 0.2))
        sim.set("ctrl", _f32([[0.3, 0.5], [-0.4, 0.2]]))
    elif name == "drone2":
        data = mj.MjData(mm, batch=2, dtype=dtype)
        sim = data.sim
        sim.reset(0)                                               # the hover keyframe, its ctrl included
        v = np.zeros((2, cm.nv)); v[1] = _f32(rng.normal(size=cm.nv) * 0.1)
        sim.set("qvel", v)
    elif name == "cartpole_sensors":
        # B = 9 on 8 lanes per environment: several points share a wave, and the last wave is partly filled
        data = mj.MjData(mm, batch=9, dtype=dtype, lanes=8)
        sim = data.sim
        sim.set("qpos", _f32(rng.uniform(-0.9, 0.9, size=(9, 2))))
        sim.set("qvel", _f32(rng.normal(size=(9, 2)) * 0.3))
        sim.set("ctrl", _f32(rng.uniform(-1, 1, size=(9, 1))))
    else:
        data = mj.MjData(mm, batch=2, dtype=dtype)
        sim = data.sim
        sim.set("qpos", _f32([[0.4], [-0.7]]))
        sim.set("qvel", _f32([[0.5], [-1.2]]))
        sim.set("ctrl", _f32([[0.3], [1.0]]))                      # [1]: at the upper bound, D's column is one-sided
    sim.sync()
    return data


@pytest.fixture(scope="module")
def runs(world):
    """(model, dtype) -> plain and sensor results of the specialised and of the generic kernel, centred and forward, plus the device
    state they were taken at and what the data object held before and after."""
    cache = {}

    def get(name, dtype):
        key = (name, dtype)
        if key in cache:
            return cache[key]
        cm, om, mm = world(name)
        data = _prepare(name, cm, mm, dtype)
        sim = data.sim
        keep = FIELDS + ("qacc", "time", "sensordata")
        before = {k: sim.get(k) for k in keep}
        out = {"pre": {k: before[k] for k in FIELDS}, "B": sim.batch}
        for kernel in ("spec", "generic"):
            if kernel == "generic":
                sim.unspecialize_fd()
            for centered in (True, False):
                plain = sim.transition_fd(EPS, centered)
                sens = sim.transition_fd(EPS, centered, sensors=True)
                out[(kernel, centered)] = (plain, sens)
            assert sim.fd_specialized is (kernel == "spec")      # the policy default loads the specialised FD kernel on the first call
        sim.sync()
        out["untouched"] = all(np.array_equal(before[k], sim.get(k)) for k in keep)
        cache[key] = out
        return out

    return get


# ---- 1. C, D against the oracle loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_sensor_jacobians_match_the_oracle_loop(world, runs, name, dtype):
    cm, om, _ = world(name)
    r = runs(name, dtype)
    worst = 0.0
    for centered in (True, False):
        _, _, C, D = r[("spec", centered)][1]
        assert C.shape == (r["B"], cm.nsensordata, 2 * cm.nv) and D.shape == (r["B"], cm.nsensordata, cm.nu)
        assert np.isfinite(C).all() and np.isfinite(D).all()
        for e in range(r["B"]):
            p = r["pre"]
            Co, Do = oracle_sensor_fd(om, cm, p["qpos"][e], p["qvel"][e], p["ctrl"][e], p["qacc_warmstart"][e], EPS, centered)
            ec = np.abs(C[e] - Co).max() / max(1.0, np.abs(Co).max())
            ed = np.abs(D[e] - Do).max() / max(1.0, np.abs(Do).max()) if cm.nu else 0.0
            print(f"fd_sensors {name} {dtype} centered={centered} env {e}: C err {ec:.3e} (max|C| {np.abs(Co).max():.3e}), D err {ed:.3e} (max|D| {np.abs(Do).max():.3e})")
            worst = max(worst, ec, ed)
    measured(f"fd_sensors/{name}/{dtype}", worst, FD_SENS_TOL[(name, dtype)])


# ---- 2. anchors that do not involve the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_jointpos_rows_are_unit_rows(world, runs, dtype):
    """Euler cart-pole: the sensors a step leaves are those of the forward pass at the perturbed point, so row i of C is the unit row of
    joint i's dof within the rounding of q +- 1e-6 at |q| <= 1 over 2e-6 (a few multiples of 5.6e-11), exactly 0 over dv; D is exactly 0."""
    cm, _, _ = world("cartpole_sensors")
    _, _, C, D = runs("cartpole_sensors", dtype)[("spec", True)][1]
    nv = cm.nv
    assert np.abs(C[:, :, :nv] - np.eye(nv)[None]).max() <= 1e-9
    assert np.all(C[:, :, nv:] == 0.0) and np.all(D == 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gyro_rows_are_the_site_rotation_transposed(runs, dtype):
    """Airborne puck: gyro = R_site' w with w the body-frame angular velocity qvel[3:6], so its rows of C over the angular dv columns
    are R_site', R_site from the imu site's quat 0.9659258 0 0.258819 0."""
    w, x, y, z = np.array([0.9659258, 0.0, 0.258819, 0.0]) / np.linalg.norm([0.9659258, 0.0, 0.258819, 0.0])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    _, _, C, _ = runs("site_wrench", dtype)[("spec", True)][1]
    for e in (0, 2):                                               # sensor order: accelerometer 0:3, gyro 3:6, framequat 6:10
        assert np.abs(C[e, 3:6, 9:12] - R.T).max() <= 1e-9


def test_model_without_sensors_gives_empty_blocks(world):
    import torch

    cm = mjcf.compile_xml_path(MODELS["cartpole"])
    data = mj.MjData(mj.MjModel.from_xml_path(MODELS["cartpole"]), batch=3, dtype="float64")
    sim = data.sim
    A0, B0 = sim.transition_fd(EPS, True)
    A, Bm, C, D = sim.transition_fd(EPS, True, sensors=True)
    assert cm.nsensordata == 0 and C.shape == (3, 0, 4) and D.shape == (3, 0, 1) and np.array_equal(A, A0) and np.array_equal(Bm, B0)
    q, v, u = sim.torch_view("qpos"), sim.torch_view("qvel"), sim.torch_view("ctrl")
    A2, B2, C2, D2 = sim.transition_fd_points(q, v, u, sensors=True)
    torch.cuda.synchronize()
    assert tuple(C2.shape) == (3, 0, 4) and tuple(D2.shape) == (3, 0, 1) and np.array_equal(A2.cpu().numpy(), A0)


# ---- 3. nothing else moves ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_a_b_are_bitwise_those_of_the_plain_call(runs, name, dtype):
    r = runs(name, dtype)
    for kernel in ("spec", "generic"):
        for centered in (True, False):
            (A0, B0), (A, Bm, C, D) = r[(kernel, centered)]
            assert np.array_equal(A, A0) and np.array_equal(Bm, B0), (kernel, centered)
    for centered in (True, False):                                 # one arithmetic: the specialised and the generic kernel agree bit for bit
        s, g = r[("spec", centered)][1], r[("generic", centered)][1]
        for a, b, what in zip(s, g, "ABCD"):
            assert np.array_equal(a, b), (what, centered)
    assert r["untouched"]                                         # state, warm start, qacc, time and sensordata of the data object


# ---- 4. points form -----------------------------------------------------------------------------------------------------------------------
def _site_wrench_points(world, dtype, order=(0, 1, 2)):
    """T = 2 trajectory of the B = 3 puck states (environments in `order`): linearize_rollout and the per-step host loop."""
    import torch

    cm, _, mm = world("site_wrench")
    tdt = torch.float32 if dtype == "float32" else torch.float64
    src = _prepare("site_wrench", cm, mm, dtype).sim
    st = {k: src.get(k)[list(order)] for k in FIELDS}
    u = torch.from_numpy(_f32([[[0.3, 0.4], [0.1, 0.2]], [[0.2, 0.5], [0.3, 0.1]], [[-0.5, 0.0], [-0.4, 0.0]]])[list(order)]).to(device="cuda", dtype=tdt)
    w0 = torch.from_numpy(st["qacc_warmstart"]).to(device="cuda", dtype=tdt)
    both = []
    for _ in range(2):
        d = mj.MjData(mm, batch=3, dtype=dtype)
        d.sim.set("qpos", st["qpos"]); d.sim.set("qvel", st["qvel"])
        d.sim.sync()
        both.append(d)
    fused, loop = both
    res = linearize_rollout(mm, fused, u, initial_warmstart=w0, sensor_derivatives=True)
    fused.sim.sync()
    torch.cuda.synchronize()
    sim = loop.sim
    sim.use_torch_stream()
    sim.torch_view("qacc_warmstart").copy_(w0)
    host = [[], [], [], []]
    for t in range(2):
        sim.torch_view("ctrl").copy_(u[:, t])
        sim.sync()
        for k, x in enumerate(sim.transition_fd(EPS, True, sensors=True)):
            host[k].append(x)
        sim.step(1)
    sim.sync()
    return [x.cpu().numpy() for x in res], [np.stack(x, axis=1) for x in host], fused.sim.fd_points_slabs()


@pytest.mark.parametrize("dtype", DTYPES)
def test_points_form_equals_the_host_loop_bitwise(world, dtype, monkeypatch):
    res, host, slabs = _site_wrench_points(world, dtype)
    assert slabs == 1
    assert res[4].shape == (3, 2, 10, 12) and res[5].shape == (3, 2, 10, 2)
    for got, want, what in zip(res[2:], host, "ABCD"):
        assert np.array_equal(got, want), what
    # the same in slabs of 2 points: 29 columns x (nq + nv + ns = 23) float64 = 5 336 bytes of scratch per point
    monkeypatch.setenv("MJB_FD_SLAB_BYTES", "12000")
    res2, _, slabs2 = _site_wrench_points(world, dtype)
    assert slabs2 >= 2
    for got, want, what in zip(res2, res, ("state", "sensordata") + tuple("ABCD")):
        assert np.array_equal(got, want), what
    monkeypatch.delenv("MJB_FD_SLAB_BYTES")
    # an environment's blocks do not depend on its position in the batch
    order = (2, 0, 1)
    res3, _, _ = _site_wrench_points(world, dtype, order)
    for k in (2, 3, 4, 5):
        assert np.array_equal(res3[k], res[k][list(order)]), "ABCD"[k - 2]


# ---- 5. linearize_rollout(sensor_derivatives=True) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_linearize_rollout_sensor_derivatives_predict_the_sensors(world, dtype):
    """C[:, t] dx_t + D[:, t] du_t is the change of sensordata[:, t] of a rollout restarted with dx = 1e-4 (state) or du = 1e-4
    (control), dx_t the state difference before step t: for jointpos sensors exact up to the second-order term, bound 1e-6."""
    import torch

    cm, _, mm = world("cartpole_sensors")
    tdt = torch.float32 if dtype == "float32" else torch.float64
    Bn, T, nq, nv, nu, ns = 4, 3, cm.nq, cm.nv, cm.nu, cm.nsensordata
    rng = np.random.default_rng(3)
    x0 = np.concatenate([np.zeros((Bn, 1)), rng.uniform(-0.5, 0.5, (Bn, nq)), rng.normal(size=(Bn, nv)) * 0.2], axis=1)
    u = rng.uniform(-1, 1, (Bn, T, nu))

    def run(x, uu, flag):
        data = mj.MjData(mm, batch=Bn, dtype=dtype)
        xt = torch.from_numpy(x).to(device="cuda", dtype=tdt)
        out = linearize_rollout(mm, data, torch.from_numpy(uu).to(device="cuda", dtype=tdt), initial_state=xt, sensor_derivatives=flag)
        torch.cuda.synchronize()
        return (*out, xt)

    plain, full = run(x0, u, False), run(x0, u, True)
    assert len(plain) == 5 and len(full) == 7
    for a, b, what in zip(plain, full, ("state", "sensordata", "A", "B")):
        assert torch.equal(a, b), what
    state, sens, A, Bm, C, D, xt = full
    assert tuple(C.shape) == (Bn, T, ns, 2 * nv) and tuple(D.shape) == (Bn, T, ns, nu) and C.dtype == torch.float64 and not C.is_contiguous()
    pre = torch.cat([xt[:, None, 1:], state[:, :-1, 1:]], dim=1).double()             # the state before step t
    for dx, du in ((np.concatenate([[0.0], 1e-4 * np.array([1.0, -0.5, 0.3, 0.8])]), 0.0), (np.zeros(1 + nq + nv), 1e-4)):
        state2, sens2, _, _, xt2 = run(x0 + dx[None], u + du, False)
        pre2 = torch.cat([xt2[:, None, 1:], state2[:, :-1, 1:]], dim=1).double()
        dxt = pre2 - pre                                                             # slide and hinge: the tangent difference is the plain one
        dut = torch.full((Bn, T, nu), du, dtype=torch.float64, device="cuda")           # (float32 data: u + du is rounded at 6e-8, D of a jointpos sensor is 0)
        pred = (C @ dxt[..., None] + D @ dut[..., None])[..., 0]
        err = float((sens2.double() - sens.double() - pred).abs().max())
        assert err <= 1e-6, err                                                      # (float32 sensordata carries its own rounding, 6e-8 at |q| <= 1)


# ---- 6. mjd_transitionFD fills the caller's C, D ------------------------------------------------------------------------------------------
def test_mjd_transition_fd_fills_c_and_d(world):
    cm, _, mm = world("cartpole_sensors")
    nx, nu, ns = 2 * cm.nv, cm.nu, cm.nsensordata
    for batch in (1, 3):
        data = mj.MjData(mm, batch=batch, dtype="float64")
        data.sim.set("qpos", _f32(np.linspace(-0.4, 0.6, 2 * batch).reshape(batch, 2)))
        data.sim.sync()
        lead = () if batch == 1 else (batch,)
        A, Bm = np.zeros(lead + (nx, nx)), np.zeros(lead + (nx, nu))
        C, D = np.full(lead + (ns, nx), 7.0), np.full(lead + (ns, nu), 7.0)
        mj.mjd_transitionFD(mm, data, EPS, True, A, Bm, C, D)
        A0, B0, C0, D0 = data.sim.transition_fd(EPS, True, sensors=True)
        assert not np.any(C == 7.0) and not np.any(D == 7.0)
        assert np.array_equal(C, C0[0] if batch == 1 else C0) and np.array_equal(D, D0[0] if batch == 1 else D0)
        assert np.array_equal(A, A0[0] if batch == 1 else A0) and np.abs(C[..., :cm.nv] - np.eye(cm.nv)).max() <= 1e-9
        A1, B1 = np.zeros_like(A), np.zeros_like(Bm)
        mj.mjd_transitionFD(mm, data, EPS, True, A1, B1, None, None)                # the reference-shaped call
        assert np.array_equal(A1, A) and np.array_equal(B1, Bm)


# ---- 7. argument checks -------------------------------------------------------------------------------------------------------------------
def test_points_sensors_argument_checks(world):
    import torch

    from tests.test_gpu_rollout_ctrl import _hip_runtime

    cm, _, mm = world("cartpole_sensors")
    Bn, nq, nv, nu, nx, ns = 3, cm.nq, cm.nv, cm.nu, 2 * cm.nv, cm.nsensordata
    sim = mj.MjData(mm, batch=Bn, dtype="float64").sim
    q, v, u = sim.torch_view("qpos"), sim.torch_view("qvel"), sim.torch_view("ctrl")
    opt = dict(dtype=torch.float64, device="cuda")
    A, Bm = torch.full((Bn, nx, nx), -3.0, **opt), torch.full((Bn, nx, nu), -3.0, **opt)
    C, D = torch.full((Bn, ns, nx), -3.0, **opt), torch.full((Bn, ns, nu), -3.0, **opt)
    L = load_library()
    torch.cuda.synchronize()

    def raw(C_, D_):
        vp = ctypes.c_void_p
        return L.mjb_transition_fd_points_sensors(sim.ptr, 1, vp(q.data_ptr()), 0, nq, vp(v.data_ptr()), 0, nv, vp(u.data_ptr()), 0, nu, None, 0, 0,
                                                  EPS, 1, vp(A.data_ptr()), vp(Bm.data_ptr()), vp(C_) if C_ else None, vp(D_) if D_ else None)

    assert raw(0, D.data_ptr()) == -1 and raw(C.data_ptr(), 0) == -1             # NULL with ns > 0 (and nu > 0): MJB_ERR_ARG
    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    assert _hip_runtime().hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(C.data_ptr())) == 0
    c_ok = (base.value + size.value - C.data_ptr()) // 8
    assert raw(C.data_ptr() + 8 * (c_ok - Bn * ns * nx + 1), D.data_ptr()) == -1   # the C blocks would end one element past the allocation
    torch.cuda.synchronize()
    for x in (A, Bm, C, D):
        assert bool((x == -3.0).all())                                           # nothing was launched
    assert raw(C.data_ptr(), D.data_ptr()) == 0
    torch.cuda.synchronize()
    sim.sync()
    A0, B0, C0, D0 = sim.transition_fd(EPS, True, sensors=True)
    for got, want in zip((A, Bm, C, D), (A0, B0, C0, D0)):
        assert np.array_equal(got.cpu().numpy(), want)
