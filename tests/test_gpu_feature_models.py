"""GPU parity of the feature scenes (tests/feature_models.py): every accepted MJCF feature through the HIP kernels — float64 against
the oracle, fp32 teacher-forced against the oracle, the specialised kernel (model baked in as constant data, branches folded on the
model's properties) and the two-wave kernel bitwise against the generic one-wave kernel, both lane layouts, the float64 finite
differences, and the run-time solver options on a baked model.  fp32 tolerances are <= 3x what was measured on an MI355X
 and go through tests.conftest.measured()."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mujoco_template_amd._capi import CTRL_RANDOM, BatchSim, DeviceModel  # noqa: E402
from mujoco_template_amd import mjcf  # noqa: E402
from oracle import mjo  # noqa: E402
from tests.conftest import measured  # noqa: E402
from tests.feature_models import SCENES, SOLVER_OPTS  # noqa: E402

NAMES = list(SCENES)
# fp32 teacher-forced single step (|dqpos|, |dqvel| / max(1, |qvel|)) and float64 finite differences (relative): 3x measured
# (measured: servo_arm 2.9e-8 / 1.8e-6, tendon_limits 2.8e-8 / 4.5e-7, contact_mix 8.3e-8 / 2.1e-6, rk4_contact 3.3e-8 / 2.6e-6,
# site_wrench 8.4e-8 / 4.8e-7; finite differences servo_arm 6.4e-10, contact_mix 1.5e-9)
STEP_TOL32 = {"servo_arm": (8.8e-8, 5.5e-6), "tendon_limits": (8.3e-8, 1.4e-6), "contact_mix": (2.5e-7, 6.2e-6), "rk4_contact": (1e-7, 7.7e-6),
              "site_wrench": (2.5e-7, 1.5e-6)}
FD_TOL64 = {"servo_arm": 1.9e-9, "contact_mix": 4.6e-9}


@pytest.fixture(scope="module")
def world():
    cache = {}

    def get(name):
        if name not in cache:
            cm = mjcf.compile_xml_string(SCENES[name].xml)
            cache[name] = (cm, mjo.OracleModel(cm), DeviceModel(cm))
        return cache[name]

    return get


def random_states(cm, od, B, seed, qs=0.05, vs=0.2):
    rng = np.random.default_rng(seed)
    q = np.stack([od.integrate_pos(cm.qpos0, rng.normal(size=cm.nv) * qs, 1.0) for _ in range(B)])
    v = rng.normal(size=(B, cm.nv)) * vs
    return q, v


def _oracle_rollouts(om, q, v, steps, seed, scale):
    """Per-environment oracle rollouts under the kernels' random controls; (qpos, qvel, counters) of each."""
    out = []
    for e in range(q.shape[0]):
        od = mjo.OracleData(om)
        od.qpos[:] = q[e]; od.qvel[:] = v[e]
        od.rollout_random(steps, seed, e, 0, scale)
        c = od.counters()
        out.append((od.qpos.copy(), od.qvel.copy(), (c["ncon"], c["nefc"], c["solver_niter"])))
    return out


def _counters(sim):
    cn = sim.counters()
    return [(int(a), int(b), int(c)) for a, b, c in zip(cn["ncon"], cn["nefc"], cn["solver_niter"])]


@pytest.mark.parametrize("name", NAMES)
def test_float64_free_running_matches_oracle(world, name):
    cm, om, dm = world(name)
    B, T = 16, 100
    q, v = random_states(cm, mjo.OracleData(om), B, 3)
    sim = BatchSim(dm, B, dtype="float64")
    sim.set("qpos", q); sim.set("qvel", v)
    sim.rollout(T, CTRL_RANDOM, seed=7, ctrl_scale=SCENES[name].ctrl_scale)
    ref = _oracle_rollouts(om, q, v, T, 7, SCENES[name].ctrl_scale)
    assert np.abs(sim.get("qpos") - np.stack([r[0] for r in ref])).max() <= 1e-9
    assert np.abs(sim.get("qvel") - np.stack([r[1] for r in ref])).max() <= 1e-7
    assert _counters(sim) == [r[2] for r in ref]
    cn = sim.counters()
    assert cn["efc_dropped"].sum() == 0 and cn["con_dropped"].sum() == 0
    if SCENES[name].contacts:
        assert max(r[2][0] for r in ref) > 0


@pytest.mark.parametrize("name", NAMES)
def test_fp32_teacher_forced_single_step(world, name):
    cm, om, dm = world(name)
    B, T = 8, 60
    sim = BatchSim(dm, B, dtype="float32")
    ods = [mjo.OracleData(om) for _ in range(B)]
    q, v = random_states(cm, ods[0], B, 4)
    for e, od in enumerate(ods):
        od.qpos[:] = q[e]; od.qvel[:] = v[e]
    worst_q = worst_v = 0.0
    for s in range(T):
        u = np.stack([od.random_ctrl(9, e, s, SCENES[name].ctrl_scale) for e, od in enumerate(ods)])
        sim.set("qpos", np.stack([od.qpos for od in ods])); sim.set("qvel", np.stack([od.qvel for od in ods]))
        sim.set("qacc_warmstart", np.stack([od.qacc_warmstart for od in ods])); sim.set("ctrl", u)
        sim.step(1)
        for e, od in enumerate(ods):
            od.ctrl[:] = u[e]; od.step()
        qo, vo = np.stack([od.qpos for od in ods]), np.stack([od.qvel for od in ods])
        worst_q = max(worst_q, np.abs(sim.get("qpos") - qo).max())
        worst_v = max(worst_v, (np.abs(sim.get("qvel") - vo) / np.maximum(1.0, np.abs(vo))).max())
    measured(f"feature_models/teacher_forced_step/{name}/qpos", worst_q, STEP_TOL32[name][0])
    measured(f"feature_models/teacher_forced_step/{name}/qvel_rel", worst_v, STEP_TOL32[name][1])


def _spec_or_skip(dm):
    import mujoco_template_amd._capi as capi

    try:
        capi.compile_spec(dm.spec_source())
    except capi.TemplateError as exc:
        pytest.skip(f"specialised kernel cannot be built here: {exc}")


def _fp32_run(dm, B, T, name, **kw):
    sim = BatchSim(dm, B, dtype="float32", **kw)
    sim.rollout(T, CTRL_RANDOM, seed=9, ctrl_scale=SCENES[name].ctrl_scale)
    return sim, [sim.get(k) for k in ("qpos", "qvel", "qacc", "xpos")] + [sim.counters()[k] for k in ("ncon", "nefc", "solver_niter")]


@pytest.mark.parametrize("name", NAMES)
def test_specialised_kernel_is_bitwise_identical_to_the_generic_one(world, name):
    cm, om, dm = world(name)
    _spec_or_skip(dm)
    spec, a = _fp32_run(dm, 64, 120, name)
    gen, b = _fp32_run(dm, 64, 120, name, specialize=False)
    assert spec.specialized and not gen.specialized
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.isfinite(a[0]).all()
    if SCENES[name].contacts:
        assert a[4].max() > 0


TWO_WAVE = [n for n in NAMES if 'integrator="RK4"' not in SCENES[n].xml]      # the two-wave kernel: fp32, 64 lanes, nv <= 32, Euler


@pytest.mark.parametrize("spec", [None, False])
@pytest.mark.parametrize("name", TWO_WAVE)
def test_two_wave_kernel_is_bitwise_identical_to_the_one_wave_kernel(world, name, spec, monkeypatch):
    cm, om, dm = world(name)
    assert cm.nv <= 32 and dm.step2_spec_source(lanes=64) is not None
    res = {}
    for mode in ("0", "policy"):
        if mode == "0":
            monkeypatch.setenv("MJB_TWO_WAVE", "0")
        else:
            monkeypatch.delenv("MJB_TWO_WAVE")
        sim, res[mode] = _fp32_run(dm, 37, 120, name, specialize=spec, lanes=64)
        assert sim.schedule_info()["waves_per_env"] == (1 if mode == "0" else 2)
    for x, y in zip(res["0"], res["policy"]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", NAMES)
def test_lanes_per_env_variants_agree(world, name):
    cm, om, dm = world(name)
    B, T = 8, 100
    q, v = random_states(cm, mjo.OracleData(om), B, 5)
    ref = _oracle_rollouts(om, q, v, T, 2, SCENES[name].ctrl_scale)
    got = {}
    for lanes in (16, 64):
        sim = BatchSim(dm, B, dtype="float64", lanes=lanes)
        assert sim.lanes == lanes
        sim.set("qpos", q); sim.set("qvel", v)
        sim.rollout(T, CTRL_RANDOM, seed=2, ctrl_scale=SCENES[name].ctrl_scale)
        got[lanes] = sim.get("qpos")
        assert np.abs(got[lanes] - np.stack([r[0] for r in ref])).max() <= 1e-9, lanes
        assert _counters(sim) == [r[2] for r in ref], lanes
    assert np.abs(got[16] - got[64]).max() <= 1e-10


@pytest.mark.parametrize("name", list(FD_TOL64))
def test_transition_fd_matches_oracle(world, name):
    cm, om, dm = world(name)
    B = 4
    od = mjo.OracleData(om)
    q, v = random_states(cm, od, B, 7, qs=0.02, vs=0.1)
    u = np.stack([od.random_ctrl(1, e, 0, 0.5) for e in range(B)])
    sim = BatchSim(dm, B, dtype="float64")
    sim.set("qpos", q); sim.set("qvel", v); sim.set("ctrl", u)
    A, Bm = sim.transition_fd(1e-6, True)
    worst = 0.0
    for e in range(B):
        od.reset(); od.qpos[:] = q[e]; od.qvel[:] = v[e]; od.ctrl[:] = u[e]
        Ao, Bo = od.transition_fd(1e-6, True)
        worst = max(worst, np.abs(A[e] - Ao).max() / max(1.0, np.abs(Ao).max()),
                    np.abs(Bm[e] - Bo).max() / max(1.0, np.abs(Bo).max()) if cm.nu else 0.0)
    measured(f"feature_models/transition_fd/{name}", worst, FD_TOL64[name], "(relative to the largest entry of A / B)")
    assert np.array_equal(sim.get("qpos"), q)


def test_run_time_options_are_not_baked_into_the_specialised_kernel():
    """set_solver / set_disableactuator after the data objects exist: the specialised and the generic fp32 kernels still agree bit for
    bit, float64 follows the oracle under the same options, and the solver stops at the iteration cap."""
    name = SOLVER_OPTS["scene"]
    cm = mjcf.compile_xml_string(SCENES[name].xml)
    om, dm = mjo.OracleModel(cm), DeviceModel(cm)
    _spec_or_skip(dm)
    B, T, scale = 16, 80, SCENES[name].ctrl_scale
    q, v = random_states(cm, mjo.OracleData(om), B, 6)
    sims = {"spec": BatchSim(dm, B, dtype="float32"), "gen": BatchSim(dm, B, dtype="float32", specialize=False),
            "f64": BatchSim(dm, B, dtype="float64")}
    assert sims["spec"].specialized
    for sim in sims.values():                                # a first launch with the compiled options
        sim.set("qpos", q); sim.set("qvel", v)
        sim.rollout(1, CTRL_RANDOM, seed=4, ctrl_scale=scale)
    q1, v1, w1 = sims["f64"].get("qpos"), sims["f64"].get("qvel"), sims["f64"].get("qacc_warmstart")
    for m in (dm, om):
        m.set_solver(SOLVER_OPTS["iterations"], SOLVER_OPTS["tolerance"])
        m.set_disableactuator(SOLVER_OPTS["disableactuator"])
    for sim in sims.values():
        sim.set("qpos", q1); sim.set("qvel", v1); sim.set("qacc_warmstart", w1)     # two Newton iterations: the warm start matters
        sim.rollout(T, CTRL_RANDOM, seed=4, step0=1, ctrl_scale=scale)
    a = [sims["spec"].get(k) for k in ("qpos", "qvel", "qacc")]
    b = [sims["gen"].get(k) for k in ("qpos", "qvel", "qacc")]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    niter = []
    qT = []
    for e in range(B):
        od = mjo.OracleData(om)
        od.qpos[:] = q1[e]; od.qvel[:] = v1[e]; od.qacc_warmstart[:] = w1[e]
        for s in range(T):
            od.ctrl[:] = od.random_ctrl(4, e, 1 + s, scale)
            od.step()
            niter.append(od.counters()["solver_niter"])
        qT.append(od.qpos.copy())
    assert max(niter) == SOLVER_OPTS["iterations"]           # the cap binds
    assert np.abs(sims["f64"].get("qpos") - np.stack(qT)).max() <= 1e-9
    for sim in sims.values():
        assert sim.counters()["solver_niter"].max() <= SOLVER_OPTS["iterations"]
    # the options changed the trajectory: the same run with the compiled options differs
    ref = BatchSim(DeviceModel(cm), B, dtype="float64")
    ref.set("qpos", q1); ref.set("qvel", v1); ref.set("qacc_warmstart", w1)
    ref.rollout(T, CTRL_RANDOM, seed=4, step0=1, ctrl_scale=scale)
    assert np.abs(ref.get("qpos") - sims["f64"].get("qpos")).max() > 1e-6
