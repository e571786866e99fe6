"""GPU parity at 33..64 dofs (tests/large_models.py): above nv = 32 the step kernel factors M, the Newton Hessian and M + h diag(damping)
with the register-tiled Cholesky on the 8x8 lane grid (tile_factor) and solves with chol_solve; J^T f is not split over the wave halves;
the 64-bit dof masks fill up to bit 63.  The product kernels through the C ABI against the float64 oracle.  Tolerances as in
test_gpu_parity.py: float64 <= 1e-9; every fp32 tolerance goes through tests.conftest.measured() at <= 3x the value measured on an
MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mujoco_template_amd import mjcf  # noqa: E402
from mujoco_template_amd._capi import CTRL_RANDOM, BatchSim, DeviceModel  # noqa: E402
from mujoco_template_amd.exceptions import ConfigError  # noqa: E402
from oracle import mjo  # noqa: E402
from tests.conftest import chain_xml, measured  # noqa: E402
from tests.large_models import LARGE_MODELS, initial_state  # noqa: E402

NAMES = ["chain33", "chain40", "chain57", "chain64", "tree", "two_free"]
CAPS = dict(nconmax=24, nefcmax=96)             # explicit: the automatic caps of a 64-dof model trade rows for occupancy

# fp32, teacher-forced, 30 steps: (qacc rel, dqpos, dqvel rel) = 3x measured on an MI355X
TF_TOL32 = {"chain33": (9.1e-05, 4.6e-08, 5.4e-06), "chain40": (0.00015, 7.2e-08, 1.5e-05), "chain57": (0.00043, 8.2e-08, 1.7e-05), "chain64": (0.00059, 3.1e-07, 6.1e-05), "tree": (9.7e-06, 4.2e-08, 5.7e-06), "two_free": (2.2e-05, 2.3e-07, 2.3e-05)}
LANES_TOL32 = {8: (4.7e-05, 8.7e-08, 2.5e-06), 16: (3.4e-05, 7.7e-08, 2.2e-06)}                   # chain17 at 8 / 16 lanes per environment
INV_TOL32 = {"tree": 2e-06, "two_free": 1.1e-06}


@pytest.fixture(scope="module")
def large():
    cache = {}

    def get(name):
        if name not in cache:
            xml = chain_xml(17) if name == "chain17" else LARGE_MODELS[name]()
            cm = mjcf.compile_xml_string(xml)
            cache[name] = (cm, mjo.OracleModel(cm), DeviceModel(cm))
        return cache[name]

    return get


def _states(cm, name, B, seed):
    rng = np.random.default_rng(seed)
    qv = [initial_state(cm, name, rng) for _ in range(B)]
    return np.stack([q for q, _ in qv]), np.stack([v for _, v in qv])


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max())))


@pytest.mark.parametrize("name", NAMES)
def test_large_nv_float64_forward_and_free_running_match_oracle(large, name):
    """float64, 64 lanes: forward phases (qM, bias, passive, actuation, qacc_smooth, constraint force, qacc, constraint rows) and 30
    free-running steps under random control, against the oracle at <= 1e-9 relative; no row or contact dropped."""
    cm, om, dm = large(name)
    B = 4
    q, v = _states(cm, name, B, 1)
    sim = BatchSim(dm, B, dtype="float64", lanes=64, **CAPS)
    assert sim.lanes == 64
    sim.set("qpos", q); sim.set("qvel", v)
    sim.debug_forward()
    ods = [mjo.OracleData(om) for _ in range(B)]
    for e, od in enumerate(ods):
        od.qpos[:] = q[e]; od.qvel[:] = v[e]; od.forward()
    worst = 0.0
    for key in ("qM", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "qacc_smooth", "qfrc_constraint"):
        worst = max(worst, _rel(sim.debug_get(key), np.stack([getattr(od, key) for od in ods])))
    worst = max(worst, _rel(sim.get("qacc"), np.stack([od.qacc for od in ods])))
    assert worst <= 1e-9, worst
    cn = sim.counters()
    assert cn["nefc"].tolist() == [od.counters()["nefc"] for od in ods] and max(cn["nefc"]) >= 8
    J = sim.debug_get("efc_J").reshape(B, sim.nefcmax, cm.nv)
    for e, od in enumerate(ods):
        n = od.counters()["nefc"]
        if n:
            assert _rel(J[e, :n], od.efc_J.reshape(n, cm.nv)) <= 1e-9
    steps = 30
    sim.set("qpos", q); sim.set("qvel", v)
    sim.rollout(steps, CTRL_RANDOM, seed=5)
    qT, vT = mjo.rollout_batch(om, B, steps, seed=5, nthreads=4, qpos_init=q, qvel_init=v)
    assert _rel(sim.get("qpos"), qT) <= 1e-9 and _rel(sim.get("qvel"), vT) <= 1e-9
    cn = sim.counters()
    assert cn["efc_dropped"].sum() == 0 and cn["con_dropped"].sum() == 0


def _teacher_forced(sims, om, cm, name, B, seed, steps, ctrl_seed):
    """Step every BatchSim of `sims` one step at a time from the oracle's states; returns the worst (qacc rel, dqpos, dqvel rel) of
    sims[0], the largest row count, and asserts that all sims stay bitwise equal to sims[0]."""
    q, v = _states(cm, name, B, seed)
    ods = [mjo.OracleData(om) for _ in range(B)]
    for e, od in enumerate(ods):
        od.qpos[:] = q[e]; od.qvel[:] = v[e]
    worst_a = worst_q = worst_v = 0.0
    rows = 0
    for s in range(steps):
        u = np.stack([od.random_ctrl(ctrl_seed, e, s, 1.0) for e, od in enumerate(ods)])
        for x in sims:
            x.set("qpos", np.stack([od.qpos for od in ods])); x.set("qvel", np.stack([od.qvel for od in ods]))
            x.set("qacc_warmstart", np.stack([od.qacc_warmstart for od in ods])); x.set("ctrl", u)
            x.step(1)
        for e, od in enumerate(ods):
            od.ctrl[:] = u[e]; od.step()
        rows = max(rows, max(od.counters()["nefc"] for od in ods))
        ao, qo, vo = np.stack([od.qacc for od in ods]), np.stack([od.qpos for od in ods]), np.stack([od.qvel for od in ods])
        worst_a = max(worst_a, _rel(sims[0].get("qacc"), ao))
        worst_q = max(worst_q, float(np.abs(sims[0].get("qpos") - qo).max()))
        worst_v = max(worst_v, float((np.abs(sims[0].get("qvel") - vo) / np.maximum(1.0, np.abs(vo))).max()))
        for x in sims[1:]:
            assert np.array_equal(sims[0].get("qpos"), x.get("qpos")) and np.array_equal(sims[0].get("qacc"), x.get("qacc")), s
    for x in sims:
        cn = x.counters()
        assert cn["efc_dropped"].sum() == 0 and cn["con_dropped"].sum() == 0
    return worst_a, worst_q, worst_v, rows


@pytest.mark.parametrize("name", NAMES)
def test_large_nv_fp32_teacher_forced_and_specialised_equals_generic(large, name):
    """fp32 product path, 64 lanes, teacher-forced along the oracle's trajectory under random control for 30 steps: qacc (relative),
    one-step qpos and qvel (relative).  The specialised kernel is bitwise equal to the generic one at every step."""
    cm, om, dm = large(name)
    B = 8
    sim = BatchSim(dm, B, dtype="float32", lanes=64, **CAPS)
    gen = BatchSim(dm, B, dtype="float32", lanes=64, specialize=False, **CAPS)
    assert sim.lanes == 64 and sim.specialized and not gen.specialized
    wa, wq, wv, rows = _teacher_forced([sim, gen], om, cm, name, B, cm.nv, 30, 5)
    assert rows >= 8                                                      # the Hessian path was taken
    measured(f"large_nv/{name}/qacc_rel", wa, TF_TOL32[name][0])
    measured(f"large_nv/{name}/qpos", wq, TF_TOL32[name][1])
    measured(f"large_nv/{name}/qvel_rel", wv, TF_TOL32[name][2])


@pytest.mark.parametrize("lanes", [8, 16])
def test_fp32_fewer_lanes_than_dofs_teacher_forced(large, lanes):
    """fp32 with 8 or 16 lanes per environment on a 17-dof chain in floor contact: the generic LDS Cholesky (chol_factor, strided
    chol_solve) against the oracle, teacher-forced.  Only the host emulation reached this branch in fp32 before."""
    cm, om, dm = large("chain17")
    B = 8
    sim = BatchSim(dm, B, dtype="float32", lanes=lanes, nconmax=16, nefcmax=72)
    assert sim.lanes == lanes < cm.nv
    wa, wq, wv, rows = _teacher_forced([sim], om, cm, "chain17", B, lanes, 30, 6)
    assert rows >= 8
    measured(f"lanes{lanes}/chain17/qacc_rel", wa, LANES_TOL32[lanes][0])
    measured(f"lanes{lanes}/chain17/qpos", wq, LANES_TOL32[lanes][1])
    measured(f"lanes{lanes}/chain17/qvel_rel", wv, LANES_TOL32[lanes][2])


@pytest.mark.parametrize("name", ["tree", "two_free"])
def test_large_nv_inverse_dynamics_matches_oracle(large, name):
    """mjb_inverse at 45 / 64 dofs, states in contact, random qacc: float64 <= 1e-9 relative, fp32 measured; actuator moments."""
    cm, om, dm = large(name)
    B = 4
    q, v = _states(cm, name, B, 3)
    a = np.random.default_rng(3).normal(size=(B, cm.nv))
    ods = []
    for e in range(B):
        od = mjo.OracleData(om)
        od.qpos[:] = q[e]; od.qvel[:] = v[e]; od.qacc[:] = a[e]
        od.inverse(); ods.append(od)
    ref = np.stack([od.qfrc_inverse for od in ods])
    for dtype in ("float64", "float32"):
        sim = BatchSim(dm, B, dtype=dtype, lanes=64, **CAPS)
        sim.set("qpos", q); sim.set("qvel", v); sim.set("qacc", a)
        sim.inverse()
        err = _rel(sim.get("qfrc_inverse"), ref)
        if dtype == "float64":
            assert err <= 1e-9, err
            assert np.abs(sim.get("actuator_moment") - np.stack([od.actuator_moment for od in ods])).max() <= 1e-12
        else:
            measured(f"large_nv_inverse/{name}/fp32", err, INV_TOL32[name], "(relative to the largest generalized force)")


def test_large_nv_transition_fd_float64_matches_oracle(large):
    """Finite-difference transition matrices at 45 dofs (A is 90 x 90): device float64 FD against the oracle's FD."""
    cm, om, dm = large("tree")
    B = 2
    q, v = _states(cm, "tree", B, 4)
    u = np.random.default_rng(4).uniform(-0.5, 0.5, size=(B, cm.nu))
    sim = BatchSim(dm, B, dtype="float64", lanes=64, **CAPS)
    sim.set("qpos", q); sim.set("qvel", v); sim.set("ctrl", u)
    A, Bm = sim.transition_fd(1e-6, True)
    assert A.shape == (B, 2 * cm.nv, 2 * cm.nv) and Bm.shape == (B, 2 * cm.nv, cm.nu)
    od = mjo.OracleData(om)
    for e in range(B):
        od.reset(); od.qpos[:] = q[e]; od.qvel[:] = v[e]; od.ctrl[:] = u[e]
        Ao, Bo = od.transition_fd(1e-6, True)
        assert _rel(A[e], Ao) <= 1e-7 and _rel(Bm[e], Bo) <= 1e-7, e     # FD quotients of states that agree to ~1e-15


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_large_nv_caps_fit_or_fail_cleanly(large, dtype):
    """Default caps at 64 dofs either fit the 160 KiB of LDS (recorded in DESIGN.md §7) or creation fails with the clean ConfigError;
    caps far beyond the budget always fail cleanly."""
    cm, om, dm = large("chain64")
    try:
        sim = BatchSim(dm, 2, dtype=dtype, lanes=64)
    except ConfigError as exc:
        assert "exceeds 160 KiB" in str(exc)
    else:
        assert sim.lds_bytes_per_env <= 160 * 1024 and sim.nefcmax >= 8 and sim.nconmax >= 1
    with pytest.raises(ConfigError, match="exceeds 160 KiB"):
        BatchSim(dm, 2, dtype=dtype, lanes=64, nconmax=64, nefcmax=600)
