"""The data object's grow-on-demand and lazily made memory blocks (``csrc/mjb_buffer.hpp`` behind ``mjb_api.hip``): every block is
grown, shrunk-in-use and reused on ONE data object and the results are compared with a fresh object's (bitwise) or with the
host law; then the ordinary life cycle - create, touch every lazily made block, drop - twenty times.

The models are the pendulum and the cart-pole at batch 3.  One test needs larger arrays: the pinned staging block of the array
getters / setters has a floor of 4096 bytes, and at batch 3 no array of these models reaches it, so that test also runs a batch of
200, at which the arrays it sends lie on both sides of the floor (the test asserts that they do)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mujoco_template_amd as mt  # noqa: E402
from mujoco_template_amd import mj, mjcf  # noqa: E402
from mujoco_template_amd._capi import CTRL_RANDOM, BatchSim, DeviceModel  # noqa: E402
from tests.conftest import MODELS, measured  # noqa: E402

NAMES = ("pendulum", "cartpole")
DTYPES = ("float32", "float64")
B3 = 3
# mjb_feedback_ctrl in fp32 against the float64 numpy law, relative to max(1, largest ctrl): the bound of
# test_batched_feedback_gemm_kernel_matches_the_host_law for the cart-pole (API_TOL32["gemm"]["cartpole"], K dx over 2 nv = 4 terms, nu = 1).
# That test has no pendulum case; its law has 2 nv = 2 terms and nu = 1, so it rounds no more often, the inputs below are drawn at that
# test's scales, and the same bound is taken.  float64: that test's 1e-12.
FEEDBACK_TOL32 = {"pendulum": 7.5e-8, "cartpole": 7.5e-8}
FEEDBACK_TOL64 = 1e-12


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name):
        if name not in cache:
            cm = mjcf.compile_xml_path(MODELS[name])
            cache[name] = (cm, DeviceModel(cm))
        return cache[name]

    return get


def _scatter(sim, cm, seed):
    """The same scattered state on every object made with the same seed (fp32-representable, so both dtypes hold it exactly)."""
    rng = np.random.default_rng(seed)
    q = (np.asarray(cm.qpos0, dtype=np.float64) + rng.normal(size=(sim.batch, cm.nq)) * 0.1).astype(np.float32).astype(np.float64)
    v = (rng.normal(size=(sim.batch, cm.nv)) * 0.3).astype(np.float32).astype(np.float64)
    u = (rng.uniform(-0.5, 0.5, size=(sim.batch, cm.nu))).astype(np.float32).astype(np.float64)
    sim.set("qpos", q), sim.set("qvel", v), sim.set("ctrl", u)
    return q, v, u


@pytest.mark.parametrize("name", NAMES)
def test_feedback_noise_tables_replace_each_other(name):
    """Noise tables of 4, then 64, then 2 steps on one data object, float32 and float64: after each, ``feedback_ctrl`` is the numpy law
    with the NEWEST table (a longer table needs new blocks, a shorter one reuses them; nothing of an earlier table may be read), then
    with the noise switched off."""
    rng = np.random.default_rng(5)
    for dtype in DTYPES:
        h = mt.ModelHandle.from_xml_path(MODELS[name], batch=B3, dtype=dtype)
        m, d = h.model, h.data
        K = rng.normal(size=(m.nu, 2 * m.nv)) * 0.2
        ctl = mt.LinearFeedbackController(K=K, ctrl0=rng.uniform(-0.2, 0.2, size=m.nu), qpos_goal=np.array(m.qpos0), qvel_goal=rng.normal(size=m.nv) * 0.01,
                                          ctrl_noise_std=rng.uniform(0.0, 0.05, size=m.nu), perturbations=rng.normal(size=(4, m.nu)), env_stride=3)
        ctl.prepare(m, d)
        dq = rng.normal(size=(B3, m.nv)) * 0.1
        q = np.tile(np.array(m.qpos0), (B3, 1))
        mj.mj_integratePos(m, q, dq, 1.0)
        d.qpos[:] = q
        d.qvel[:] = rng.normal(size=(B3, m.nv)) * 0.3
        for nsteps in (4, 64, 2, 0):
            if nsteps:
                ctl.perturbations = rng.normal(size=(nsteps, m.nu))
                ctl.ctrl_noise_std = rng.uniform(0.0, 0.05, size=m.nu)
            else:
                ctl.perturbations = ctl.ctrl_noise_std = None
            ctl._uploaded = None                                 # the next call uploads gains and noise again
            for step in (0, 1, 5, 63):
                ctl.step_count = step
                want = ctl.host_law(m, d, step)
                ctl(m, d, 0.0)
                got = np.array(d.ctrl)
                assert got.shape == (B3, m.nu)
                err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
                print(f"feedback noise {name} {dtype} nsteps={nsteps} step={step}: err {err:.3e}")
                if dtype == "float32":
                    measured(f"buffers/feedback_noise/{name}/fp32", err, FEEDBACK_TOL32[name], "(relative to the largest ctrl)")
                else:
                    assert err <= FEEDBACK_TOL64, (name, nsteps, step, err)
            if nsteps:                                           # the noise term is a visible part of the law: without it ctrl differs
                table, ctl.perturbations = ctl.perturbations, None
                assert np.abs(ctl.host_law(m, d, 63) - want).max() > 1e-6
                ctl.perturbations = table


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_jac_requests_of_changing_size(models, name, dtype):
    """``jac`` with 1, then 5, then 2 requests on one object: each result is bitwise that of a fresh object given the same request."""
    cm, dm = models(name)
    body = cm.nbody - 1
    requests = [([1], [body]), ([0, 1, 2, 3, 1], [0, body, body, body, 0]), ([3, 0], [body, 0])]
    one = BatchSim(dm, B3, dtype=dtype, specialize=False)
    _scatter(one, cm, 1)
    for kinds, ids in requests:
        fresh = BatchSim(dm, B3, dtype=dtype, specialize=False)
        _scatter(fresh, cm, 1)
        jp, jr = one.jac(kinds, ids)
        fp, fr = fresh.jac(kinds, ids)
        assert jp.shape == (B3, len(kinds), 3, cm.nv)
        assert np.array_equal(jp, fp) and np.array_equal(jr, fr), (kinds, ids)
        assert np.isfinite(jp).all() and np.isfinite(jr).all() and np.abs(jr).max() > 0   # (the hinge's axis: the results were written)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_fd_points_of_changing_size(models, name, dtype):
    """``transition_fd_points`` with T = 1, 3, 1 on one object: each result is bitwise that of a fresh object, and ``transition_fd``
    afterwards is what a fresh object gives."""
    import torch

    cm, dm = models(name)
    tdt = torch.float32 if dtype == "float32" else torch.float64
    one = BatchSim(dm, B3, dtype=dtype, specialize=False)
    _scatter(one, cm, 2)
    rng = np.random.default_rng(3)
    for T in (1, 3, 1):
        q = torch.from_numpy(np.asarray(cm.qpos0) + rng.normal(size=(T, B3, cm.nq)) * 0.1).to(device="cuda", dtype=tdt)
        v = torch.from_numpy(rng.normal(size=(T, B3, cm.nv)) * 0.3).to(device="cuda", dtype=tdt)
        u = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(T, B3, cm.nu))).to(device="cuda", dtype=tdt)
        fresh = BatchSim(dm, B3, dtype=dtype, specialize=False)
        _scatter(fresh, cm, 2)
        A, Bm = one.transition_fd_points(q, v, u)
        Af, Bf = fresh.transition_fd_points(q, v, u)
        torch.cuda.synchronize()
        assert tuple(A.shape) == (T, B3, 2 * cm.nv, 2 * cm.nv) and tuple(Bm.shape) == (T, B3, 2 * cm.nv, cm.nu)
        assert torch.equal(A, Af) and torch.equal(Bm, Bf), T
        assert bool(torch.isfinite(A).all()) and float(A.abs().max()) > 0
    fresh = BatchSim(dm, B3, dtype=dtype, specialize=False)
    _scatter(fresh, cm, 2)
    A1, B1 = one.transition_fd()
    A2, B2 = fresh.transition_fd()
    assert np.array_equal(A1, A2) and np.array_equal(B1, B2)
    A1b, B1b = one.transition_fd()                             # and the result blocks are reused unchanged
    assert np.array_equal(A1, A1b) and np.array_equal(B1, B1b)


@pytest.mark.parametrize("batch", [B3, 200])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_host_arrays_of_alternating_size(models, name, dtype, batch):
    """``set`` / ``get`` and ``set_env_params`` from host memory with sizes that alternate (at batch 200: across the 4096-byte floor of
    the pinned staging block, in both directions): what is read back equals what was sent."""
    cm, dm = models(name)
    sim = BatchSim(dm, batch, dtype=dtype, specialize=False)
    rng = np.random.default_rng(4)
    esize = 4 if dtype == "float32" else 8
    sent = []
    for arr in ("qvel", "xpos", "qpos", "xquat", "time", "xpos"):
        n = sim.array_ptr(arr)[1]
        x = rng.normal(size=(batch, n)).astype(np.float32).astype(np.float64)
        sim.set(arr, x)
        assert np.array_equal(sim.get(arr), x), arr
        sent.append(batch * n * (8 if arr == "time" else esize))
    params = ("dof_damping", "body_inertia", "dof_damping", "gravity", "dof_armature", "body_inertia")
    for k, field in enumerate(params):
        shape = tuple(sim.env_params(field).shape[1:])
        x = rng.uniform(0.5, 1.5, size=(batch, *shape))
        if k % 2:
            x = x.astype(np.float32).astype(np.float64)
        sim.set_env_params(**{field: x})
        assert np.array_equal(sim.env_params(field), x), field
        sent.append(batch * int(np.prod(shape)) * 8)
    sim.clear_env_params()
    assert sim.env_param_mask() == 0
    if batch == 200:                                            # the sizes sent lie on both sides of the floor, and alternate across it
        side = [s >= 4096 for s in sent]
        assert sum(a != b for a, b in zip(side, side[1:])) >= 6, sent
    else:
        assert len(set(sent)) > 2 and max(sent) < 4096, sent


def test_life_cycle_of_every_lazy_block(models, monkeypatch):
    """Twenty times: create a data object, touch every lazily made block (host mirror and its shadow, FD result blocks and scratch,
    Jacobian buffers, parameter rows and their stage, feedback gains / noise / scratch, an observation spec with ids, the debug arrays,
    the hand-over buffer of the ticket map), and drop it.  Every call succeeds and the device is healthy afterwards."""
    import gc

    import torch

    monkeypatch.setenv("MJB_CHUNK_STEPS", "4")                 # the ticket map (float32) at this small batch
    rng = np.random.default_rng(6)
    for it in range(20):
        name, dtype = NAMES[it % 2], DTYPES[(it // 2) % 2]
        cm, dm = models(name)
        tdt = torch.float32 if dtype == "float32" else torch.float64
        sim = BatchSim(dm, B3, dtype=dtype, specialize=False)
        q, v, u = _scatter(sim, cm, 7)
        view = sim.host_view("qpos")
        sim.sync_to_host()
        assert np.array_equal(view, q)
        sim.step_host_auto(1)
        A, Bm = sim.transition_fd()
        assert np.isfinite(A).all() and np.isfinite(Bm).all()
        pts = [torch.from_numpy(x).to(device="cuda", dtype=tdt) for x in (q, v, u)]
        Ap, _ = sim.transition_fd_points(*pts)
        assert bool(torch.isfinite(Ap).all())
        jp, _ = sim.jac([1, 0], [cm.nbody - 1, 0])
        assert np.isfinite(jp).all()
        sim.set_env_params(dof_damping=rng.uniform(0.5, 1.5, size=(B3, cm.nv)), body_mass=rng.uniform(0.5, 1.5, size=(B3, cm.nbody)))
        sim.step(2)
        sim.clear_env_params()
        sim.set_feedback(rng.normal(size=(cm.nu, 2 * cm.nv)) * 0.1, np.zeros(cm.nu), np.asarray(cm.qpos0, dtype=np.float64))
        sim.set_feedback_noise(np.full(cm.nu, 0.01), rng.normal(size=(5, cm.nu)), 1)
        sim.feedback_ctrl(3)
        spec = sim.make_obs_spec(1 | 2 | 16, site_ids=[0], body_ids=[cm.nbody - 1], geom_ids=[0], subtree_ids=[0])
        obs = torch.zeros((B3, spec.dim), dtype=tdt, device="cuda")
        sim.obs_gather(spec, obs.data_ptr())
        sim.debug_forward()
        assert np.isfinite(sim.debug_get("qM")).all()
        sim.rollout(40, CTRL_RANDOM, seed=it, ctrl_scale=0.01)
        sim.sync()
        assert sim.schedule_info()["map"] == ("tickets" if dtype == "float32" else "static")
        assert sim.engine_flags() == 0
        assert np.isfinite(sim.get("qpos")).all() and bool(torch.isfinite(obs).all())
        del spec, view, sim
        gc.collect()
    torch.cuda.synchronize()
