"""The reference's unit/integration assertions (reference tests/test_mujoco_template.py:74-588: shapes,
key sets, identity / shares_memory, call counts, ordering) re-targeted at the batched ``Env``, plus
the batched fast paths (fused rollout, device observation gather).  Needs a GPU (no CPU fallback)."""
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mujoco_template_amd as mt  # noqa: E402
from mujoco_template_amd import mj  # noqa: E402
from mujoco_template_amd import runtime  # noqa: E402
from tests.conftest import BASE_XML, MODELS, measured  # noqa: E402

# fp32 tolerances of the parity-type checks in this file: <= 3x the error measured on an MI355X (gpurun_out/parity_measured.json)
API_TOL32 = {"gemm": {"humanoid": 7e-7, "drone2": 2.7e-7, "cartpole": 7.5e-8}, "gemm_fused": {"humanoid": 7.1e-7, "drone2": 5.4e-7, "cartpole": 8.8e-8},
             "lqr_1000_pair": 2.8e-5, "lqr_1000_oracle": 2.0e-5, "pid_300_oracle": 9.0e-7, "pid_300_pair": 2.5e-6}


@pytest.fixture
def handle():
    h = mt.ModelHandle.from_xml_string(BASE_XML)
    h.forward()
    return h


def test_model_handle_wraps_existing_data():
    model = mj.MjModel.from_xml_string(BASE_XML)
    data = mj.MjData(model)
    data.qpos[0] = 0.25
    h = mt.ModelHandle.from_model_and_data(model, data)
    assert h.model is model and h.data is data
    env = mt.Env(h, obs_spec=mt.ObservationSpec(include_qpos=True))
    assert env.data is data
    env.reset()
    assert env.data is data


def test_model_handle_rejects_mismatched_data():
    a, b = mj.MjModel.from_xml_string(BASE_XML), mj.MjModel.from_xml_string(BASE_XML)
    with pytest.raises(mt.ConfigError):
        mt.ModelHandle(a, data=mj.MjData(b))


def test_host_edits_reach_the_device(handle):
    handle.data.qpos[0] = 0.005                  # in-place edit of the mirror, as reference controllers do in prepare()
    handle.forward()
    assert handle.data.site_xpos[0] == pytest.approx([0, 0, 0.2])
    assert handle.data.sensordata[0] == pytest.approx(0.005, abs=1e-7)   # jointpos sensor follows the edit
    handle.data.qvel[:] = 1.0
    handle.step()
    assert handle.data.qpos[0] == pytest.approx(0.005 + 0.005 * 1.0, abs=2e-4)   # inside the +-1 degree range: free motion


def test_env_step_can_skip_observation_and_hooks(handle):
    calls = {"extract": 0, "reward": 0, "done": 0, "info": 0}
    seen = []

    def reward_fn(model, data, obs):
        calls["reward"] += 1; seen.append(obs); return 0.0

    def done_fn(model, data, obs):
        calls["done"] += 1; seen.append(obs); return False

    def info_fn(model, data, obs):
        calls["info"] += 1; seen.append(obs); return {"value": float(data.time)}

    env = mt.Env(handle, obs_spec=mt.ObservationSpec(include_qpos=True), reward_fn=reward_fn, done_fn=done_fn, info_fn=info_fn)
    original = env.extractor

    def counting(data):
        calls["extract"] += 1
        return original(data)

    env.extractor = counting
    env.reset()
    for k in calls:
        calls[k] = 0
    seen.clear()
    result = env.step(return_obs=False)
    assert calls == {"extract": 0, "reward": 1, "done": 1, "info": 1}
    assert seen == [None, None, None]
    assert result.obs is None and result.reward == 0.0 and result.done is False
    assert result.info == {"value": pytest.approx(float(env.data.time))}


def test_iterate_passive_respects_return_obs_flag(handle):
    env = mt.Env(handle, obs_spec=mt.ObservationSpec(include_qpos=True))
    original, n = env.extractor, [0]

    def counting(data):
        n[0] += 1
        return original(data)

    env.extractor = counting
    env.reset()
    n[0] = 0
    results = list(runtime.iterate_passive(env, max_steps=2, return_obs=False))
    assert n[0] == 0 and all(r.obs is None for r in results)


def test_observation_extractor_dict_and_array(handle):
    spec = dict(include_qpos=True, include_qvel=True, include_act=True, include_ctrl=True, include_sensordata=True, include_time=True,
                sites_pos=("tip",), bodies_pos=("torso",), geoms_pos=("torso_geom",), subtree_com=("torso",))
    ex = mt.ObservationExtractor(handle.model, mt.ObservationSpec(as_dict=True, **spec))
    obs = ex(handle.data)
    assert set(obs) == {"qpos", "qvel", "act", "ctrl", "sensordata", "time", "sites_pos", "bodies_pos", "geoms_pos", "subtree_com"}
    m = handle.model
    assert obs["qpos"].shape == (m.nq,) and obs["qvel"].shape == (m.nv,) and obs["ctrl"].shape == (m.nu,)
    assert obs["sensordata"].shape == (m.nsensordata,) and obs["time"].shape == (1,)
    assert obs["sites_pos"].shape == (1, 3) and obs["bodies_pos"].shape == (1, 3) and obs["geoms_pos"].shape == (1, 3)
    flat = mt.ObservationExtractor(m, mt.ObservationSpec(as_dict=False, **spec))(handle.data)
    assert flat.shape == (m.nq + m.nv + m.nu + m.nsensordata + 1 + 3 + 3 + 3 + 3,)
    # device gather kernel produces the same flat layout (sorted keys)
    dev = mt.ObservationExtractor(m, mt.ObservationSpec(as_dict=False, **{**spec, "include_act": False})).gather_device(handle.data)
    assert dev.shape == (1, flat.size) and dev.cpu().numpy()[0] == pytest.approx(flat, abs=1e-6)


def test_observation_extractor_zero_copy_flag(handle):
    obs = mt.ObservationExtractor(handle.model, mt.ObservationSpec(copy=False))(handle.data)
    assert np.shares_memory(obs["qpos"], handle.data.qpos) and np.shares_memory(obs["qvel"], handle.data.qvel)
    obs = mt.ObservationExtractor(handle.model, mt.ObservationSpec(copy=True))(handle.data)
    assert not np.shares_memory(obs["qpos"], handle.data.qpos)


def test_observation_extractor_custom_extras(handle):
    spec = mt.ObservationSpec(include_qpos=False, include_qvel=False,
                              extras={"twice": lambda m, d: 2 * np.array(d.qpos), "prod": mt.ObservationProducer(lambda m, d: [1.0, 2.0], copy=True)})
    obs = mt.ObservationExtractor(handle.model, spec)(handle.data)
    assert set(obs) == {"twice", "prod"} and obs["prod"].tolist() == [1.0, 2.0]
    with pytest.raises(ValueError):
        mt.ObservationExtractor(handle.model, mt.ObservationSpec(extras={"qpos": lambda m, d: [0.0]}))(handle.data)
    with pytest.raises(TypeError):
        mt.ObservationExtractor(handle.model, mt.ObservationSpec(extras={"bad": 3}))


def test_observation_extractor_missing_sensors_warns_once():
    h = mt.ModelHandle.from_xml_path(MODELS["cartpole"])
    ex = mt.ObservationExtractor(h.model, mt.ObservationSpec(include_sensordata=True))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = ex(h.data); ex(h.data)
    assert a["sensordata"].shape == (0,)
    assert len([x for x in w if issubclass(x.category, RuntimeWarning)]) == 1


def test_model_handle_actuator_group_mask(handle):
    handle.set_enabled_actuator_groups([1])
    assert int(handle.model.opt.disableactuator) == 1 << 0
    assert handle.enabled_actuator_mask().tolist() == [False, True]
    # the disabled torque motor produces no force on the device
    handle.data.ctrl[:] = [5.0, 0.0]
    handle.forward()
    assert abs(handle.data.qacc[0]) < 1e-6
    with pytest.raises(mt.CompatibilityError):
        handle.set_enabled_actuator_groups([])
    with pytest.raises(mt.ConfigError):
        handle.set_enabled_actuator_groups([40])
    with pytest.raises(mt.CompatibilityError):
        handle.set_enabled_actuator_groups([7])


def test_linearize_discrete_native_and_fd(handle):
    for native in (True, False):
        A, B = mt.linearize_discrete(handle.model, handle.data, use_native=native)
        assert A.shape == (2, 2) and B.shape == (2, 2)
        assert np.isfinite(A).all() and np.isfinite(B).all()
    A1, B1 = mt.linearize_discrete(handle.model, handle.data, use_native=True)
    A2, B2 = mt.linearize_discrete(handle.model, handle.data, use_native=False)
    assert A1 == pytest.approx(A2, abs=1e-4) and B1 == pytest.approx(B2, abs=1e-4)      # both use the native sign convention


def test_compute_requested_jacobians_returns_expected_blocks(handle):
    jac = mt.compute_requested_jacobians(handle.model, handle.data, ["site:tip", "body:torso", "bodycom:torso", "subtreecom:torso"])
    nv = handle.model.nv
    assert set(jac) == {"site:tip", "body:torso", "bodycom:torso", "subtreecom:torso"}
    assert jac["site:tip"]["jacp"].shape == (3, nv) and jac["site:tip"]["jacr"].shape == (3, nv)
    assert set(jac["bodycom:torso"]) == {"jacp"} and set(jac["subtreecom:torso"]) == {"jacp"}
    assert jac["site:tip"]["jacr"][:, 0] == pytest.approx([0, 0, 1])          # hinge about z
    with pytest.raises(mt.ConfigError):
        mt.compute_requested_jacobians(handle.model, handle.data, ["com"])
    with pytest.raises(mt.NameLookupError):
        mt.compute_requested_jacobians(handle.model, handle.data, ["site:nope"])


class _Ctl:
    def __init__(self, caps):
        self.capabilities = caps
        self.prepared = 0
        self.calls = []

    def prepare(self, model, data):
        self.prepared += 1

    def __call__(self, model, data, t):
        self.calls.append((t, float(data.qpos[0])))
        data.ctrl[:] = [0.5, 0.1]


def test_env_step_invokes_controller_and_produces_precomputes(handle):
    caps = mt.ControllerCapabilities(control_space=mt.ControlSpace.TORQUE, needs_linearization=True,
                                     needs_jacobians=("site:tip", "bodycom:torso"), actuator_groups=(0,))
    ctl = _Ctl(caps)
    with pytest.warns(RuntimeWarning):
        env = mt.Env(handle, obs_spec=mt.ObservationSpec(include_ctrl=True), controller=ctl, control_decimation=2,
                     info_fn=lambda m, d, o: {"extra_metric": 1.0})
    env.reset()
    assert ctl.prepared == 2                                      # __init__ and reset (reference tests:452-454)
    r1 = env.step()
    assert len(ctl.calls) == 1 and ctl.calls[0][0] == pytest.approx(0.0)
    assert r1.info["A"].shape == (2, 2) and r1.info["B"].shape == (2, 2)
    assert set(r1.info["jacobians"]) == {"site:tip", "bodycom:torso"}
    assert "compat_warnings" in r1.info and r1.info["extra_metric"] == 1.0
    assert r1.obs["ctrl"] == pytest.approx([0.5, 0.1], abs=1e-6)
    r2 = env.step()
    assert len(ctl.calls) == 1                                    # decimation 2: no controller call on the odd substep
    assert "A" not in r2.info and "compat_warnings" not in r2.info
    env.step()
    assert len(ctl.calls) == 2 and ctl.calls[1][0] == pytest.approx(2 * 0.005)
    env2 = mt.Env(handle, info_fn=lambda m, d, o: {"compat_warnings": 1}, controller=_Ctl(mt.ControllerCapabilities()))
    with pytest.raises(mt.TemplateError):
        env2.step()


def test_env_step_accumulates_substep_instrumentation(handle):
    caps = mt.ControllerCapabilities(needs_linearization=True, needs_jacobians=("site:tip",))
    env = mt.Env(handle, controller=_Ctl(caps))
    env.reset()
    r = env.step(3)
    assert isinstance(r.info["A"], list) and len(r.info["A"]) == 3 and len(r.info["B"]) == 3 and len(r.info["jacobians"]) == 3
    with pytest.raises(mt.ConfigError):
        env.step(0)
    with pytest.raises(mt.ConfigError):
        mt.Env(handle, control_decimation=0)


def test_env_from_xml_path_auto_resets_and_pendulum_config1():
    """BASELINE config 1: examples/pendulum, ZeroController, Env.passive 200 steps, batch 1."""
    env = mt.Env.from_xml_path(MODELS["pendulum"], controller=mt.ZeroController())
    assert env.data.time == pytest.approx(0.0)
    env.data.qpos[0] = np.pi / 2                                   # released from 90 degrees (pendulum_passive_config.py:58)
    results = list(env.passive(max_steps=200))
    assert len(results) == 200 and all(isinstance(r, mt.StepResult) for r in results)
    assert env.data.time == pytest.approx(200 * 0.005)
    assert set(results[-1].obs) == {"qpos", "qvel"}
    m, I, L = 0.7941946228, 0.06809102997, 0.25
    energy = 0.5 * I * env.data.qvel[0] ** 2 - m * 9.81 * L * np.cos(env.data.qpos[0])
    assert energy == pytest.approx(0.0, abs=2e-4)                  # RK4 in fp32: energy of the 90-degree release is conserved
    with pytest.raises(mt.ConfigError):
        mt.Env.from_xml_path(MODELS["pendulum"], auto_reset=False, keyframe=0)
    with pytest.raises(mt.ConfigError):
        list(env.passive(max_steps=0))
    with pytest.raises(mt.ConfigError):
        list(env.passive(duration=-1.0))


def test_env_passive_duration_and_keyframes():
    env = mt.Env.from_xml_path(MODELS["drone2"], keyframe="hover")
    assert env.data.qpos == pytest.approx([0, 0, 0.3, 1, 0, 0, 0]) and env.data.ctrl == pytest.approx([3.2495625] * 4)
    n = runtime.run_passive_headless(env, duration=0.1)
    # ten steps of 0.01 accumulate to 0.09999999999999999 < 0.1 in float64 (MuJoCo's `time += timestep` does the same), so the
    # reference's stop test `data.time >= duration` (runtime.py:658-663) lets an ELEVENTH step through; fused and per-step paths agree
    assert n == 11 and env.data.time == pytest.approx(0.11)
    again = mt.Env.from_xml_path(MODELS["drone2"], keyframe="hover")
    assert runtime.run_passive_headless(again, duration=0.1, hooks=lambda r: None) == 11
    assert env.data.qpos == pytest.approx([0, 0, 0.3, 1, 0, 0, 0], abs=1e-5)    # hover is a fixed point (K1)
    with pytest.raises(mt.NameLookupError):
        env.reset("nope")
    with pytest.raises(mt.ConfigError):
        env.reset(5)


def test_batched_env_fused_rollout_matches_stepwise():
    """The fused K-step kernel launch and the per-step Env.step loop produce identical states (same RNG stream)."""
    kw = dict(obs_spec=mt.ObservationSpec(as_dict=False, sites_pos=("imu", "thrust1"), bodies_pos=("x2",)), batch=64)
    a = mt.Env.from_xml_path(MODELS["drone2"], controller=mt.RandomCtrlController(seed=2, scale=0.3), **kw)
    b = mt.Env.from_xml_path(MODELS["drone2"], controller=mt.RandomCtrlController(seed=2, scale=0.3), **kw)
    obs_ring = a.rollout(20, obs_every=1)                                         # [20, 64, dim] on the GPU
    last = None
    for _ in range(20):
        last = b.step()
    assert np.array_equal(np.array(a.data.qpos), np.array(b.data.qpos))
    assert obs_ring.shape == (20, 64, 3 + 7 + 6 + 6)
    assert obs_ring[-1].cpu().numpy() == pytest.approx(last.obs, abs=1e-6)        # bodies_pos | qpos | qvel | sites_pos
    assert runtime.run_passive_headless(a, max_steps=30) == 30 and a.data.time[0] == pytest.approx(0.5)
    # host RandomCtrlController.__call__ writes exactly the device's ctrl
    c = mt.Env.from_xml_path(MODELS["drone2"], batch=4)
    ctl = mt.RandomCtrlController(seed=2, scale=0.3)
    ctl.prepare(c.model, c.data)
    ctl(c.model, c.data, 0.0)
    d = mt.Env.from_xml_path(MODELS["drone2"], controller=mt.RandomCtrlController(seed=2, scale=0.3), batch=4)
    d.rollout(1)
    assert np.array(d.data.ctrl) == pytest.approx(np.array(c.data.ctrl), abs=1e-6)


def test_batched_env_shapes_and_linearization():
    """BASELINE config 4 shape contract: cartpole needs_linearization, batch 512 -> A [512,4,4], B [512,4,1]."""
    class Lin(_Ctl):
        def __call__(self, model, data, t):
            data.ctrl[...] = 0.0

    env = mt.Env.from_xml_path(MODELS["cartpole"], controller=Lin(mt.ControllerCapabilities(needs_linearization=True)), batch=512)
    r = env.step()
    assert r.info["A"].shape == (512, 4, 4) and r.info["B"].shape == (512, 4, 1)
    assert r.obs["qpos"].shape == (512, 2)
    assert np.allclose(r.info["A"][0], r.info["A"][511])          # identical replicas -> identical linearisation


def test_linear_feedback_controller_fused_equals_host_loop():
    """LinearFeedbackController: the fused device evaluation and the per-step host __call__ drive the same trajectory."""
    rng = np.random.default_rng(2)
    probe = mt.Env.from_xml_path(MODELS["drone2"], keyframe="hover", batch=2)
    nu, nv = probe.model.nu, probe.model.nv
    K = rng.normal(size=(nu, 2 * nv)) * 0.3
    q_goal, u_goal = np.array(probe.data.qpos[0]), np.array(probe.data.ctrl[0])

    class HostOnly:                                    # same law, but without device_ctrl_mode: forces the reference-style loop
        def __init__(self, inner):
            self.inner, self.capabilities = inner, inner.capabilities
        def prepare(self, model, data):
            self.inner.prepare(model, data)
        def __call__(self, model, data, t):
            self.inner(model, data, t)

    def make(ctl):
        env = mt.Env.from_xml_path(MODELS["drone2"], controller=ctl, keyframe="hover", batch=8, dtype="float64")
        env.data.qpos[:, 2] += np.linspace(0.0, 0.07, 8)     # different height offsets -> different feedback
        return env

    a = make(mt.LinearFeedbackController(K=K, ctrl0=u_goal, qpos_goal=q_goal))
    b = make(HostOnly(mt.LinearFeedbackController(K=K, ctrl0=u_goal, qpos_goal=q_goal)))
    assert a.can_fuse() and not b.can_fuse()
    a.rollout(40)
    for _ in range(40):
        b.step(return_obs=False)
    assert np.abs(np.array(a.data.qpos) - np.array(b.data.qpos)).max() < 1e-9
    assert np.abs(np.array(a.data.ctrl) - np.array(b.data.ctrl)).max() < 1e-9


def test_steady_ctrl0_drone_hover_and_errors():
    """reference setpoints.steady_ctrl0 (setpoints.py:10-58): the drone's hover keyframe needs ctrl 3.2495625 per rotor
    (x2.xml:90: 1.325 kg * 9.81 / 4); argument checks and the nu == 0 error keep the reference's exception types."""
    h = mt.ModelHandle.from_xml_path(MODELS["drone2"], dtype="float64")
    m, d = h.model, h.data
    key_qpos = np.array(m.compiled.arrays["key_qpos"]).reshape(-1, m.nq)[0]
    before = (np.array(d.qpos), np.array(d.qvel), float(d.time))
    u = mt.steady_ctrl0(m, d, key_qpos)
    assert u.shape == (m.nu,) and u == pytest.approx([3.2495625] * 4, abs=1e-8)
    assert np.array_equal(np.array(d.qpos), before[0]) and np.array_equal(np.array(d.qvel), before[1]) and float(d.time) == before[2]
    with pytest.raises(mt.ConfigError):
        mt.steady_ctrl0(m, d, np.zeros(m.nq + 1))
    with pytest.raises(mt.ConfigError):
        mt.steady_ctrl0(m, d, key_qpos, np.zeros(m.nv + 2))
    # the reference's own densification code path runs unchanged against the CSR views
    mj.mj_resetDataKeyframe(m, d, 0); mj.mj_forward(m, d); d.qacc[:] = 0.0; mj.mj_inverse(m, d)
    M = np.zeros((m.nu, m.nv))
    mj.mju_sparse2dense(M, np.reshape(d.actuator_moment, (-1,)), d.moment_rownnz, d.moment_rowadr, np.reshape(d.moment_colind, (-1,)))
    assert (np.atleast_2d(np.array(d.qfrc_inverse)) @ np.linalg.pinv(M)).ravel() == pytest.approx([3.2495625] * 4, abs=1e-8)
    # batched, fp32: one set-point for all environments -> [batch, nu]
    hb = mt.ModelHandle.from_xml_path(MODELS["drone2"], batch=3)
    ub = mt.steady_ctrl0(hb.model, hb.data, key_qpos)
    assert ub.shape == (3, m.nu) and np.abs(ub - 3.2495625).max() < 1e-4
    nu0 = mt.ModelHandle.from_xml_string("<mujoco><worldbody><body><joint type='hinge'/><geom size='0.1'/></body></worldbody></mujoco>")
    with pytest.raises(mt.CompatibilityError):
        mt.steady_ctrl0(nu0.model, nu0.data, np.zeros(1))


def test_state_control_recorder_hook_and_bulk_feeds(tmp_path):
    """reference logging.StateControlRecorder (logging.py:31-247): the StepHook feed and the batched device-ring feed
    log identical rows; the CSV on disk parses back to them; probe validation keeps the reference's errors."""
    import csv

    from mujoco_template_amd.logging import DataProbe, StateControlRecorder

    def make():
        return mt.Env.from_xml_path(MODELS["cartpole"], controller=mt.RandomCtrlController(seed=3, scale=0.01), batch=4)

    env = make()
    probe = DataProbe("pole_angle", lambda e, r: np.asarray(e.data.qpos)[2, 1])
    path = tmp_path / "hook.csv"
    with StateControlRecorder(env, log_path=path, probes=[probe], env_index=2) as rec:
        n = runtime.run_passive_headless(env, max_steps=12, hooks=rec)
    assert n == 12 and len(rec.rows) == 12
    assert rec.columns == ("time_s", "qpos[slider]", "qvel[slider]", "qpos[hinge]", "qvel[hinge]", "ctrl[cart_force]", "pole_angle")
    assert rec.rows[-1][0] == pytest.approx(12 * 0.01)
    assert rec.rows[3][6] == rec.rows[3][2]      # reference row order: time, ALL qpos, ALL qvel, ctrl (logging.py:207-224)
    with open(path, newline="") as f:
        disk = list(csv.reader(f))
    assert tuple(disk[0]) == rec.columns and len(disk) == 13 and float(disk[5][1]) == rec.rows[4][1]
    # bulk feed on a fresh, identically seeded environment: same rows (no probes there)
    env2 = make()
    rec2 = StateControlRecorder(env2, env_index=2)
    assert rec2.record_rollout(12, chunk=5) == 12
    for a, b in zip(rec.rows, rec2.rows):
        assert a[1:6] == pytest.approx(b[1:], rel=0, abs=0)
        assert a[0] == pytest.approx(b[0], abs=1e-6)            # the device ring holds time in the data dtype (fp32)
    # all environments: leading env column
    env3 = make()
    rec3 = StateControlRecorder(env3, env_index=None)
    rec3.record_rollout(3)
    assert rec3.columns[0] == "env" and len(rec3.rows) == 12 and [r[0] for r in rec3.rows[:4]] == [0, 1, 2, 3]
    assert rec3.rows[2][1:] == pytest.approx(rec2.rows[0], abs=0)
    assert next(rec3.as_dicts())["time_s"] == pytest.approx(0.01)
    env4 = make()
    rec4 = StateControlRecorder(env4, env_index=2, align_columns=True)
    rec4.record_rollout(2)
    assert (rec4.rows[1][1], rec4.rows[1][3], rec4.rows[1][2], rec4.rows[1][4]) == tuple(rec2.rows[1][1:5])
    with pytest.raises(mt.ConfigError):
        StateControlRecorder(env, probes=[probe, probe])
    with pytest.raises(mt.ConfigError):
        StateControlRecorder(env, probes=[DataProbe("", lambda e, r: 0.0)])
    with pytest.raises(mt.ConfigError):
        StateControlRecorder(env, env_index=7)
    with pytest.raises(mt.ConfigError):
        StateControlRecorder(env, probes=[probe]).record_rollout(2)
    bad = StateControlRecorder(env, probes=[DataProbe("vec", lambda e, r: np.zeros(2))])
    with pytest.raises(mt.ConfigError):
        bad(env.step())


def test_host_mirror_is_one_pinned_block_and_steps_match_the_device_path():
    """mjb_host_view / mjb_step_host (VERDICT r1 "finish the boundary"): data.qpos & co are numpy views over the library's pinned
    float64 block (stable objects, obs copy=False aliases them), in-place edits travel as one packed upload, and the
    host-driven step gives exactly the state the plain device path (mjb_set_array + mjb_step) gives."""
    from mujoco_template_amd._capi import BatchSim

    B = 6
    h = mt.ModelHandle.from_xml_path(MODELS["humanoid"], batch=B, dtype="float32")
    d = h.data
    q_view, v_view, u_view = d.qpos, d.qvel, d.ctrl
    assert q_view is d.qpos and np.shares_memory(q_view, d.sim.host_view("qpos"))        # the same pinned memory every time
    span = [d.sim.host_view(n) for n in ("qpos", "qvel", "ctrl", "qacc", "qacc_warmstart", "time")]
    for a, b in zip(span[:-1], span[1:]):                                                  # contiguous fields of ONE block
        assert a.ctypes.data + a.nbytes == b.ctypes.data
    rng = np.random.default_rng(0)
    ref = BatchSim(h.model._device_model(), B, dtype="float32")
    for s in range(5):
        u = rng.uniform(-1, 1, size=(B, h.model.nu))
        d.ctrl[:] = u                                                                      # in-place edit, as reference controllers do
        if s == 2:
            d.qvel[:, 0] += 0.25
            ref.set("qvel", d.qvel)
        ref.set("ctrl", u)
        h.step()
        ref.step(1)
        assert d.qpos is q_view and d.qvel is v_view and d.ctrl is u_view
        assert np.array_equal(d.qpos, ref.get("qpos")) and np.array_equal(d.qvel, ref.get("qvel"))
        assert np.array_equal(d.qacc_warmstart, ref.get("qacc_warmstart"))
        assert d.time == pytest.approx((s + 1) * h.model.opt.timestep)
    d.time = 0.5
    h.step()
    assert d.time == pytest.approx(0.5 + h.model.opt.timestep)
    assert d.sim.get("time")[:, 0] == pytest.approx(0.5 + h.model.opt.timestep)
    assert d.engine_warnings == []
    # edit detection lives in the library (mjb_mirror_edited_mask / mjb_mirror_commit / mjb_step_host_auto): bitwise comparison of the
    # pinned block with its shadow, per field, bit order of MIRROR_FIELDS
    sim = d.sim
    assert sim.mirror_edited_mask() == 0
    d.ctrl[2, 3] += 0.125
    assert sim.mirror_edited_mask() == 4
    d.qpos[0, 2] += 1e-9
    d.qacc_warmstart[1, 0] = 7.0
    assert sim.mirror_edited_mask() == 1 | 4 | 16
    sim.mirror_commit(1)
    assert sim.mirror_edited_mask() == 4 | 16
    assert sim.step_host_auto(1) == 4 | 16 and sim.mirror_edited_mask() == 0             # uploaded what differed, shadow refreshed
    assert sim.get("ctrl")[2, 3] == np.float32(d.ctrl[2, 3])
    assert sim.step_host_auto(0, compare=False) == 0                                       # mj_forward, nothing compared
    # the small-batch path returns on the environments' completion words (polled), the large one on the stream: same results
    big = mt.ModelHandle.from_xml_path(MODELS["humanoid"], batch=80, dtype="float32")      # block > 64 KB: staged copies, no polling
    big.data.ctrl[:] = np.tile(u, (14, 1))[:80]
    d.ctrl[:] = u
    d.qpos[:] = big.data.qpos[:B]; d.qvel[:] = big.data.qvel[:B]; d.qacc_warmstart[:] = big.data.qacc_warmstart[:B]; d.qacc[:] = big.data.qacc[:B]; d.time = 0.0; big.data.time = 0.0
    for _ in range(3):
        h.step(); big.step()
    assert np.array_equal(d.qpos, big.data.qpos[:B]) and np.array_equal(d.qvel, big.data.qvel[:B])


def test_truncated_physics_is_surfaced_once():
    """contacts / rows beyond the LDS caps are dropped AND reported: one RuntimeWarning, data.engine_warnings,
    info['engine_warnings'] of the first Env.step after it was seen."""
    with pytest.warns(RuntimeWarning, match="beyond the per-environment caps"):
        env = mt.Env.from_xml_path(MODELS["humanoid"], batch=4, dtype="float32", nconmax=1, nefcmax=8, controller=None)
        infos = [env.step(return_obs=False).info for _ in range(12)]                       # the standing humanoid has 4+ foot contacts
    seen = [i for i in infos if "engine_warnings" in i]
    assert len(seen) == 1 and "nconmax=1" in seen[0]["engine_warnings"][0]               # reported once
    assert env.data.counters()["con_dropped"].sum() > 0 and len(env.data.engine_warnings) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert "engine_warnings" not in env.step(return_obs=False).info
        full = mt.Env.from_xml_path(MODELS["humanoid"], batch=4, dtype="float32")
        for _ in range(30):
            assert "engine_warnings" not in full.step(return_obs=False).info
        assert full.data.engine_warnings == []


def test_binary_model_steps_like_the_xml_model(tmp_path):
    a = mt.ModelHandle.from_xml_path(MODELS["drone2"], batch=3, dtype="float64")
    path = str(tmp_path / "m.mjbm")
    a.save_binary(path)
    b = mt.ModelHandle.from_binary_path(path, batch=3, dtype="float64")
    for h in (a, b):
        h.reset_keyframe("hover")
        h.data.ctrl[:] = 4.0
        h.step(20)
    assert np.array_equal(a.data.qpos, b.data.qpos) and np.array_equal(a.data.qvel, b.data.qvel)


def test_fd_fallback_is_float64_batched_and_matches_native_away_from_zero():
    """the Python FD fallback used to nudge the fp32 device state by eps = 1e-6 (8 ulps of an O(1) state) and refused
    batches.  Now: a float64 twin, all replicas in one launch, any batch, horizon_steps; at a NON-ZERO state it agrees with the
    native mjd_transitionFD to 1e-4 relative, and a 3-step horizon equals the chain of three one-step linearisations."""
    rng = np.random.default_rng(4)
    for name, B in (("cartpole", 3), ("drone2", 2)):
        h = mt.ModelHandle.from_xml_path(MODELS[name], batch=B, dtype="float32")
        m, d = h.model, h.data
        q = np.array(d.qpos)
        if name == "cartpole":
            q[:] = rng.uniform(-0.4, 0.4, size=q.shape)
        else:
            q[:, 2] += 0.5 + rng.uniform(0, 0.2, size=B)                         # airborne: smooth dynamics
        d.qpos[:] = q
        d.qvel[:] = rng.normal(size=d.qvel.shape) * 0.3
        if name == "drone2":
            # the fallback measures dq' at the BASE state (the reference's _dqpos(after, base)), mjd_transitionFD at the NEXT state:
            # for a free body spinning at w the rotation blocks differ by the antisymmetric 1/2 [w h]x; compare without spin
            d.qvel[:, 3:6] = 0.0
        d.ctrl[:] = 3.2495625 if name == "drone2" else rng.uniform(-20, 20, size=d.ctrl.shape)   # hover thrust: no angular acceleration
        h.forward()
        before = np.array(d.qpos), np.array(d.qvel)
        A1, B1 = mt.linearize_discrete(m, d, use_native=True)
        A2, B2 = mt.linearize_discrete(m, d, use_native=False)
        assert A2.shape == (B, 2 * m.nv, 2 * m.nv) and B2.shape == (B, 2 * m.nv, m.nu)
        assert np.abs(A1 - A2).max() <= 1e-4 * max(1.0, np.abs(A1).max()) and np.abs(B1 - B2).max() <= 1e-4 * max(1.0, np.abs(B1).max())
        assert np.array_equal(d.qpos, before[0]) and np.array_equal(d.qvel, before[1])       # data untouched
        # horizon: d x_3 / d x_0 = A(x_2) A(x_1) A(x_0) along the trajectory (float64 data so that the chain is exact to FD error)
        h64 = mt.ModelHandle.from_xml_path(MODELS[name], batch=B, dtype="float64")
        h64.data.qpos[:] = before[0]; h64.data.qvel[:] = before[1]; h64.data.ctrl[:] = d.ctrl
        h64.forward()
        A3, _ = mt.linearize_discrete(h64.model, h64.data, use_native=False, horizon_steps=3)
        chain = np.tile(np.eye(2 * m.nv), (B, 1, 1))
        for _ in range(3):
            Ak, _ = mt.linearize_discrete(h64.model, h64.data, use_native=True)
            chain = Ak @ chain
            h64.step()
        assert np.abs(A3 - chain).max() <= 2e-4 * max(1.0, np.abs(chain).max())


@pytest.mark.parametrize("name,B", [("humanoid", 100), ("drone2", 33), ("cartpole", 64)])
def test_batched_feedback_gemm_kernel_matches_the_host_law(name, B):
    """mjb_feedback_ctrl (SURVEY §8(f) rank 2 as specified: K dx as a batched [B, 2nv] x [2nv, nu] GEMM on MFMA in fp32, plain
    float64 otherwise) incl. the reference law's pre-drawn ctrl noise (lqr.py:160-165) against the numpy law on the host mirrors;
    batches that are not a multiple of the 32-environment tile, nu from 1 to 21."""
    rng = np.random.default_rng(11)
    for dtype, tol in (("float32", None), ("float64", 1e-12)):
        h = mt.ModelHandle.from_xml_path(MODELS[name], batch=B, dtype=dtype)
        m, d = h.model, h.data
        K = rng.normal(size=(m.nu, 2 * m.nv)) * 0.2
        u0 = rng.uniform(-0.2, 0.2, size=m.nu) + (3.0 if name == "drone2" else 0.0)
        ctl = mt.LinearFeedbackController(K=K, ctrl0=u0, qpos_goal=np.array(m.qpos0), qvel_goal=rng.normal(size=m.nv) * 0.01,
                                          ctrl_noise_std=rng.uniform(0.0, 0.05, size=m.nu), perturbations=rng.normal(size=(7, m.nu)), env_stride=3)
        ctl.prepare(m, d)
        dq = rng.normal(size=(B, m.nv)) * 0.1
        q = np.tile(np.array(m.qpos0), (B, 1))
        mj.mj_integratePos(m, q, dq, 1.0)                      # quaternion-aware offsets (humanoid / drone root)
        d.qpos[:] = q
        d.qvel[:] = rng.normal(size=(B, m.nv)) * 0.3
        for step in (0, 5):
            ctl.step_count = step
            want = ctl.host_law(m, d, step)                    # from the float64 mirrors of the (possibly fp32) device state
            ctl(m, d, 0.0)
            got = np.array(d.ctrl)
            assert got.shape == (B, m.nu)
            err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
            if dtype == "float32":
                measured(f"feedback_gemm/{name}/fp32", err, API_TOL32["gemm"][name], "(relative to the largest ctrl)")
            else:
                assert err <= tol, (name, dtype, step, err)
        lim = np.asarray(m.actuator_ctrllimited, dtype=bool)
        assert (got[:, lim] <= m.actuator_ctrlrange[lim, 1] + 1e-12).all() and (got[:, lim] >= m.actuator_ctrlrange[lim, 0] - 1e-12).all()
        # the law inside the fused rollout uses the same noise table (step = the rollout's step counter)
        env = mt.Env.from_xml_path(MODELS[name], controller=mt.LinearFeedbackController(K=K, ctrl0=u0, qpos_goal=np.array(m.qpos0), qvel_goal=ctl.qvel_goal,
                                   ctrl_noise_std=ctl.ctrl_noise_std, perturbations=ctl.perturbations, env_stride=3), batch=B, dtype=dtype)
        env.data.qpos[:] = q
        env.data.qvel[:] = np.array(d.qvel)
        ctl.step_count = 0
        ctl.qpos_goal = np.array(m.qpos0)
        first = ctl.host_law(m, env.data, 0)
        env.rollout(1)
        err = np.abs(np.array(env.data.ctrl) - first).max() / max(1.0, np.abs(first).max())
        if dtype == "float32":
            measured(f"feedback_fused_first_ctrl/{name}/fp32", err, API_TOL32["gemm_fused"][name])
        else:
            assert err <= 1e-12, err


def test_fused_headless_run_waits_for_a_clock_restarted_by_the_bad_state_guard():
    """run_passive_headless's fused path used to fix its step count up front; an in-kernel bad-state reset
    (mj_checkVel -> mj_resetData: that environment's clock restarts at 0) must extend a `duration` run exactly as the per-step
    loop would (runtime.py:631-663 stops when EVERY clock has reached the duration)."""
    def make():
        env = mt.Env.from_xml_path(MODELS["cartpole"], controller=mt.ZeroController(), batch=3, dtype="float32")
        env.data.time = 0.03
        env.data.qvel[1, 0] = 1e12                                   # environment 1 trips the guard at its first step
        return env

    a = make()
    with pytest.warns(RuntimeWarning, match="bad-state"):
        n = runtime.run_passive_headless(a, duration=0.08, chunk=4)
        times = np.array(a.data.time)
    dt = float(a.model.opt.timestep)                                  # 0.01: the healthy clocks need 5 steps, the restarted one 8
    assert n == 8 and times == pytest.approx([0.03 + 8 * dt, 8 * dt, 0.03 + 8 * dt])
    assert a.data.counters()["warn_badqvel"].tolist() == [0, 1, 0]
    b = make()                                                        # the per-step loop (a hook forces it) agrees
    with pytest.warns(RuntimeWarning, match="bad-state"):
        assert runtime.run_passive_headless(b, duration=0.08, hooks=lambda r: None) == 8


def test_c_abi_allgather_obs_runs_ncclallgather_on_a_one_rank_communicator():
    """mjb_allgather_obs (SURVEY §8(b) export list): the path's one collective for a host that owns an ncclComm_t.  Exercised here
    with a one-rank RCCL communicator created through ctypes on the RCCL torch loaded (the multi-rank case is torch.distributed's
    all_gather_into_tensor in the Python front; two ranks cannot share the one GPU of this box)."""
    import ctypes

    import torch

    from mujoco_template_amd._capi import load_library

    L = load_library()
    L.mjb_allgather_obs.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
    L.mjb_allgather_obs.restype = ctypes.c_int
    assert L.mjb_allgather_obs(None, None, None, 4, 0, None) == -1                      # argument check, no RCCL call
    rccl = None
    for name in (os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so"), "librccl.so.1"):
        try:
            rccl = ctypes.CDLL(name, mode=ctypes.RTLD_GLOBAL)
            break
        except OSError:
            continue
    if rccl is None:
        pytest.skip("no loadable librccl")
    class UniqueId(ctypes.Structure):                                                   # ncclUniqueId: 128 opaque bytes, passed BY VALUE
        _fields_ = [("internal", ctypes.c_char * 128)]

    uid = UniqueId()
    rccl.ncclGetUniqueId.argtypes = [ctypes.POINTER(UniqueId)]
    assert rccl.ncclGetUniqueId(ctypes.byref(uid)) == 0
    comm = ctypes.c_void_p()
    rccl.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, UniqueId, ctypes.c_int]
    torch.cuda.set_device(0)
    assert rccl.ncclCommInitRank(ctypes.byref(comm), 1, uid, 0) == 0
    try:
        send = torch.arange(6 * 55, device="cuda", dtype=torch.float32).reshape(6, 55) * 0.5
        recv = torch.zeros_like(send)
        stream = torch.cuda.current_stream().cuda_stream
        assert L.mjb_allgather_obs(comm, ctypes.c_void_p(send.data_ptr()), ctypes.c_void_p(recv.data_ptr()), send.numel(), 0, ctypes.c_void_p(stream)) == 0
        torch.cuda.synchronize()
        assert torch.equal(send, recv)
    finally:
        rccl.ncclCommDestroy.argtypes = [ctypes.c_void_p]
        rccl.ncclCommDestroy(comm)


@pytest.mark.parametrize("global_batch", [24, 25])
def test_sharded_env_gathers_the_global_observation_block(global_batch, tmp_path):
    """The multi-GPU surface of Env (reference signature mujoco_template/env.py:100-143 kept):
    ``Env.from_xml_path(..., batch=GLOBAL, shard=True)`` under torchrun takes its block of the global batch, ``rollout(gather=True)`` /
    ``observe_device(gather=True)`` return the all-gathered block.  Two ranks (gloo: both on this box's one GPU; 24 = equal shards,
    25 = ragged 13 + 12) against the one-process run of the same global batch: bitwise equal - random ctrl is keyed by the global
    environment index.  (RCCL with two ranks needs two GPUs: the nccl form of this path runs in the driver's multi-GPU bench; the
    C-ABI collective on a one-rank RCCL communicator is the next test.)"""
    import socket
    import subprocess
    import sys

    import torch

    one = mt.Env.from_xml_path(MODELS["humanoid"], obs_spec=mt.ObservationSpec(as_dict=False), controller=mt.RandomCtrlController(seed=4), batch=global_batch)
    ring = one.rollout(12, obs_every=4, gather=True).cpu().numpy()          # no shard: gather is the identity
    now = one.observe_device(gather=True).cpu().numpy()
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mp_env_shard_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        worker, str(tmp_path), str(global_batch), "gloo"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rank in (0, 1):
        assert np.array_equal(np.load(tmp_path / f"ring_{rank}.npy"), ring), rank
        assert np.array_equal(np.load(tmp_path / f"now_{rank}.npy"), now), rank
    e0, c, how = open(tmp_path / "info_1.txt").read().split(None, 2)
    assert (int(e0), int(c)) == (global_batch - global_batch // 2, global_batch // 2) and "torch.distributed (gloo)" in how
    del torch


def test_sharded_env_uses_the_c_abi_collective_on_an_rccl_communicator(tmp_path):
    """One rank under torchrun with backend ``nccl``: the sharded Env creates its own RCCL communicator (unique id over the torch group,
    ``ncclCommInitRank``) and its gather goes through ``mjb_allgather_obs`` - the library's own collective, the one a multi-GPU job uses
    when every rank has its GPU."""
    import socket
    import subprocess
    import sys

    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mp_env_shard_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", str(port),
                        worker, str(tmp_path), "16", "nccl"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "mjb_allgather_obs" in open(tmp_path / "info_0.txt").read()
    one = mt.Env.from_xml_path(MODELS["humanoid"], obs_spec=mt.ObservationSpec(as_dict=False), controller=mt.RandomCtrlController(seed=4), batch=16)
    assert np.array_equal(np.load(tmp_path / "ring_0.npy"), one.rollout(12, obs_every=4).cpu().numpy())


def test_humanoid_balances_on_one_leg_under_the_tutorial_lqr_and_fp32_tracks_float64():
    """The reference's humanoid example end to end (examples/humanoid/controllers/lqr.py:34-170), with the recipe of DeepMind's LQR tutorial
    that example transcribes (the reference keeps its text as LQR.txt:159-323,354-417): height sweep by batched ``mj_inverse``, set-point
    ``ctrl0``, ``(A, B)`` from ``linearize_discrete``, COM-over-foot cost from the Jacobians, ``K`` from scipy's DARE, then the law with the
    tutorial's seed-1 smoothed ctrl noise evaluated inside the fused kernel.  Behavioural known answer of real MuJoCo on this very XML and
    noise sequence: the humanoid keeps its balance for the 12 s.  Closed loop = not chaotic, so BASELINE's drift bound applies as written:
    fp32 vs float64 kernels stay within 1e-4 over 1000 steps (measured 6e-6; 1.1e-4 over all 2400 steps, contacts active throughout)."""
    scipy = pytest.importorskip("scipy")  # noqa: F841
    import importlib.util

    spec = importlib.util.spec_from_file_location("gpu_humanoid_lqr", os.path.join(os.path.dirname(os.path.dirname(__file__)), "scripts", "gpu_humanoid_lqr.py"))
    lqr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lqr)
    model = mj.MjModel.from_xml_path(MODELS["humanoid"])
    assert model.body("torso").id == 1 and model.joint(3).name == "abdomen_x"            # the named accessors the example uses (lqr.py:93-95,222)
    with pytest.raises(KeyError):
        model.body("no_such_body")
    d = lqr.design(model, lqr.TUTORIAL, verbose=False)
    assert d["bal"].tolist() == [7, 8, 15, 17, 18, 19, 20]                                 # abdomen_y/x + left hip_x/y, knee, ankle_y/x
    assert -1e-3 < d["offset"] < 0 and abs(d["forces"][-1] - 40.8446 * 9.81) < 0.05        # +1 mm: foot off the floor, residual = the weight
    assert np.abs(d["ctrl0"]).max() < 1.0 and abs(d["rho"] - 1.0) < 1e-6                   # set-point inside ctrlrange; marginal translation modes only
    assert float(np.abs(np.linalg.eigvals(d["A"])).max()) > 1.03                           # open loop: unstable (it falls without feedback)
    up64, up32, dev = lqr.single_env_pair(d, 12.0, verbose=False)
    assert up64 and up32
    measured("humanoid_lqr/fp32_vs_float64_kernels_1000_steps", max(dev[:5]), API_TOL32["lqr_1000_pair"], "(BASELINE: <= 1e-4 over 1000 steps)")
    assert max(dev) < 1e-3, dev
    # the float64 kernels against the ORACLE driven by the same law from Python (differentiatePos, K dx, noise row s, clip), 1000 closed-loop steps
    from oracle import mjo
    from mujoco_template_amd import mjcf as _mjcf

    om = mjo.OracleModel(_mjcf.compile_xml_path(MODELS["humanoid"]))
    od = mjo.OracleData(om)
    od.reset(); od.qpos[:] = d["qpos0"]; od.qvel[:] = 0
    lo, hi = model.actuator_ctrlrange[:, 0], model.actuator_ctrlrange[:, 1]
    for s_ in range(1000):
        dx = np.concatenate([od.differentiate_pos(d["qpos0"], od.qpos), od.qvel])
        od.ctrl[:] = np.clip(d["ctrl0"] - d["K"] @ dx + d["ctrl_std"] * d["perturbations"][s_], lo, hi)
        od.step()
    ctl = mt.LinearFeedbackController(K=d["K"], ctrl0=d["ctrl0"], qpos_goal=d["qpos0"], ctrl_noise_std=d["ctrl_std"], perturbations=d["perturbations"], env_stride=0)
    e64 = mt.Env.from_xml_path(MODELS["humanoid"], controller=ctl, keyframe=1, batch=1, dtype="float64")
    e64.data.qpos[...] = d["qpos0"]
    e64.data.qvel[...] = 0.0
    e64.rollout(1000)
    assert np.abs(np.array(e64.data.qpos, dtype=float).ravel() - od.qpos).max() < 1e-8      # same algorithm, different summation order, stabilised loop
    ctl32 = mt.LinearFeedbackController(K=d["K"], ctrl0=d["ctrl0"], qpos_goal=d["qpos0"], ctrl_noise_std=d["ctrl_std"], perturbations=d["perturbations"], env_stride=0)
    e32 = mt.Env.from_xml_path(MODELS["humanoid"], controller=ctl32, keyframe=1, batch=1, dtype="float32")
    e32.data.qpos[...] = d["qpos0"]
    e32.data.qvel[...] = 0.0
    e32.rollout(1000)
    drift = float(np.abs(np.array(e32.data.qpos, dtype=float).ravel() - od.qpos).max())
    measured("humanoid_lqr/fp32_vs_oracle_1000_steps", drift, API_TOL32["lqr_1000_oracle"], "(BASELINE / north_star: fp32 qpos drift vs the CPU reference over 1000 steps <= 1e-4)")
    # the closed loop does not depend on how the batch is scheduled: two-wave kernel (512 environments), ticket map (4096), every environment
    # at its own phase of the noise table -> the first 512 environments are bitwise the same
    def closed_loop(batch):
        ctl = mt.LinearFeedbackController(K=d["K"], ctrl0=d["ctrl0"], qpos_goal=d["qpos0"], ctrl_noise_std=d["ctrl_std"],
                                          perturbations=d["perturbations"], env_stride=3)
        env = mt.Env.from_xml_path(MODELS["humanoid"], controller=ctl, keyframe=1, batch=batch)
        env.data.qpos[...] = d["qpos0"]
        env.data.qvel[...] = 0.0
        env.rollout(150)
        return np.array(env.data.qpos), env.data.sim.schedule_info()
    qa, sa = closed_loop(512)
    qb, sb = closed_loop(4096)
    assert sa["waves_per_env"] == 2 and sb["map"] == "tickets"
    assert np.array_equal(qb[:512], qa) and np.abs(qa - d["qpos0"]).max() > 1e-3


def test_cartpole_config2_batch_1024_recovers_under_the_references_pid_as_a_device_law(oracle):
    """The reference's cart-pole example on the engine at BASELINE config[1]'s batch: its PID law with the shipped gains
    (examples/cartpole/controllers/pid.py:26-49, cartpole_config.py:72-79; ki = 0, so it IS a linear state feedback) as a
    LinearFeedbackController inside the fused kernel, 1024 initial pole angles across +-30 degrees (the example starts at 30).  Every
    environment settles at the origin in fp32 and float64; the 30-degree one follows the oracle driven by the same law from Python."""
    B = 1024
    K = -np.array([[1.11, 16.66, 2.20, 4.45]])                      # ctrl = u0 - K [q - q0; v]  ->  + kp_x x + kp_th th + kd_x xd + kd_th thd
    ang = np.deg2rad(np.linspace(-30.0, 30.0, B))
    out = {}
    for dtype in ("float64", "float32"):
        ctl = mt.LinearFeedbackController(K=K, ctrl0=np.zeros(1), qpos_goal=np.zeros(2))
        env = mt.Env.from_xml_path(MODELS["cartpole"], controller=ctl, batch=B, dtype=dtype)
        env.data.qpos[:, 0] = 0.0
        env.data.qpos[:, 1] = ang
        env.data.qvel[...] = 0.0
        env.rollout(300)
        mid = np.array(env.data.qpos)
        env.rollout(900)
        q, v = np.array(env.data.qpos), np.array(env.data.qvel)
        assert np.abs(q).max() < 2e-3 and np.abs(v).max() < 2e-3, dtype
        out[dtype] = mid
    m, d = oracle("cartpole")
    d.reset(); d.qpos[:] = [0.0, ang[-1]]; d.qvel[:] = 0
    for s in range(300):
        d.ctrl[0] = np.clip(1.11 * d.qpos[0] + 2.20 * d.qvel[0] + 16.66 * d.qpos[1] + 4.45 * d.qvel[1], -200.0, 200.0)
        d.step()
    assert np.abs(out["float64"][-1] - d.qpos).max() < 1e-9
    measured("cartpole_pid/fp32_vs_oracle_300_steps", np.abs(out["float32"][-1] - d.qpos).max(), API_TOL32["pid_300_oracle"], "(closed loop: BASELINE's drift bound 1e-4)")
    measured("cartpole_pid/fp32_vs_float64_kernels_300_steps", np.abs(out["float32"] - out["float64"]).max(), API_TOL32["pid_300_pair"])


def test_module_smoke_cli_runs_baseline_config_0():
    """``python -m mujoco_template_amd pendulum.xml --steps 200 --zero`` = the reference's smoke CLI (mujoco_template/__main__.py:10-33) on
    BASELINE config[0] (pendulum, ZeroController, Env.passive, 200 steps, batch 1), and the same flags with a batch."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra in ([], ["--batch", "64"], ["--decim", "2"]):
        r = subprocess.run([sys.executable, "-m", "mujoco_template_amd", MODELS["pendulum"], "--steps", "200", "--zero", *extra],
                           capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Completed 200 steps." in r.stdout
    r = subprocess.run([sys.executable, "-m", "mujoco_template_amd", MODELS["pendulum"], "--steps", "7"], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "Completed 7 steps." in r.stdout, r.stdout + r.stderr


def test_drone_example_law_with_yaw_shaping_and_integral_matches_its_literal_restatement():
    """The drone example's controller (examples/drone2/main.py:400-471): LQR delta, yaw P / D / I shaping along the yaw control direction
    ``B[yaw_rate_row]``, yaw control scale, clip.  ``LinearFeedbackController.fold_yaw_shaping`` puts the P, D and scale terms into the gain
    matrix and ``integ_*`` carry the clipped yaw integral; the result drives a batch exactly like the example's own per-step arithmetic
    (restated literally below, one environment, Python) - and a law with integrator state is host-batched, never fused."""
    rng = np.random.default_rng(5)
    probe = mt.Env.from_xml_path(MODELS["drone2"], keyframe="hover", batch=1, dtype="float64")
    m = probe.model
    nu, nv = m.nu, m.nv
    q_goal, u_hover = np.array(probe.data.qpos, dtype=float).ravel(), np.array(probe.data.ctrl, dtype=float).ravel()
    A, Bm = mt.linearize_discrete(m, probe.data, eps=1e-6)
    yaw_err, yaw_rate = 5, nv + 5                                   # pos_dim + rot_dim - 1, nv + pos_dim + rot_dim - 1 (main.py:379-383,432-433)
    ydir = np.array(Bm[yaw_rate, :nu], dtype=float)
    assert float(ydir @ ydir) > 0
    K = rng.normal(size=(nu, 2 * nv)) * 0.05
    kp, kd, ki, scale, lim, dt = 18.0, 4.5, 4.0, 6.0, 6.0, float(m.opt.timestep)      # the example's defaults (main.py:36-40)
    lo, hi = m.actuator_ctrlrange[:, 0], m.actuator_ctrlrange[:, 1]

    class Literal:                                                   # the example's __call__, line by line, one environment
        capabilities = mt.ControllerCapabilities(control_space=mt.ControlSpace.TORQUE)
        def prepare(self, model, data):
            self.integral = 0.0
        def __call__(self, model, data, t):
            dq = np.zeros(nv)
            mj.mj_differentiatePos(model, dq, 1.0, q_goal, np.array(data.qpos, dtype=float).ravel())
            dx = np.concatenate([dq, np.array(data.qvel, dtype=float).ravel()])
            delta = K @ dx
            self.integral = float(np.clip(self.integral + dx[yaw_err] * dt, -lim, lim))
            delta = delta + ki * self.integral * ydir
            delta = delta + (kp * dx[yaw_err] + kd * dx[yaw_rate]) * ydir
            delta = delta + (scale - 1.0) * (float(delta @ ydir) / float(ydir @ ydir)) * ydir
            data.ctrl[...] = np.clip(u_hover - delta, lo, hi).reshape(np.shape(data.ctrl))

    # the integral term enters BEFORE the scale in the example: its gain along ydir is ki * scale after folding
    Kf = mt.LinearFeedbackController.fold_yaw_shaping(K, ydir, yaw_err, yaw_rate, proportional_gain=kp, derivative_gain=kd, control_scale=scale)
    rows = np.zeros((1, 2 * nv)); rows[0, yaw_err] = 1.0
    ours = mt.LinearFeedbackController(K=Kf, ctrl0=u_hover, qpos_goal=q_goal, integ_rows=rows, integ_gain=(ki * scale * ydir)[None, :], integ_limit=[lim])

    def make(ctl, batch):
        env = mt.Env.from_xml_path(MODELS["drone2"], controller=ctl, keyframe="hover", batch=batch, dtype="float64")
        q = np.atleast_2d(env.data.qpos)
        q[:, 2] += 0.4
        q[:, 3:7] = np.array([np.cos(0.15), 0.0, 0.0, np.sin(0.15)])            # 0.3 rad of yaw error: the integral and the clip matter
        v = np.atleast_2d(env.data.qvel)
        v[:, 5] = 0.5
        return env
    a, b = make(Literal(), 1), make(ours, 3)
    assert not b.can_fuse() and ours.device_ctrl_mode is None
    for _ in range(120):
        a.step(return_obs=False)
        b.step(return_obs=False)
    qa, qb = np.array(a.data.qpos, dtype=float).ravel(), np.array(b.data.qpos, dtype=float)
    assert np.abs(qb - qa).max() < 1e-10 and np.abs(np.array(b.data.ctrl) - np.array(a.data.ctrl).ravel()).max() < 1e-9
    assert abs(ours._integ[0, 0]) > 1e-3 and np.abs(qa - q_goal).max() > 1e-2
    # without integrators the same controller class is the fused device law again
    plain = mt.LinearFeedbackController(K=Kf, ctrl0=u_hover, qpos_goal=q_goal)
    assert make(plain, 2).can_fuse()


def test_bench_dump_outputs_hold_what_the_timed_path_computed_in_its_last_step(tmp_path):
    """`bench.py --dump-outputs DIR` writes the observation ring of the last timed launch and the state after the last timed step: bit
    for bit what the same rollout (5 warm-up steps, then the 30 timed ones in one launch) returns in this process."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5", "--global-batch", "64",
                        "--obs-every", "10", "--no-cpu-baseline", "--no-host-loop", "--no-other-configs", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 30 and line["ms_per_step"] > 0 and not line["outputs_dumped"]["sampled"]
    got = {k: np.load(tmp_path / "out" / f"{k}.npy") for k in ("obs", "qpos", "qvel", "ctrl", "qacc")}
    assert all(a.dtype == np.float32 for a in got.values())
    env = mt.Env.from_xml_path(MODELS["humanoid"], obs_spec=mt.ObservationSpec(as_dict=False), controller=mt.RandomCtrlController(seed=0, scale=1.0),
                               batch=64, shard=True, dtype="float32")
    env.rollout(5, obs_every=5)
    ring = env.rollout(30, obs_every=10).cpu().numpy()
    assert got["obs"].shape == (3, 64, env.model.nq + env.model.nv) and np.array_equal(got["obs"], ring)
    for k in ("qpos", "qvel", "ctrl", "qacc"):
        assert np.array_equal(got[k], env.data.sim.torch_view(k).cpu().numpy()), k
    np.testing.assert_allclose(got["obs"][-1], np.concatenate([got["qpos"], got["qvel"]], axis=1), rtol=1e-6, atol=1e-6)   # the ring's last row: the last step
