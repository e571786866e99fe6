"""Work the step loop does once per launch or once per several steps instead of every step, on the real kernels (fp32, at most 64
environments): random controls drawn for floor(lanes / nu) steps in one Philox pass, the world body's constants written in front
of the step loop, and cdof formed with one lane per dof.  Everything is pinned bit for bit: a launch against the same steps cut
into shorter launches (every launch starts a pass of its own, so the cuts fall at every phase of a pass), the kernel variants
against each other, a poisoned environment against its neighbours."""
import numpy as np
import pytest

from mujoco_template_amd import mjcf
from mujoco_template_amd._capi import CTRL_RANDOM, BatchSim, DeviceModel
from tests.conftest import CAPSULES_XML, MODELS, chain_xml
from tests.large_models import initial_state, two_free_xml
from tests.step_invariants_models import GUARD_XML, poisoned_state

pytestmark = pytest.mark.gpu

STATE = ("qpos", "qvel", "qacc", "qacc_warmstart", "ctrl")
SEED = 11


def _shipped(name):
    cm = mjcf.compile_xml_path(MODELS[name])
    return cm, DeviceModel(cm)


def _start(cm, B, seed=0, spread=0.05):
    rng = np.random.default_rng(seed)
    q = np.tile(np.asarray(cm.qpos0, dtype=np.float64), (B, 1))
    v = rng.normal(size=(B, cm.nv)) * spread
    return q, v


def _make(dm, q, v, monkeypatch, *, variant="spec", chunk="0", **caps):
    """A data object at (q, v) whose first stepping launch reads the launch policy set here (it is read once per object)."""
    monkeypatch.setenv("MJB_TWO_WAVE", "1" if variant == "two" else "0")
    monkeypatch.setenv("MJB_CHUNK_STEPS", chunk)
    sim = BatchSim(dm, q.shape[0], dtype="float32", specialize=variant != "generic", **caps)
    assert sim.specialized == (variant != "generic")
    sim.set("qpos", q); sim.set("qvel", v)
    return sim


def _launches(sim, N, piece, scale, step0=50):
    done = 0
    while done < N:
        n = min(piece, N - done)
        sim.rollout(n, CTRL_RANDOM, seed=SEED, step0=step0 + done, ctrl_scale=scale)
        done += n
    return {k: sim.get(k) for k in STATE}


def _same(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what} {k}: {int((a[k] != b[k]).sum())} of {a[k].size} values differ"


# (model, lanes, steps per pass k, steps N, batch, control scale, kernel variants).  The shipped models have their specialised kernels
# in the build's cache; the others run the generic kernel (a specialised one would be compiled inside the test).
#   humanoid   21 actuators on 64 lanes: k = 3           drone2   4 on 16: k = 4            cart-pole   1 on 8: k = 8
#   chain17 at 8 lanes: 5 actuators, more than half the lanes: k = 1        two capsules: no actuator, nothing to draw
ROLLOUTS = [("humanoid", 0, 3, 7, 5, 1.0, ("spec", "generic", "two")), ("drone2", 0, 4, 9, 9, 0.3, ("spec", "generic")),
            ("cartpole", 0, 8, 17, 19, 0.01, ("spec", "generic")), ("chain17", 8, 1, 5, 11, 0.5, ("generic",)), ("capsules", 0, 0, 5, 3, 1.0, ("generic",))]


def _rollout_model(name):
    if name == "chain17":
        cm = mjcf.compile_xml_string(chain_xml(17))
        return cm, DeviceModel(cm), dict(nconmax=16, nefcmax=72)
    if name == "capsules":
        cm = mjcf.compile_xml_string(CAPSULES_XML)
        return cm, DeviceModel(cm), {}
    return (*_shipped(name), {})


@pytest.mark.parametrize("name,lanes,k,N,B,scale,variants", ROLLOUTS)
def test_one_launch_equals_shorter_launches(name, lanes, k, N, B, scale, variants, monkeypatch):
    """N steps in one launch == the same N steps as launches of 1, 2 and k + 1 steps: state, warm start and ctrl after the last step."""
    cm, dm, caps = _rollout_model(name)
    if lanes:
        caps["lanes"] = lanes
    q, v = _start(cm, B)
    ref = None
    for variant in variants:
        whole = _make(dm, q, v, monkeypatch, variant=variant, **caps)
        got = _launches(whole, N, N, scale)
        assert whole.schedule_info()["waves_per_env"] == (2 if variant == "two" else 1)
        lanes_used = whole.lanes
        assert (lanes_used // cm.nu if 0 < cm.nu <= lanes_used else 0) == k, (lanes_used, cm.nu)
        assert np.isfinite(got["qpos"]).all()
        if cm.nu:
            assert np.abs(got["ctrl"]).max() > 0
        if ref is None:
            ref = got
        _same(ref, got, f"{variant} against {variants[0]}")
        for piece in sorted({1, 2, k + 1}):
            _same(ref, _launches(_make(dm, q, v, monkeypatch, variant=variant, **caps), N, piece, scale), f"{variant}, launches of {piece}")


@pytest.mark.parametrize("chunk", [2, 4])
def test_ticket_chunks_start_at_every_phase_of_a_pass(chunk, monkeypatch):
    """The humanoid (3 steps per pass) under the ticket map with chunks of 2 and of 4 steps: a chunk starts a pass of its own at its
    first step, whatever that is modulo 3."""
    cm, dm = _shipped("humanoid")
    q, v = _start(cm, 5)
    static = _make(dm, q, v, monkeypatch)
    ref = _launches(static, 7, 7, 1.0)
    assert static.schedule_info()["map"] == "static"
    tick = _make(dm, q, v, monkeypatch, chunk=str(chunk))
    got = _launches(tick, 7, 7, 1.0)
    info = tick.schedule_info()
    assert info["map"] == "tickets" and info["chunk_steps"] == chunk
    _same(ref, got, f"tickets of {chunk}")


def test_reset_in_mid_pass_leaves_the_others_and_the_stream_alone(monkeypatch):
    """One environment's weight falls at the bad-state bound: the first step carries it past the bound, the qvel guard resets it at
    the top of the second step - the second of a four-step pass (8 lanes, 2 actuators).  Every other environment, the seven that
    share the victim's wavefront included, is bitwise what it is without the poison; the victim's ctrl after the launch is the
    stream's value for the last step (what it holds in the run without the poison), and its state is that of an environment with
    its global index that starts at qpos0 at step 1."""
    cm = mjcf.compile_xml_string(GUARD_XML)
    dm = DeviceModel(cm)
    B, victim, N = 19, 10, 6
    q, v = poisoned_state(B, victim)
    q0, v0 = q.copy(), v.copy()
    q0[victim], v0[victim] = q[0], v[0]

    def run(qq, vv, n, step0=0):
        sim = _make(dm, qq, vv, monkeypatch, variant="generic")
        assert sim.lanes == 8
        out = _launches(sim, n, n, 1.0, step0=step0)
        c = sim.counters()
        return out, np.stack([c["warn_badqpos"], c["warn_badqvel"], c["warn_badqacc"]], axis=1)

    _, bad1 = run(q, v, 1)
    assert bad1.sum() == 0                                         # the first step runs from the poisoned state
    _, bad2 = run(q, v, 2)
    assert bad2[victim].tolist() == [0, 1, 0] and bad2.sum() == 1  # the guard fires at the top of the second step
    got, bad = run(q, v, N)
    ref, badref = run(q0, v0, N)
    assert bad[victim].tolist() == [0, 1, 0] and bad.sum() == 1 and badref.sum() == 0
    others = np.arange(B) != victim
    for k in STATE:
        assert got[k][others].tobytes() == ref[k][others].tobytes(), k
    assert got["ctrl"][victim].tobytes() == ref["ctrl"][victim].tobytes() and np.abs(got["ctrl"][victim]).max() > 0
    fresh, _ = run(np.zeros_like(q), np.zeros_like(v), N - 1, step0=1)   # qpos0 (zeros in this model), at rest, from step 1
    for k in STATE:
        assert got[k][victim].tobytes() == fresh[k][victim].tobytes(), k
    assert np.isfinite(got["qpos"]).all()


def _assert_world(sim, rows=None):
    sel = slice(None) if rows is None else rows
    assert (sim.get("xpos")[sel, :3] == 0).all() and (sim.get("xipos")[sel, :3] == 0).all()
    assert (sim.get("xquat")[sel, :4] == np.array([1, 0, 0, 0], dtype=np.float32)).all()


def _assert_world_dumps(sim):
    sim.debug_forward()
    assert (sim.debug_get("cinert")[:, :10] == 0).all() and (sim.debug_get("cvel")[:, :6] == 0).all()
    assert np.abs(sim.debug_get("cinert")[:, 10:]).max() > 0
    _assert_world(sim)


def _poison_world(sim, nbody):
    for k, n in (("xpos", 3), ("xquat", 4), ("xipos", 3)):
        sim.set(k, np.full((sim.batch, n * nbody), np.nan))


@pytest.mark.parametrize("name,variant", [("humanoid", "spec"), ("humanoid", "generic"), ("humanoid", "two"), ("two_free", "generic"), ("chain17", "generic")])
def test_world_body_entries_after_a_launch(name, variant, monkeypatch):
    """xpos[0], xquat[0], xipos[0], cinert[0], cvel[0] hold the world body's constants after a stepping launch, a forward launch, a
    masked forward and a launch after a per-environment reset.  two_free (55 bodies, 64 lanes) takes the per-level tree sums,
    chain17 at 8 lanes also the per-level kinematics."""
    caps = {}
    if name == "humanoid":
        cm, dm = _shipped(name)
        q, v = _start(cm, 6)
    else:
        cm = mjcf.compile_xml_string(two_free_xml() if name == "two_free" else chain_xml(17))
        dm = DeviceModel(cm)
        caps = dict(lanes=64) if name == "two_free" else dict(lanes=8, nconmax=16, nefcmax=72)
        rng = np.random.default_rng(3)
        qs, vs = zip(*(initial_state(cm, name, rng) for _ in range(6)))
        q, v = np.stack(qs), np.stack(vs)
    sim = _make(dm, q, v, monkeypatch, variant=variant, **caps)
    _poison_world(sim, cm.nbody)                                   # whatever the arrays held: every launch writes the world body's entries
    sim.rollout(4, CTRL_RANDOM, seed=SEED, ctrl_scale=0.2)
    assert sim.schedule_info()["waves_per_env"] == (2 if variant == "two" else 1)
    _assert_world(sim)
    assert np.isfinite(sim.get("xpos")).all()
    _assert_world_dumps(sim)                                        # forward mode, with the dumps
    _poison_world(sim, cm.nbody)
    mask = np.zeros(6, dtype=bool); mask[[1, 4]] = True
    sim.forward_envs(mask)
    _assert_world(sim, rows=mask)
    sim.reset_envs(mask)
    sim.rollout(2, CTRL_RANDOM, seed=SEED, step0=4, ctrl_scale=0.2)
    _assert_world(sim)
    _assert_world_dumps(sim)


def _cdof(dm, q, v, variant, monkeypatch, **caps):
    sim = _make(dm, q, v, monkeypatch, variant=variant, **caps)
    sim.debug_forward()
    return sim.debug_get("cdof"), sim


@pytest.mark.parametrize("name", ["humanoid", "drone2", "cartpole", "pendulum"])
def test_cdof_is_the_same_in_every_kernel_variant(name, monkeypatch):
    """cdof dumped in forward mode, generic against specialised kernel: a free joint (humanoid, drone2), a slide joint (cart-pole),
    neither (pendulum).  The two-wave kernel has no forward mode and no dumps (stepping launches only): it is pinned through the
    state after three steps, which every entry of cdof enters through the mass matrix and the bias forces."""
    cm, dm = _shipped(name)
    rng = np.random.default_rng(5)
    q, v = _start(cm, 7, seed=5, spread=0.3)
    oracle_q = np.ascontiguousarray(q, dtype=np.float64)
    dm.integrate_pos(oracle_q, rng.normal(size=(7, cm.nv)) * 0.2, 1.0)   # states off qpos0: turned joints and, for a free joint, a turned frame
    gen, _ = _cdof(dm, oracle_q, v, "generic", monkeypatch)
    spec, _ = _cdof(dm, oracle_q, v, "spec", monkeypatch)
    assert np.isfinite(gen).all() and np.abs(gen).max() > 0
    assert gen.tobytes() == spec.tobytes(), f"{int((gen != spec).sum())} of {gen.size} values differ"
    if dm.step2_spec_source() is None:
        return
    res = []
    for variant in ("generic", "two"):
        sim = _make(dm, oracle_q, v, monkeypatch, variant=variant)
        sim.rollout(3, CTRL_RANDOM, seed=SEED, ctrl_scale=0.3)
        assert sim.schedule_info()["waves_per_env"] == (2 if variant == "two" else 1)
        res.append({k: sim.get(k) for k in STATE})
    _same(res[0], res[1], "two-wave against generic")
