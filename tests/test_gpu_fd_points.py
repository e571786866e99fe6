"""Linearising whole rollouts on the GPU: ``mjb_transition_fd_points`` / ``BatchSim.transition_fd_points`` (finite-difference
transition matrices at T x B points held in device tensors), the warm-start column of the rollout ring (observation flag 128,
``rollout(return_warmstart=True)``) and ``linearize_rollout``.

The definition is bitwise: block (t, e) is what ``transition_fd`` returns for environment e once the data's rows hold point (t, e),
so ``linearize_rollout`` equals the host loop ``for t: ctrl <- u[:, t]; transition_fd(); step(1)``.  Every point is also compared
with the float64 oracle's ``mjo_transition_fd`` about the recorded device state.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mujoco_template_amd import ConfigError, TemplateError, linearize_rollout, mj, mjcf, rollout  # noqa: E402
from mujoco_template_amd._capi import CTRL_RANDOM, BatchSim, DeviceModel, load_library  # noqa: E402
from oracle import mjo  # noqa: E402
from tests.conftest import MODELS, measured  # noqa: E402
from tests.model_params_oracle import env_oracle  # noqa: E402

NAMES = ("pendulum", "cartpole", "drone2", "humanoid")
DTYPES = ("float64", "float32")
B4, T8 = 4, 8
CTRL_SCALE = {"pendulum": 1.0, "cartpole": 0.005, "drone2": 1.0, "humanoid": 1.0}   # cart-pole: +-1 of its +-200 range keeps the cart off its joint limits
STATE = ("qpos", "qvel", "ctrl", "qacc", "qacc_warmstart", "time")

# Device float64 FD at the points of a trajectory vs the oracle's FD about the same recorded state, relative to max(1, largest entry),
# worst over the T x B = 32 points; each tolerance <= 3x the value measured on an MI355X (measured values in the comments).
# The arithmetic is that of transition_fd, whose bounds in tests/test_gpu_parity.py are FD_TOL (pendulum 4.2e-11, cartpole 2.5e-10, drone2
# 8.4e-11) and, for the humanoid in contact, FD_CONTACT_TOL (3.0e-9 / 3.4e-9).
#  * drone2 is above 10x its bound (measured 7.5e-10 = 9x, tolerance 2.2e-9).  Cause: rounding of the next state.  The errors are whole
#    multiples of 2^-54 / 2e-6 = 2.8e-11 (7.5e-10 = 27 of them, a 1.5e-15 = 7 ulp(1) disagreement of one next-state entry of magnitude
#    1 .. 2 between two implementations of a step), they sit in A, not in B, and they do not follow the thrust: 4.2e-10 / 2.8e-10 /
#    3.7e-10 / 7.5e-10 at 2 % / 10 % / 30 % / 100 % of the control range, |qvel| up to 0.84 / 0.85 / 0.87 / 1.66.  The states here are
#    2.5x as far from qpos0 and twice as fast as those of the parity test (0.05 / 0.2 against 0.02 / 0.1), so the entries whose
#    roundings are differenced are several times larger.
#  * humanoid: every point whose solve was refined by a second Newton iteration is bound by 2.8e-8 (3x the 9.5e-9 measured, below
#    10x FD_CONTACT_TOL).  Points where the oracle's solver stops after ONE Newton iteration from the warm start (solver_niter = 1: the
#    second iteration finds no improvement even at tolerance 0, so the rounding error of that single solve, Hessian condition 1.4e4 at
#    |qacc| = 1.1e3, is never refined) are bound apart, by 2.1e-7: the two largest errors of the run are two of its three such
#    points, 6.8e-8 and 1.4e-8 (a 9.4e-13 disagreement of one next velocity, 1.7e-13 of |qacc| h, against cond * 2^-53 = 1.5e-12).  Both
#    are in B, whose largest entry is 6.9; the same absolute error in A (largest entry 138) is 3.5e-9 relative.  This is the explanation
#    the evidence supports, not a proof: conditioning alone does not single these points out.
FD_POINTS_TOL = {
    ("pendulum", "float64"): 1.7e-10, ("pendulum", "float32"): 1.7e-10,        # measured 2.8e-11 / 5.6e-11
    ("cartpole", "float64"): 3.3e-10, ("cartpole", "float32"): 3.3e-10,        # measured 1.1e-10 / 8.3e-11
    ("drone2", "float64"): 2.2e-9, ("drone2", "float32"): 1.7e-9,              # measured 7.5e-10 / 5.6e-10
    ("humanoid", "float64"): 2.8e-8, ("humanoid", "float32"): 2.8e-8,          # points with solver_niter > 1: measured 9.5e-9 / 9.7e-9
}
FD_POINTS_PARAMS_TOL = {                                                       # the same with per-environment body_mass / actuator_gear rows
    ("pendulum", "float64"): 1.7e-10, ("pendulum", "float32"): 1.7e-10,        # measured 5.6e-11 / 2.8e-11
    ("cartpole", "float64"): 3.3e-10, ("cartpole", "float32"): 3.3e-10,        # measured 1.1e-10 / 1.1e-10
    ("drone2", "float64"): 2.0e-9, ("drone2", "float32"): 1.8e-9,              # measured 6.7e-10 / 6.1e-10
    ("humanoid", "float64"): 2.8e-8, ("humanoid", "float32"): 2.8e-8,          # measured 2.3e-8 / 1.4e-8 over all points
}
# humanoid points with solver_niter == 1 (in all four humanoid runs the largest error is at such a point): measured 6.8e-8 / 7.0e-8, and
# 2.3e-8 / 1.4e-8 with per-environment rows
FD_SINGLE_NEWTON_TOL = {(False, "float64"): 2.1e-7, (False, "float32"): 2.1e-7, (True, "float64"): 6.8e-8, (True, "float32"): 4.3e-8}


def _tdt(dtype):
    import torch

    return torch.float32 if dtype == "float32" else torch.float64


@pytest.fixture(scope="module")
def world():
    cache = {}

    def get(name):
        if name not in cache:
            cm = mjcf.compile_xml_path(MODELS[name])
            cache[name] = (cm, mjo.OracleModel(cm), mj.MjModel.from_xml_path(MODELS[name]))
        return cache[name]

    return get


def _start_state(cm, om, name, B, seed=0, pair=False):
    """fp32-representable start states: the humanoid standing at qpos0 (feet on the floor) with a small velocity, the others scattered
    about qpos0.  ``pair``: environments 0 and 1 start alike."""
    od = mjo.OracleData(om)
    rng = np.random.default_rng(seed)
    if name == "humanoid":
        q = np.tile(np.asarray(cm.qpos0, dtype=np.float64), (B, 1))
        v = rng.normal(size=(B, cm.nv)) * 0.02
    else:
        q = np.stack([od.integrate_pos(cm.qpos0, rng.normal(size=cm.nv) * 0.05, 1.0) for _ in range(B)])
        v = rng.normal(size=(B, cm.nv)) * 0.2
    w = rng.normal(size=(B, cm.nv)) * 0.1
    if pair:
        q[1], v[1], w[1] = q[0], v[0], w[0]
    f = lambda x: x.astype(np.float32).astype(np.float64)   # noqa: E731
    return f(q), f(v), f(w)


def _table(cm, name, B, T, dtype, seed=1, pair=False):
    import torch

    lo, hi = np.full(cm.nu, -1.0), np.full(cm.nu, 1.0)
    rg = np.reshape(np.asarray(cm.arrays["actuator_ctrlrange"], dtype=np.float64), (-1, 2))
    lim = np.asarray(cm.arrays["actuator_ctrllimited"]).astype(bool)
    lo[lim], hi[lim] = rg[lim, 0], rg[lim, 1]
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * CTRL_SCALE[name]
    u = np.random.default_rng(seed).uniform(mid - half, mid + half, size=(B, T, cm.nu)).astype(np.float32)
    if pair:
        u[1] = u[0]
    return torch.from_numpy(u).to(device="cuda", dtype=_tdt(dtype))


def _params(cm, B, seed=5):
    """body_mass and actuator_gear rows that differ between the environments (+-20 %)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in ("body_mass", "actuator_gear"):
        own = np.array(cm.arrays[k], dtype=np.float64)
        out[k] = np.broadcast_to(own, (B, *own.shape)) * rng.uniform(0.8, 1.2, (B, *own.shape))
    return out


def _make(mm, dtype, q, v, prm, specialize=None):
    data = mj.MjData(mm, batch=q.shape[0], dtype=dtype, specialize=specialize)
    sim = data.sim
    if prm:
        sim.set_env_params(**prm)
    sim.set("qpos", q); sim.set("qvel", v)
    sim.forward()
    sim.sync()
    return data


def _host_loop(sim, u, w0, T):
    """The definition: for t: ctrl <- u[:, t]; (A_t, B_t) <- transition_fd(); step(1).  Also records the device state each
    linearisation was taken at (what the oracle is set to) and the state after each step."""
    import torch

    sim.use_torch_stream()
    sim.torch_view("qacc_warmstart").copy_(w0)
    ctrl = sim.torch_view("ctrl")
    As, Bs, pre, rows, ws_after = [], [], [], [], []
    for t in range(T):
        ctrl.copy_(u[:, t])
        sim.sync()
        pre.append({k: sim.get(k) for k in ("qpos", "qvel", "ctrl", "qacc_warmstart")})
        A, Bm = sim.transition_fd(1e-6, True)
        As.append(A); Bs.append(Bm)
        sim.step(1)
        rows.append(torch.cat([sim.torch_view("time").to(u.dtype), sim.torch_view("qpos"), sim.torch_view("qvel")], dim=1).clone())
        ws_after.append(sim.torch_view("qacc_warmstart").clone())
    sim.sync()
    return (np.stack(As, axis=1), np.stack(Bs, axis=1), pre, torch.stack(rows, dim=1).cpu().numpy(), torch.stack(ws_after, dim=1).cpu().numpy())


@pytest.fixture(scope="module")
def runs(world):
    """(model, dtype, with per-environment parameters) -> both ways of linearising the same T = 8 trajectory of B = 4 environments."""
    cache = {}

    def get(name, dtype, with_params):
        import torch

        key = (name, dtype, with_params)
        if key not in cache:
            cm, om, mm = world(name)
            q, v, w = _start_state(cm, om, name, B4, pair=with_params)
            prm = _params(cm, B4) if with_params else None
            u = _table(cm, name, B4, T8, dtype, pair=with_params)
            w0 = torch.from_numpy(w).to(device="cuda", dtype=_tdt(dtype))
            spec = False if with_params else None              # batched rows: the generic kernel (no per-test compile of a parameterised one)
            fused, loop = _make(mm, dtype, q, v, prm, spec), _make(mm, dtype, q, v, prm, spec)
            state, sens, A, Bm = linearize_rollout(mm, fused, u, initial_warmstart=w0)
            fused.sim.sync()
            assert A.shape == (B4, T8, 2 * cm.nv, 2 * cm.nv) and Bm.shape == (B4, T8, 2 * cm.nv, cm.nu)
            assert A.dtype == torch.float64 and A.is_cuda and not A.is_contiguous()          # permuted views of the [T, B, ...] blocks
            assert state.shape == (B4, T8, 1 + cm.nq + cm.nv) and sens.shape == (B4, T8, cm.nsensordata)
            final = {k: fused.sim.get(k) for k in STATE}
            hA, hB, pre, hstate, _ = _host_loop(loop.sim, u, w0, T8)
            # the policy default loads the specialised FD kernel (built by build()); the runs with batched rows force the generic one
            assert fused.sim.fd_specialized is (not with_params) and loop.sim.fd_specialized is (not with_params)
            for k in STATE:
                assert np.array_equal(final[k], loop.sim.get(k)), k                          # data ends in the rollout's final state
            cache[key] = dict(A=A.cpu().numpy(), B=Bm.cpu().numpy(), state=state.cpu().numpy(), hA=hA, hB=hB, hstate=hstate, pre=pre, prm=prm)
        return cache[key]

    return get


# ---- 4. the definition, bitwise ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_params", [False, True], ids=["model", "env_params"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_linearize_rollout_equals_host_loop_bitwise(runs, name, dtype, with_params):
    """linearize_rollout == for t: ctrl <- u[:, t]; transition_fd(); step(1): A, B and the states bit for bit (T x B points in one
    launch use another columns-per-job chunk than B points do: the chunking is result-neutral).  With per-environment body_mass /
    actuator_gear rows, two environments with equal states and controls get different A: the rows are used."""
    r = runs(name, dtype, with_params)
    assert np.isfinite(r["A"]).all() and np.isfinite(r["B"]).all()
    assert np.array_equal(r["state"], r["hstate"]), "states differ"
    assert np.array_equal(r["A"], r["hA"]), f"A differs: max |d| {np.abs(r['A'] - r['hA']).max():.3e}"
    assert np.array_equal(r["B"], r["hB"]), f"B differs: max |d| {np.abs(r['B'] - r['hB']).max():.3e}"
    assert np.abs(r["B"]).max() > 0
    if with_params:
        assert np.array_equal(r["pre"][0]["qpos"][0], r["pre"][0]["qpos"][1]) and np.array_equal(r["pre"][0]["ctrl"][0], r["pre"][0]["ctrl"][1])
        assert not np.array_equal(r["A"][0, 0], r["A"][1, 0])
        assert not np.array_equal(r["B"][0, 0], r["B"][1, 0])
    else:
        assert not np.array_equal(r["A"][:, 0], r["A"][:, -1])                              # the trajectory moved


# ---- 5. against the oracle, every point -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_params", [False, True], ids=["model", "env_params"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_every_point_matches_the_oracle(world, runs, name, dtype, with_params):
    """Every point (t, e): an OracleData set to the recorded device qpos, qvel, ctrl and warm start before step t, mjo_transition_fd,
    error relative to max(1, largest entry) as test_transition_fd_matches_oracle measures it."""
    cm, om, mm = world(name)
    r = runs(name, dtype, with_params)
    worst, worst1, n1, ncon = 0.0, 0.0, 0, []
    for e in range(B4):
        ome = env_oracle(cm, **{k: v[e] for k, v in r["prm"].items()}) if with_params else om
        od = mjo.OracleData(ome)
        for t in range(T8):
            p = r["pre"][t]
            od.reset()
            od.qpos[:] = p["qpos"][e]; od.qvel[:] = p["qvel"][e]; od.ctrl[:] = p["ctrl"][e]
            od.qacc_warmstart[:] = p["qacc_warmstart"][e]
            od.forward()                                        # the nominal column's solve: from the recorded warm start
            cn = od.counters()
            ncon.append(cn["ncon"])
            single = name == "humanoid" and cn["solver_niter"] == 1           # one unrefined Newton step (see FD_POINTS_TOL)
            od.qacc_warmstart[:] = p["qacc_warmstart"][e]
            Ao, Bo = od.transition_fd(1e-6, True)
            err = max(np.abs(r["A"][e, t] - Ao).max() / max(1.0, np.abs(Ao).max()), np.abs(r["B"][e, t] - Bo).max() / max(1.0, np.abs(Bo).max()))
            print(f"fd_points {name} {dtype} params={with_params} t={t} e={e} ncon={ncon[-1]} niter={cn['solver_niter']} err={err:.3e}")
            if single:
                worst1, n1 = max(worst1, err), n1 + 1
            else:
                worst = max(worst, err)
    if name == "humanoid":
        assert min(ncon) >= 1, ncon                             # standing: every point is in contact
        assert n1 <= 8, n1                                      # the looser bound covers a few points, not the run
    tol = (FD_POINTS_PARAMS_TOL if with_params else FD_POINTS_TOL)[(name, dtype)]
    tag = "_env_params" if with_params else ""
    if n1:
        measured(f"fd_points{tag}_single_newton_step/{name}/{dtype}", worst1, FD_SINGLE_NEWTON_TOL[(with_params, dtype)], f"(relative; {n1} points)")
    measured(f"fd_points{tag}/{name}/{dtype}", worst, tol, f"(relative; contacts per point {min(ncon)}..{max(ncon)})")


# ---- 6. a control at its ctrlrange bound --------------------------------------------------------------------------------------------------
def test_control_at_the_lower_bound_is_one_sided(world):
    import torch

    cm, om, mm = world("drone2")
    q, v, w = _start_state(cm, om, "drone2", B4)
    u = _table(cm, "drone2", B4, T8, "float64")
    te, ee = 3, 1
    u[ee, te, :] = 0.0                                          # the lower bound of ctrlrange [0, 13]
    w0 = torch.from_numpy(w).to("cuda")
    state, _, A, Bm = linearize_rollout(mm, _make(mm, "float64", q, v, None), u, initial_warmstart=w0)
    st2, _, ws = rollout(mm, _make(mm, "float64", q, v, None), u, initial_warmstart=w0, return_warmstart=True)
    assert torch.equal(state, st2)
    od = mjo.OracleData(om)
    od.qpos[:] = state[ee, te - 1, 1:1 + cm.nq].cpu().numpy(); od.qvel[:] = state[ee, te - 1, 1 + cm.nq:].cpu().numpy()
    od.ctrl[:] = 0.0
    od.qacc_warmstart[:] = ws[ee, te - 1].cpu().numpy()
    Ao, Bo = od.transition_fd(1e-6, True)
    got = Bm[ee, te].cpu().numpy()
    assert np.abs(got - Bo).max() < 1e-5 * max(1.0, np.abs(Bo).max())
    assert np.abs(got).max() > 0


# ---- 7. the points API on its own ---------------------------------------------------------------------------------------------------------
def _ring_sim(world, dtype, B=B4, T=T8, name="humanoid"):
    """A BatchSim a few random steps into a trajectory (non-zero warm start) plus a [T, B, dim] ring with the warm-start column."""
    import torch

    cm, om, mm = world(name)
    sim = BatchSim(DeviceModel(cm), B, dtype=dtype)
    sim.use_torch_stream()
    sim.rollout(3, CTRL_RANDOM, seed=4, ctrl_scale=0.3)
    spec = sim.make_obs_spec(1 | 2 | 8 | 16 | 128)
    ring = torch.full((T, B, spec.dim), float("nan"), device="cuda", dtype=_tdt(dtype))
    u = _table(cm, name, B, T, dtype, seed=9)
    sim.rollout_ctrl(T, u, obs_spec=spec, obs_out_ptr=ring.data_ptr(), obs_every=1)
    sim.sync()
    assert torch.isfinite(ring).all()
    return cm, sim, ring, u


@pytest.mark.parametrize("dtype", DTYPES)
def test_points_api(world, dtype):
    import torch

    cm, sim, ring, u = _ring_sim(world, dtype)
    nq, nv, nu, nx = cm.nq, cm.nv, cm.nu, 2 * cm.nv
    tc = nq + nv + cm.nsensordata
    tv = sim.torch_view
    # [B, n] inputs equal to the data's own arrays == transition_fd()
    A0, B0 = sim.transition_fd(1e-6, True)
    A1, B1 = sim.transition_fd_points(tv("qpos"), tv("qvel"), tv("ctrl"), tv("qacc_warmstart"))
    assert A1.shape == (B4, nx, nx) and B1.shape == (B4, nx, nu) and A1.dtype == torch.float64 and A1.is_cuda
    assert np.array_equal(A1.cpu().numpy(), A0) and np.array_equal(B1.cpu().numpy(), B0)
    assert np.array_equal(ring[-1, :, tc + 1:].double().cpu().numpy(), sim.get("qacc_warmstart"))
    # column views of the ring + an expand-ed control == dense copies
    qv, vv, wv = ring[..., :nq], ring[..., nq:nq + nv], ring[..., tc + 1:]
    ue = u[0, 0].expand(T8, B4, nu)
    assert not qv.is_contiguous() and ue.stride() == (0, 0, 1)
    Av, Bv = sim.transition_fd_points(qv, vv, ue, wv)
    Ad, Bd = sim.transition_fd_points(qv.contiguous(), vv.contiguous(), ue.contiguous(), wv.contiguous())
    assert Av.shape == (T8, B4, nx, nx) and torch.equal(Av, Ad) and torch.equal(Bv, Bd)
    # a [B, T, nu] control read through its strides
    ub = u.permute(1, 0, 2)
    Ap, Bp = sim.transition_fd_points(qv, vv, ub, wv)
    Aq, Bq = sim.transition_fd_points(qv, vv, ub.contiguous(), wv)
    assert torch.equal(Ap, Aq) and torch.equal(Bp, Bq) and not torch.equal(Bp, Bv)
    # no warm start == zeros
    An, Bn = sim.transition_fd_points(qv, vv, ub)
    Az, Bz = sim.transition_fd_points(qv, vv, ub, torch.zeros_like(wv))
    assert torch.equal(An, Az) and torch.equal(Bn, Bz) and not torch.equal(An, Ap)
    # out= is filled in place
    oA = torch.full((T8, B4, nx, nx), float("nan"), device="cuda", dtype=torch.float64)
    oB = torch.full((T8, B4, nx, nu), float("nan"), device="cuda", dtype=torch.float64)
    rA, rB = sim.transition_fd_points(qv, vv, ub, wv, out=(oA, oB))
    assert rA is oA and rB is oB and torch.equal(oA, Ap) and torch.equal(oB, Bp)
    # one-sided differences: eps and centered are honoured
    Af, _ = sim.transition_fd_points(qv, vv, ub, wv, centered=False)
    assert not torch.equal(Af, Ap) and torch.isfinite(Af).all()


# ---- 8. slabs -----------------------------------------------------------------------------------------------------------------------------
def test_slab_size_does_not_change_the_result(world, monkeypatch):
    """T x B = 32 humanoid points under a budget of 12 points' scratch run in 3 slabs: bitwise the one-slab result."""
    import torch

    cm, sim, ring, u = _ring_sim(world, "float32")
    nq, nv = cm.nq, cm.nv
    tc = nq + nv + cm.nsensordata
    args = (ring[..., :nq], ring[..., nq:nq + nv], u.permute(1, 0, 2), ring[..., tc + 1:])
    per_point = (1 + 2 * (2 * nv + cm.nu)) * (nq + nv) * 8
    monkeypatch.delenv("MJB_FD_SLAB_BYTES", raising=False)
    A1, B1 = sim.transition_fd_points(*args)
    assert sim.fd_points_slabs() == 1
    monkeypatch.setenv("MJB_FD_SLAB_BYTES", str(12 * per_point + 100))
    A3, B3 = sim.transition_fd_points(*args)
    assert sim.fd_points_slabs() == 3
    monkeypatch.setenv("MJB_FD_SLAB_BYTES", "1")               # one point exceeds the budget: one point per slab
    A32, B32 = sim.transition_fd_points(*args)
    assert sim.fd_points_slabs() == 32
    sim.sync()
    assert torch.equal(A1, A3) and torch.equal(B1, B3) and torch.equal(A1, A32) and torch.equal(B1, B32)
    assert torch.isfinite(A1).all()


# ---- 9. the data is left alone; rejections --------------------------------------------------------------------------------------------------
def test_leaves_the_data_alone_and_rejects_bad_arguments(world):
    import torch

    from tests.test_gpu_rollout_ctrl import _hip_runtime

    cm, sim, ring, u = _ring_sim(world, "float32", name="cartpole")
    nq, nv, nu, nx = cm.nq, cm.nv, cm.nu, 2 * cm.nv
    tc = nq + nv + cm.nsensordata
    qv, vv, wv, ub = ring[..., :nq], ring[..., nq:nq + nv], ring[..., tc + 1:], u.permute(1, 0, 2)
    L = load_library()

    def snap():
        sim.sync_to_host()
        return [sim.get(k) for k in STATE] + [np.array([float(sim.host_view("engine_flags")[0]), sim.engine_flags()])]

    before = snap()
    A, Bm = sim.transition_fd_points(qv, vv, ub, wv)
    sim.sync()
    for k, a, b in zip(STATE + ("flags",), before, snap()):
        assert np.array_equal(a, b), k
    oA, oB = torch.empty_like(A), torch.empty_like(Bm)
    dim = ring.shape[-1]

    def raw(q=None, qs=None, A_=None, B_=None, T=T8, ws=None, eps=1e-6):
        q = qv.data_ptr() if q is None else q
        qs = (B4 * dim, dim) if qs is None else qs
        return L.mjb_transition_fd_points(sim.ptr, T, ctypes.c_void_p(q), qs[0], qs[1], ctypes.c_void_p(vv.data_ptr()), B4 * dim, dim,
                                          ctypes.c_void_p(ub.data_ptr()), ub.stride(0), ub.stride(1),
                                          ctypes.c_void_p(wv.data_ptr() if ws is None else ws), B4 * dim, dim, eps, 1,
                                          ctypes.c_void_p(oA.data_ptr() if A_ is None else A_), ctypes.c_void_p(oB.data_ptr() if B_ is None else B_))

    host = np.zeros((T8, B4, nq), dtype=np.float32)             # pageable host memory
    hostA = np.zeros((T8, B4, nx, nx))
    assert raw(q=host.ctypes.data, qs=(B4 * nq, nq)) == -1
    assert raw(A_=hostA.ctypes.data) == -1
    assert raw(qs=(-1, dim)) == -1 and raw(qs=(B4 * dim, -dim)) == -1          # negative strides
    assert raw(q=0) == -1 and raw(A_=0) == -1 and raw(B_=0) == -1                # NULL where the width is not zero
    assert raw(T=0) == -1 and raw(eps=0.0) == -1
    # the allocation one element short: the extent is measured against what hipMemGetAddressRange reports behind the pointer
    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    assert _hip_runtime().hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(qv.data_ptr())) == 0
    n_ok = (base.value + size.value - qv.data_ptr()) // 4       # float32 elements from qpos[0, 0, 0] to the end of its block
    assert n_ok >= T8 * B4 * dim - (dim - nq)
    assert raw(T=2, qs=(n_ok - nq + 1, 0)) == -1                # highest element one past the end
    assert _hip_runtime().hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(oA.data_ptr())) == 0
    a_ok = (base.value + size.value - oA.data_ptr()) // 8
    assert raw(A_=oA.data_ptr() + 8 * (a_ok - T8 * B4 * nx * nx + 1)) == -1     # the A blocks would end one element past the allocation
    # the Python front: wrong device, dtype, shape, disagreeing T
    for bad in ((qv.cpu(), vv, ub, wv), (qv.double(), vv, ub, wv), (qv[..., :1], vv, ub, wv), (qv[:, :2], vv, ub, wv), (qv[:3], vv, ub, wv),
                (host, vv, ub, wv), (qv, vv, ub, wv.cpu())):
        with pytest.raises(ConfigError):
            sim.transition_fd_points(*bad)
    with pytest.raises(ConfigError):
        sim.transition_fd_points(qv, vv, ub, wv, out=(oA.float(), oB))
    with pytest.raises(TemplateError):
        sim.transition_fd_points(qv, vv, ub, wv, eps=0.0)       # MJB_ERR_ARG -> the package's exception
    sim.sync()
    for k, a, b in zip(STATE + ("flags",), before, snap()):
        assert np.array_equal(a, b), k
    A2, B2 = sim.transition_fd_points(qv, vv, ub, wv)           # a following valid call succeeds, with the same result
    sim.sync()
    torch.cuda.synchronize()
    assert torch.equal(A2, A) and torch.equal(B2, Bm)


# ---- 10. the ring column on the device ------------------------------------------------------------------------------------------------------
# the ticket scheduler and the two-wave kernel exist for float32 data only (float64 data always take the static map, one wave)
RING_SHAPES = [("cartpole", "float32", "static", 64), ("cartpole", "float64", "static", 64), ("humanoid", "float64", "static", 64),
               ("humanoid", "float32", "static", 64), ("humanoid", "float32", "tickets", 256), ("humanoid", "float32", "two_wave", 512)]


@pytest.mark.parametrize("name,dtype,shape,B", RING_SHAPES)
def test_rollout_warmstart_column_equals_stepwise(world, name, dtype, shape, B, monkeypatch):
    """rollout(return_warmstart=True)[2][:, t] == data.qacc_warmstart after t + 1 single steps, bitwise, under the static map, the
    ticket scheduler and the two-wave kernel; rollout without the flag returns what the per-step loop gives, and the same state."""
    import torch

    cm, om, mm = world(name)
    T = 20
    monkeypatch.setenv("MJB_CHUNK_STEPS", "7" if shape == "tickets" else "0")
    monkeypatch.setenv("MJB_TWO_WAVE", "1" if shape == "two_wave" else "0")
    q, v, w = _start_state(cm, om, name, B)
    u = _table(cm, name, B, T, dtype, seed=2)
    w0 = torch.from_numpy(w).to(device="cuda", dtype=_tdt(dtype))
    d_ws, d_plain, d_loop = (_make(mm, dtype, q, v, None) for _ in range(3))
    state, sens, ws = rollout(mm, d_ws, u, initial_warmstart=w0, return_warmstart=True)
    info = d_ws.sim.schedule_info()
    assert info["launch_steps"] == T and info["map"] == ("tickets" if shape == "tickets" else "static")
    assert info["waves_per_env"] == (2 if shape == "two_wave" else 1)
    out = rollout(mm, d_plain, u, initial_warmstart=w0)
    assert len(out) == 2 and ws.shape == (B, T, cm.nv)
    assert torch.equal(out[0], state) and torch.equal(out[1], sens)
    _, _, _, hstate, hws = _host_loop_steps(d_loop.sim, u, w0, T)
    assert np.array_equal(state.cpu().numpy(), hstate)
    assert np.array_equal(ws.cpu().numpy(), hws)
    assert np.abs(hws).max() > 0
    for k in STATE:
        assert np.array_equal(d_ws.sim.get(k), d_loop.sim.get(k)), k
        assert np.array_equal(d_plain.sim.get(k), d_loop.sim.get(k)), k
    assert d_ws.sim.engine_flags() & 8 == 0


def _host_loop_steps(sim, u, w0, T):
    """_host_loop without the linearisations: T x (write ctrl, step(1))."""
    import torch

    sim.use_torch_stream()
    sim.torch_view("qacc_warmstart").copy_(w0)
    ctrl, rows, ws_after = sim.torch_view("ctrl"), [], []
    for t in range(T):
        ctrl.copy_(u[:, t])
        sim.step(1)
        rows.append(torch.cat([sim.torch_view("time").to(u.dtype), sim.torch_view("qpos"), sim.torch_view("qvel")], dim=1).clone())
        ws_after.append(sim.torch_view("qacc_warmstart").clone())
    sim.sync()
    return None, None, None, torch.stack(rows, dim=1).cpu().numpy(), torch.stack(ws_after, dim=1).cpu().numpy()
