"""``mjb_traj_cost`` / ``mjb_traj_select`` on the GPU (``mt.trajectory_cost`` / ``mt.select_candidates``).

The yardstick is never the kernel: the numpy restatement of ``tests/traj_common.py`` in long double is the truth, the same restatement
in float64 measures what float64 arithmetic alone loses, and every bound is 8 x that measure (floor 1e-13); a float32 output may differ
from the truth's float32 rounding by one float32 ulp.  Both values of every comparison go through ``tests.conftest.measured``."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import lqr_common as lc
from tests import traj_common as tc
from tests.conftest import MODELS, measured

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch

    from mujoco_template_amd import mj

    models, datas = {}, {}

    def get(name, batch=1, dtype="float64"):
        if name not in models:
            models[name] = mj.MjModel.from_xml_path(MODELS[name])
        key = (name, batch, dtype)
        if key not in datas:
            datas[key] = mj.MjData(models[name], batch=batch, dtype=dtype)
        return models[name], datas[key]

    return torch, get


def _dev(torch, x, dtype=None):
    x = np.array(x, order="C")                               # a writable copy (broadcast views are not)
    return torch.as_tensor(x, dtype=dtype or (torch.float32 if x.dtype == np.float32 else torch.float64), device="cuda")


def _np(res):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in res._asdict().items()}


def gpu_cost(torch, data, case, **kw):
    """``mt.trajectory_cost`` on a ``traj_common.generate``-style case: x [B, T+1, nq+nv] -> state [B, T, 1+nq+nv] and initial_state."""
    import mujoco_template_amd as mt

    x = case["x"]
    B = x.shape[0]
    withtime = np.concatenate([np.zeros(x.shape[:2] + (1,), dtype=x.dtype), x], axis=2)
    args = dict(initial_state=_dev(torch, withtime[:, 0]), Q=_dev(torch, case["Q"]), R=_dev(torch, case["R"]), Qf=_dev(torch, case["Qf"]),
                x_ref=_dev(torch, case["x_ref"]), u_ref=None if case.get("u_ref") is None else _dev(torch, np.broadcast_to(case["u_ref"], case["u"].shape)))
    args.update(kw)
    res = mt.trajectory_cost(data, _dev(torch, withtime[:, 1:]), _dev(torch, case["u"]), **args)
    assert res.cost.shape == (B,) and res.cost_t.shape == (B, x.shape[1])
    return _np(res)


def restated(cm, case, dtype):
    return tc.restate_cost(tc.joint_table(cm), case["nq"], case["nv"], case["nu"], case["x"], case["u"], case["x_ref"], case.get("u_ref"),
                           case["Q"], case["R"], case["Qf"], dtype)


def compare(tag, got, truth, f64, keys=tc.COST_OUTPUTS):
    for key in keys:
        mine, numpy64 = lc.rel_err(got[key], truth[key]), lc.rel_err(f64[key], truth[key])
        print(f"{tag} {key}: kernel {mine:.3e}  float64 numpy {numpy64:.3e}  bound {lc.bound(numpy64):.3e}")
        measured(f"traj/{tag}/{key}", mine, lc.bound(numpy64), f"(float64 numpy restatement: {numpy64:.3e})")


# ---- 1. on real rollouts, against the restatement ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rollouts(ctx):
    """The two rollouts (cart-pole float64 through linearize_rollout, T = 7, B = 3; humanoid float32 through rollout, T = 5, B = 2,
    random controls within ctrlrange), made once: the returned state views, and per cost layout the case with both restatements."""
    import mujoco_template_amd as mt

    torch, get = ctx
    out = {}
    for name, T, B, dtype, lin in (("cartpole", 7, 3, "float64", True), ("humanoid", 5, 2, "float32", False)):
        model, data = get(name, B, dtype)
        cm = data.sim.model.compiled
        nq, nv, nu = int(cm.nq), int(cm.nv), int(cm.nu)
        rng = np.random.default_rng(11)
        lo, hi = np.asarray(cm.actuator_ctrlrange, dtype=np.float64).reshape(nu, 2).T
        tdt = torch.float32 if dtype == "float32" else torch.float64
        u = _dev(torch, rng.uniform(lo, hi, size=(B, T, nu))).to(tdt)
        x0 = np.zeros((B, 1 + nq + nv))
        x0[:, 1:1 + nq] = np.asarray(cm.qpos0, dtype=np.float64)
        x0[:, 1 + nq:] = 0.1 * rng.normal(size=(B, nv))
        if name == "cartpole":
            x0[:, 2] = 0.3
        x0 = _dev(torch, x0)
        state = (mt.linearize_rollout(model, data, u, initial_state=x0) if lin else mt.rollout(model, data, u, initial_state=x0))[0]
        assert state.dtype == tdt and state.shape == (B, T, 1 + nq + nv)
        x0s = x0.to(tdt)                                          # the start state as the rollout saw it
        x = np.concatenate([x0s[:, None, 1:].cpu().numpy(), state[..., 1:].cpu().numpy()], axis=1)
        cases = {}
        for per_point in (False, True):
            case = tc.generate(cm, T, B, seed=12, per_point_cost=per_point)
            # references around the rolled-out states: scalars nearby, every free joint's reference the state's quaternion turned back
            # by the generator's 0.05 .. 2.5 rad (the generator's x is its x_ref turned by that rotation; swap the roles)
            gx, gref = case["x"], case["x_ref"]
            ref = x.astype(np.float64) + (gref - gx)
            jt, jq, _ = tc.joint_table(cm)
            for j in np.flatnonzero(jt == tc.JNT_FREE):
                qa = int(jq[j])
                for e in range(B):
                    for t in range(T + 1):
                        rel = tc._quat_mul(np.array([1, -1, -1, -1.0]) * gx[e, t, qa + 3:qa + 7], gref[e, t, qa + 3:qa + 7])      # x -> ref in the generator
                        ref[e, t, qa + 3:qa + 7] = tc._quat_mul(x[e, t, qa + 3:qa + 7].astype(np.float64), rel)
            ref[0, 1, :nq] = x[0, 1, :nq]
            case.update(x=x, x_ref=ref, u=u.cpu().numpy())
            cases[per_point] = (case, restated(cm, case, np.longdouble), restated(cm, case, np.float64))
        out[name] = (data, cm, state, u, x0, cases)
    return out


@pytest.mark.parametrize("per_point", [False, True], ids=["Q_broadcast", "Q_per_point"])
@pytest.mark.parametrize("name", ["cartpole", "humanoid"])
def test_cost_on_real_rollouts_matches_the_restatement(ctx, rollouts, name, per_point):
    """The state is read in place from the views ``linearize_rollout`` / ``rollout`` returned."""
    import mujoco_template_amd as mt

    torch, _ = ctx
    data, cm, state, u, x0, cases = rollouts[name]
    case, truth, f64 = cases[per_point]
    nv = case["nv"]
    ang = np.linalg.norm(truth["dx"][..., 3:6].astype(np.float64), axis=-1) if name == "humanoid" else None
    if ang is not None:
        rot = np.delete(ang.reshape(-1), 1)                      # all but the point with qpos == qref
        assert rot.min() > 0.04 and rot.max() < 2.6
    res = mt.trajectory_cost(data, state, u, initial_state=x0, Q=_dev(torch, case["Q"]), R=_dev(torch, case["R"]), Qf=_dev(torch, case["Qf"]),
                             x_ref=_dev(torch, case["x_ref"]), u_ref=_dev(torch, case["u_ref"]))
    assert res.lx.shape == truth["lx"].shape and res.lx.stride(1) > res.lx.stride(0)          # the permuted [T, B, nx] block lqr_backward reads in place
    got = _np(res)
    compare(f"gpu/{name}/{'pp' if per_point else 'bc'}", got, truth, f64)
    assert np.array_equal(truth["dx"][0, 1, :nv], np.zeros(nv))
    only = mt.trajectory_cost(data, state, u, initial_state=x0, Q=_dev(torch, case["Q"]), R=_dev(torch, case["R"]), Qf=_dev(torch, case["Qf"]),
                              x_ref=_dev(torch, case["x_ref"]), u_ref=_dev(torch, case["u_ref"]), gradients=False)
    assert only.lx is None and only.VxT is None and torch.equal(only.cost, res.cost) and torch.equal(only.cost_t, res.cost_t)


def test_defaults_are_qpos0_and_zero(ctx, rollouts):
    """x_ref = None is the model's qpos0 at zero velocity, u_ref = None is zero; a [T, nu] control is shared by every trajectory."""
    import mujoco_template_amd as mt

    torch, _ = ctx
    data, cm, state, u, x0, cases = rollouts["humanoid"]
    case = dict(cases[False][0])
    nq, nv = case["nq"], case["nv"]
    Q, R, Qf = (_dev(torch, case[k]) for k in ("Q", "R", "Qf"))
    got = _np(mt.trajectory_cost(data, state, u[0], initial_state=x0, Q=Q, R=R, Qf=Qf))
    case.update(x_ref=np.concatenate([np.asarray(cm.qpos0, dtype=np.float64), np.zeros(nv)]), u_ref=None, u=np.broadcast_to(case["u"][0], case["u"].shape))
    compare("gpu/humanoid/defaults", got, restated(cm, case, np.longdouble), restated(cm, case, np.float64))


# ---- 3. exact integers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_point", [False, True], ids=["Q_broadcast", "Q_per_point"])
def test_exact_integers_are_bit_equal_to_numpy(ctx, per_point):
    torch, get = ctx
    _, data = get("cartpole")
    cm = data.sim.model.compiled
    T, B, nq, nv, nu, nx = 5, 3, 2, 2, 1, 4
    rng = np.random.default_rng(3)
    lead = (B, T) if per_point else ()
    scale = np.array([[1, 10, 100, 1000], [10, 1, 1000, 100], [100, 1000, 1, 10], [1000, 100, 10, 1]], dtype=np.float64)
    G = rng.integers(1, 10, size=lead + (nx, nx)).astype(np.float64)
    Gf = rng.integers(1, 10, size=(nx, nx)).astype(np.float64)
    case = {"x": rng.integers(-9, 10, size=(B, T + 1, nq + nv)).astype(np.float64), "u": rng.integers(-9, 10, size=(B, T, nu)).astype(np.float64),
            "x_ref": rng.integers(-4, 5, size=(B, T + 1, nq + nv)).astype(np.float64), "u_ref": rng.integers(-4, 5, size=(B, T, nu)).astype(np.float64),
            "Q": (G + np.swapaxes(G, -1, -2)) * scale, "R": rng.integers(1, 10, size=lead + (nu, nu)).astype(np.float64), "Qf": (Gf + Gf.T) * scale,
            "nq": nq, "nv": nv, "nu": nu}
    ref = restated(cm, case, np.float64)
    got = gpu_cost(torch, data, case)
    for key in tc.COST_OUTPUTS:
        assert np.array_equal(got[key], ref[key]), key


# ---- 4. position independence, 5. non-finite input -------------------------------------------------------------------------------------------
def test_a_trajectory_gives_the_same_bits_anywhere(ctx):
    torch, get = ctx
    _, data = get("humanoid", 2, "float32")
    cm = data.sim.model.compiled
    big = tc.generate(cm, 5, 7, seed=4, per_point_cost=True)
    one = {k: (v[5:6] if isinstance(v, np.ndarray) and v.ndim >= 3 else v) for k, v in big.items()}
    a, b = gpu_cost(torch, data, big), gpu_cost(torch, data, one)
    for key in tc.COST_OUTPUTS:
        assert np.array_equal(a[key][5:6], b[key]), key
    again = gpu_cost(torch, data, big)                            # and run to run
    for key in tc.COST_OUTPUTS:
        assert np.array_equal(a[key], again[key]), key


def test_a_nan_state_costs_inf_and_touches_nothing_else(ctx):
    torch, get = ctx
    _, data = get("humanoid", 2, "float32")
    cm = data.sim.model.compiled
    case = tc.generate(cm, 5, 3, seed=5, state_dtype=np.float32)
    clean = gpu_cost(torch, data, case)
    case["x"][1, 3, 9] = np.nan
    got = gpu_cost(torch, data, case)
    assert got["cost"][1] == np.inf and np.isfinite(got["cost"][[0, 2]]).all()
    for key in tc.COST_OUTPUTS:
        assert np.array_equal(got[key][[0, 2]], clean[key][[0, 2]]), key


# ---- 6. select -----------------------------------------------------------------------------------------------------------------------------------
def test_argmin_ties_non_finite_costs_and_the_copy(ctx):
    import mujoco_template_amd as mt

    torch, get = ctx
    _, data = get("cartpole")
    rng = np.random.default_rng(6)
    G, n, T, nu = 4, 9, 3, 2
    cand = rng.normal(size=(G, n, T, nu))
    cost = rng.integers(3, 9, size=(G, n)).astype(np.float64)
    cost[0, [6, 2, 4]] = 1.0
    cost[1, 0], cost[1, 1], cost[1, 5] = -np.inf, np.nan, 2.0
    cost[2, :] = [np.nan, np.inf, -np.inf] * 3
    cost[3, 8] = -5.0
    for cdt, odt in ((np.float64, np.float64), (np.float64, np.float32), (np.float32, np.float32), (np.float32, np.float64)):
        c = cand.astype(cdt)
        out = torch.full((G, T, nu), -77.0, dtype=torch.float32 if odt == np.float32 else torch.float64, device="cuda")
        res = mt.select_candidates(data, _dev(torch, cost), _dev(torch, c), out=out)
        assert res.u is out and res.weights is None
        assert res.best.tolist() == [2, 5, -1, 8] and res.best_cost.tolist() == [1.0, 2.0, np.inf, -5.0]
        u = out.cpu().numpy()
        for g, b in ((0, 2), (1, 5), (3, 8)):
            assert np.array_equal(u[g], c[g, b].astype(odt)), (cdt, odt, g)
        assert (u[2] == -77.0).all()                              # unwritten: the caller's nominal is kept
    wide = rng.normal(size=(1, 3, 150, 3))                        # T * nu = 450: 29 chunks of 16 elements, the last one partial
    res = mt.select_candidates(data, _dev(torch, np.array([[2.0, 1.0, 3.0]])), _dev(torch, wide))
    assert np.array_equal(res.u.cpu().numpy()[0], wide[0, 1])


@pytest.mark.parametrize("ncand", [1, 5, 64, 1000])
def test_softmin_matches_the_restatement(ctx, ncand):
    import mujoco_template_amd as mt

    torch, get = ctx
    _, data = get("cartpole")
    rng = np.random.default_rng(7)
    G, T, nu = 2, 4, 3
    cand = rng.normal(size=(G, ncand, T, nu))
    cost = rng.uniform(1.0, 3.0, size=(G, ncand))
    cost[1] = 1.0 + 1e6 * np.arange(ncand)[rng.permutation(ncand)]
    if ncand > 1:
        cost[0, ncand // 2] = np.inf
    temperature = 0.7
    truth, f64 = tc.restate_select(cost, cand, "softmin", temperature, np.longdouble), tc.restate_select(cost, cand, "softmin", temperature, np.float64)
    res = mt.select_candidates(data, _dev(torch, cost), _dev(torch, cand), mode="softmin", temperature=temperature)
    got = {"u": res.u.cpu().numpy(), "weights": res.weights.cpu().numpy()}
    assert np.array_equal(res.best.cpu().numpy(), truth["best"]) and np.array_equal(res.best_cost.cpu().numpy(), cost[np.arange(G), truth["best"]])
    for key in ("weights", "u"):
        mine, numpy64 = lc.rel_err(got[key], truth[key]), lc.rel_err(f64[key], truth[key])
        print(f"softmin n={ncand} {key}: kernel {mine:.3e}  float64 numpy {numpy64:.3e}")
        measured(f"traj/gpu/softmin/{ncand}/{key}", mine, lc.bound(numpy64))
    if ncand > 1:
        assert got["weights"][0, ncand // 2] == 0.0
    assert got["weights"][1].max() == 1.0 and np.count_nonzero(got["weights"][1]) == 1
    assert np.array_equal(got["u"][1], cand[1, truth["best"][1]])
    c32 = cand.astype(np.float32)
    r32 = mt.select_candidates(data, _dev(torch, cost), _dev(torch, c32), mode="softmin", temperature=temperature)
    assert r32.u.dtype == torch.float32
    ulps = tc.float32_ulp_error(r32.u.cpu().numpy(), tc.restate_select(cost, c32, "softmin", temperature, np.longdouble)["u"])
    measured(f"traj/gpu/softmin/{ncand}/u_f32_ulps", ulps, 1.0)
    out = torch.full((1, T, nu), -77.0, dtype=torch.float64, device="cuda")
    none = mt.select_candidates(data, _dev(torch, np.full((1, ncand), np.nan)), _dev(torch, cand[:1]), mode="softmin", temperature=temperature, out=out)
    assert int(none.best[0]) == -1 and float(none.best_cost[0]) == np.inf and bool((out == -77.0).all()) and bool((none.weights == 0).all())


# ---- 7. the chain of an iLQR iteration, on a side stream -------------------------------------------------------------------------------------
def test_ilqr_chain_on_a_side_stream_needs_no_synchronise(ctx):
    """trajectory_cost -> lqr_backward -> lqr_candidates -> rollout -> trajectory_cost -> select_candidates(out=u), enqueued back to back
    on a non-default stream, equals bitwise the same chain with a synchronise after every call; and u is the candidate that a host
    argmin over the restatement's costs picks."""
    import mujoco_template_amd as mt

    torch, get = ctx
    model, nominal = get("cartpole", 1, "float64")
    T, na = 7, 4
    _, search = get("cartpole", na, "float64")
    cm = nominal.sim.model.compiled
    nq, nv, nu, nx = 2, 2, 1, 4
    x0 = torch.zeros(1 + nq + nv, dtype=torch.float64, device="cuda"); x0[2] = 0.3
    Q = torch.diag(torch.tensor([0.5, 10.0, 0.05, 0.1], dtype=torch.float64, device="cuda"))
    R = 0.01 * torch.eye(nu, dtype=torch.float64, device="cuda")
    Qf = 20 * Q
    x_ref = torch.zeros(nq + nv, dtype=torch.float64, device="cuda")
    alphas = torch.tensor([1.0, 0.5, 0.25, 0.0], dtype=torch.float64, device="cuda")

    def chain(sync):
        wait = torch.cuda.synchronize if sync else (lambda: None)
        u = 0.1 * torch.ones((1, T, nu), dtype=torch.float64, device="cuda")
        state, _, A, Bm = mt.linearize_rollout(model, nominal, u, initial_state=x0); wait()
        c = mt.trajectory_cost(nominal, state, u, initial_state=x0, Q=Q, R=R, Qf=Qf, x_ref=x_ref); wait()
        sol = mt.lqr_backward(nominal, A, Bm, lx=c.lx, lu=c.lu, lxx=Q, luu=R, VxT=c.VxT, VxxT=Qf, mu=1e-6); wait()
        cand = mt.lqr_candidates(nominal, A, Bm, sol.k, sol.K, u, alphas, lo=-4.0, hi=4.0); wait()
        st, _ = mt.rollout(model, search, cand[0], initial_state=x0); wait()
        cc = mt.trajectory_cost(search, st, cand[0], initial_state=x0, Q=Q, R=R, Qf=Qf, x_ref=x_ref, gradients=False); wait()
        sel = mt.select_candidates(nominal, cc.cost[None], cand, out=u); wait()
        assert sel.u is u
        return u, c.cost.clone(), cc.cost.clone(), cand.clone(), st.clone(), sel.best.clone(), sel.best_cost.clone(), sol.status.clone()

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fast = chain(False)
    side.synchronize()
    with torch.cuda.stream(side):
        slow = chain(True)
    torch.cuda.synchronize()
    for a, b in zip(fast, slow):
        assert torch.equal(a, b)
    u, c0, cc, cand, st, best, best_cost, status = fast
    assert int(status[0]) == 0 and torch.isfinite(cc).all()
    # the host's choice: the restatement's costs of the four candidate rollouts, argmin
    x = np.concatenate([np.broadcast_to(x0[1:].cpu().numpy(), (na, 1, nq + nv)), st[..., 1:].cpu().numpy()], axis=1)
    case = {"x": x, "u": cand[0].cpu().numpy(), "x_ref": x_ref.cpu().numpy(), "u_ref": None, "Q": Q.cpu().numpy(), "R": R.cpu().numpy(), "Qf": Qf.cpu().numpy(),
            "nq": nq, "nv": nv, "nu": nu}
    truth, f64 = restated(cm, case, np.longdouble), restated(cm, case, np.float64)
    compare("gpu/chain/candidates", {"cost": cc.cpu().numpy()}, truth, f64, keys=("cost",))
    pick = int(np.argmin(truth["cost"]))
    assert int(best[0]) == pick and float(best_cost[0]) == float(cc[pick])
    assert torch.equal(u[0], cand[0, pick])
    assert float(cc[pick]) <= float(c0[0])                        # alpha = 0 is the nominal itself: the choice never raises the cost


# ---- 8. argument checks ------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_outputs_untouched(ctx):
    import mujoco_template_amd as mt
    from mujoco_template_amd.exceptions import ConfigError, TemplateError

    torch, get = ctx
    _, data = get("cartpole")
    sim = data.sim
    T, B, nq, nv, nu, nx = 3, 2, 2, 2, 1, 4
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    state, ctrl, x0, xref, Q, R = z(T, B, 1 + nq + nv), z(T, B, nu), z(B, 1 + nq + nv), z(nq + nv), torch.eye(nx, dtype=torch.float64, device="cuda"), torch.eye(nu, dtype=torch.float64, device="cuda")
    outs = {"cost": torch.full((B,), 7.0, dtype=torch.float64, device="cuda"), "cost_t": torch.full((B, T + 1), 7.0, dtype=torch.float64, device="cuda"),
            "lx": torch.full((T, B, nx), 7.0, dtype=torch.float64, device="cuda"), "lu": torch.full((T, B, nu), 7.0, dtype=torch.float64, device="cuda"),
            "VxT": torch.full((B, nx), 7.0, dtype=torch.float64, device="cuda")}
    host = np.zeros(T * B * (1 + nq + nv))
    dim = 1 + nq + nv

    def call(**override):
        arrays = {"qpos0": (x0.data_ptr() + 8, 0, dim, 1), "qvel0": (x0.data_ptr() + 8 * (1 + nq), 0, dim, 1),
                  "qpos": (state.data_ptr() + 8, B * dim, dim, 1), "qvel": (state.data_ptr() + 8 * (1 + nq), B * dim, dim, 1),
                  "ctrl": (ctrl.data_ptr(), B * nu, nu, 1), "qref": (xref.data_ptr(), 0, 0), "vref": (xref.data_ptr() + 8 * nq, 0, 0), "uref": (0, 0, 0),
                  "Q": (Q.data_ptr(), 0, 0), "R": (R.data_ptr(), 0, 0), "Qf": (Q.data_ptr(), 0, 0)}
        sizes = override.pop("sizes", {"T": T, "batch": B})
        arrays.update(override)
        sim.traj_cost(sizes, arrays, {k: v.data_ptr() for k, v in outs.items()})

    call()                                                       # the well-formed call goes through
    torch.cuda.synchronize()
    assert outs["cost"].tolist() == [0.0, 0.0]
    for v in outs.values():
        v.fill_(7)
    from tests.test_gpu_rollout_ctrl import _hip_runtime

    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    assert _hip_runtime().hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(ctrl.data_ptr())) == 0
    short = base.value + size.value - 8 * (T * B * nu) + 8        # a control block that ends one element past its allocation
    call(ctrl=(short - 8, B * nu, nu, 1))                        # ending exactly at the end of the block: accepted
    torch.cuda.synchronize()
    for v in outs.values():
        v.fill_(7)
    bad = [("not device-accessible", dict(qpos=(host.ctypes.data + 8, B * dim, dim, 1))), ("beyond its allocation", dict(ctrl=(short, B * nu, nu, 1))),
           ("strides must be", dict(qvel=(state.data_ptr() + 8 * (1 + nq), -1, dim, 1))), ("T must be", dict(sizes={"T": 0, "batch": B})),
           ("qref is NULL", dict(qref=(0, 0, 0))), ("share one dtype", dict(qvel0=(x0.data_ptr() + 8 * (1 + nq), 0, dim, 0)))]
    for msg, kw in bad:
        with pytest.raises((ConfigError, TemplateError), match=msg):
            call(**kw)
    with pytest.raises(ConfigError, match="on cuda"):            # the tensor interface: a host tensor, a wrong shape
        mt.trajectory_cost(data, state.permute(1, 0, 2).cpu(), ctrl.permute(1, 0, 2), initial_state=x0, Q=Q, R=R, Qf=Q)
    with pytest.raises(ConfigError, match="Qf must be"):
        mt.trajectory_cost(data, state.permute(1, 0, 2), ctrl.permute(1, 0, 2), initial_state=x0, Q=Q, R=R, Qf=R)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == 7).all()), k

    # nu > 64: a model with 65 actuators is refused before anything is launched
    from mujoco_template_amd import mj
    from tests.conftest import chain_xml

    xml = chain_xml(4).replace("</actuator>", "".join(f'<motor name="x{k}" joint="j{k % 4}"/>' for k in range(64)) + "</actuator>")
    wide = mj.MjData(mj.MjModel.from_xml_string(xml), batch=1, dtype="float64")
    wnu = int(wide.sim.model.compiled.nu)
    assert wnu == 65
    cost = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises((ConfigError, TemplateError), match="nu must lie in"):
        mt.trajectory_cost(wide, z(1, 2, 1 + 8), z(1, 2, wnu), initial_state=z(1 + 8), Q=torch.eye(8, dtype=torch.float64, device="cuda"),
                           R=torch.eye(wnu, dtype=torch.float64, device="cuda"), Qf=torch.eye(8, dtype=torch.float64, device="cuda"))
    assert float(cost[0]) == 7.0

    # select: temperature <= 0, a host tensor, a cost one element too short - u_out, best, weights untouched
    G, n = 2, 4
    cand, c, u = z(G, n, T, nu), z(G, n), torch.full((G, T, nu), 7.0, dtype=torch.float64, device="cuda")
    best, bc, w = torch.full((G,), 7, dtype=torch.int32, device="cuda"), torch.full((G,), 7.0, dtype=torch.float64, device="cuda"), torch.full((G, n), 7.0, dtype=torch.float64, device="cuda")

    def sel(temperature=0.5, **override):
        ptrs = {"cost": c.data_ptr(), "cand": cand.data_ptr(), "u_out": u.data_ptr(), "best": best.data_ptr(), "best_cost": bc.data_ptr(), "weights": w.data_ptr()}
        ptrs.update(override)
        sim.traj_select({"nprob": G, "ncand": n, "T": T, "nu": nu, "mode": 1, "cand_dtype": 1, "out_dtype": 1, "temperature": temperature}, ptrs)

    assert _hip_runtime().hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(c.data_ptr())) == 0
    end = base.value + size.value
    for msg, kw in (("temperature must be", dict(temperature=0.0)), ("temperature must be", dict(temperature=-1.0)),
                    ("not device-accessible", dict(cand=host.ctypes.data)), ("beyond its allocation", dict(cost=end - 8 * (G * n) + 8)),
                    ("u_out is NULL", dict(u_out=0))):
        with pytest.raises((ConfigError, TemplateError), match=msg):
            sel(**kw)
    with pytest.raises(ConfigError, match="needs a temperature"):
        mt.select_candidates(data, c, cand, mode="softmin")
    with pytest.raises(ConfigError, match="temperature must be"):
        mt.select_candidates(data, c, cand, mode="softmin", temperature=0.0, out=u)
    torch.cuda.synchronize()
    for v in (u, best, bc, w):
        assert bool((v == 7).all())
    sel()                                                        # and the well-formed call goes through
    torch.cuda.synchronize()
    assert best.tolist() == [0, 0] and bool((u == 0).all())
