"""``mjb_lqr_dlyap`` on the GPU (``mt.closed_loop_cost``).

The yardstick is never the kernel: the numpy restatement of ``tests/dlyap_common.py`` in long double is the truth, the same restatement
in float64 measures what float64 arithmetic alone loses, and every bound is 8 x that measure (floor 1e-13; 1e-11 against scipy's
``solve_discrete_lyapunov``).  Both values of every comparison go through ``tests.conftest.measured`` under ``dlyap/...``
(profiles/dlyap_parity_measured.json keeps the recorded pairs)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import dare_common as dc
from tests import dlyap_common as lc
from tests.conftest import MODELS, measured

pytestmark = pytest.mark.gpu

NB = 5


@pytest.fixture(scope="module")
def ctx():
    import torch

    from mujoco_template_amd import mj

    model = mj.MjModel.from_xml_path(MODELS["cartpole"])
    data = mj.MjData(model, batch=1, dtype="float64")
    return torch, model, data


def _dev(torch, x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")


def _np(res):
    return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in ("P", "J", "status", "iters", "change")}


def _record(key, value, tol):
    measured(key, value, tol, "(8 x the float64 numpy restatement's own figure, with the floor)")


def _solve(torch, data, case, **kw):
    """Dense [n, ...] tensors of whatever the case holds."""
    import mujoco_template_amd as mt

    t = {k: _dev(torch, case[k]) for k in ("A", "B", "K", "Q", "R", "x0") if case.get(k) is not None}
    return _np(mt.closed_loop_cost(data, t["A"], t.get("B"), t.get("K"), Q=t["Q"], R=t.get("R"), x0=t.get("x0"), **kw))


# ---- 1. the restatement cases, five distinct systems per launch -----------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "strided_shared_gain", "strided_own_gain"])
@pytest.mark.parametrize("name,make", lc.CASES, ids=[c[0] for c in lc.CASES])
def test_smith_iteration_matches_the_restatement(ctx, name, make, layout):
    """dense: A, B, K, Q, R, x0 as [5, ...] tensors.  The strided layouts: A, B as non-contiguous leading-axis views (every second block
    of a NaN-filled [10, ...] tensor) and Q, R passed once as their trailing block (the first system's, for all five), read in place.
    strided_shared_gain passes K once as well: the first system's gain stabilises its own system and next to none of the others
    (spectral radii up to 3.6), so the float64 restatement says which problems end with status 2 - these must show it, NaN and +inf
    beside a problem 0 that is compared as usual.  strided_own_gain passes each system's own K [5, nu, nx]: all five are compared."""
    import mujoco_template_amd as mt

    torch, _, data = ctx
    case = lc.gain_case(name, make, NB)
    nx, nu = case["A"].shape[1], case["B"].shape[2]
    if layout == "dense":
        got = _solve(torch, data, case)
    else:
        case["Q"] = np.broadcast_to(case["Q"][0], case["Q"].shape).copy()
        case["R"] = np.broadcast_to(case["R"][0], case["R"].shape).copy()
        if layout == "strided_shared_gain":
            case["K"] = np.broadcast_to(case["K"][0], case["K"].shape).copy()
        wide = {}
        for k in "AB":
            w = torch.full((2 * NB,) + case[k].shape[1:], float("nan"), dtype=torch.float64, device="cuda")
            w[::2] = _dev(torch, case[k])
            wide[k] = w[::2]
            assert not wide[k].is_contiguous()
        K = _dev(torch, case["K"][0] if layout == "strided_shared_gain" else case["K"])
        res = mt.closed_loop_cost(data, wide["A"], wide["B"], K, Q=_dev(torch, case["Q"][0]), R=_dev(torch, case["R"][0]), x0=_dev(torch, case["x0"]))
        assert res.P.shape == (NB, nx, nx) and res.J.shape == (NB,) and res.status.shape == (NB,)
        got = _np(res)
    lc.judge(case, got, f"dlyap/{layout}/{name}", record=_record, shared_gain=layout == "strided_shared_gain")


# ---- 2. the humanoid balance design ---------------------------------------------------------------------------------------------------
def test_humanoid_policy_evaluation_is_the_dare_solution(ctx):
    """The fixture and two copies with Q scaled by 0.5 and 2, each with the gain of the float64 DARE restatement (A, B, R shared, read
    once): two closed-loop modes of modulus 1 that S does not see, so the stop must be at the FIRST change <= tol - iteration 19 for all
    three.  Truth: the long-double DARE solution (policy evaluation of the optimal gain is X); against scipy's solve_discrete_lyapunov,
    itself 1e-10 off, within 8 x the float64 restatement's distance from scipy (floor 1e-11).
    The float64 restatement is 3.1e-14 and 2.4e-14 from that truth for Q x 1 and x 0.5 but 3.4e-10 for Q x 2 (with a Lyapunov
    residual of 2.3e-15: the distance is that of the float64 DARE gain's own P from X on the marginal modes, not rounding of this
    iteration); each copy is judged against its own bound, and the kernel measured 3.4e-10 on the third as well."""
    import mujoco_template_amd as mt
    from scipy.linalg import solve_discrete_lyapunov

    torch, _, data = ctx
    case = lc.humanoid_case((1.0, 0.5, 2.0))
    res = mt.closed_loop_cost(data, _dev(torch, case["A"][0]), _dev(torch, case["B"][0]), _dev(torch, case["K"]), Q=_dev(torch, case["Q"]),
                              R=_dev(torch, case["R"][0]), x0=_dev(torch, case["x0"]))
    got = _np(res)
    f64 = []
    for e, scale in enumerate(("1", "0.5", "2")):                 # each copy against its own bound
        one = lambda d: {k: None if v is None else v[e:e + 1] for k, v in d.items()}
        f64 += lc.judge(one(case), one(got), f"dlyap/humanoid/Qx{scale}", record=_record, truth_P=case["X"][e:e + 1])
    assert got["iters"].tolist() == [19, 19, 19] == [f["iters"] for f in f64]
    Ps = []
    for e in range(3):
        M, S = lc.closed_loop(case["A"][e], case["B"][e], case["K"][e], case["Q"][e], case["R"][e], np.float64)
        Ps.append(solve_discrete_lyapunov(M.T, S))
    mine, np64 = lc.rel_err(got["P"], np.stack(Ps)), lc.rel_err(np.stack([f["P"] for f in f64]), np.stack(Ps))
    print(f"humanoid P vs scipy: kernel {mine:.2e}  float64 numpy {np64:.2e}")
    measured("dlyap/humanoid/P_vs_scipy", mine, lc.bound(np64, lc.FLOOR_DARE), f"(float64 numpy restatement: {np64:.3e})")


# ---- 3. the Gramian form, the optional arguments, the sign ----------------------------------------------------------------------------
def test_gramian_form_and_optional_arguments(ctx):
    """transpose on (12, 4), (17, 5) and at the edge sizes (16, 9) (the largest one-wave state) and (3, 9) (nu > nx) against the
    restatement; M = A alone; R absent; feedback_sign=+1 with -K bitwise -1 with K; no x0: J is None."""
    torch, _, data = ctx
    for nx, nu in ((12, 4), (17, 5), (16, 9), (3, 9)):
        case = lc.gain_case(f"gen{nx}x{nu}", lambda n: dc.generator_case(nx, nu, n), NB)
        lc.judge(case, _solve(torch, data, case, transpose=True), f"dlyap/gramian/gen{nx}x{nu}", record=_record, transpose=True)
    case = lc.gain_case("gen17x5", lambda n: dc.generator_case(17, 5, n), NB)
    alone = {"A": 0.9 * case["A"], "Q": case["Q"], "x0": case["x0"]}
    lc.judge(alone, _solve(torch, data, alone), "dlyap/open_loop/gen17x5", record=_record)
    no_r = {k: v for k, v in case.items() if k != "R"}
    lc.judge(no_r, _solve(torch, data, no_r), "dlyap/no_R/gen17x5", record=_record)
    minus, plus = _solve(torch, data, case), _solve(torch, data, {**case, "K": -case["K"]}, feedback_sign=+1)
    for key in ("P", "J", "change", "iters", "status"):
        assert np.array_equal(minus[key], plus[key]), key
    assert _solve(torch, data, {k: v for k, v in case.items() if k != "x0"})["J"] is None


# ---- 4. statuses and isolation ----------------------------------------------------------------------------------------------------------
def test_failures_are_reported_not_propagated(ctx):
    torch, _, data = ctx
    lc.check_statuses(lambda case, max_iter: _solve(torch, data, case, max_iter=max_iter), "gpu")


def test_results_do_not_depend_on_the_batch_position(ctx):
    """(16, 9), the largest one-wave state: five systems in one launch against each system launched alone, every output bit for bit."""
    torch, _, data = ctx
    case = lc.gain_case("gen16x9", lambda n: dc.generator_case(16, 9, n), NB)
    got = _solve(torch, data, case)
    assert got["status"].tolist() == [0] * NB and np.isfinite(got["P"]).all()
    for e in range(NB):
        alone = _solve(torch, data, {k: v[e:e + 1] for k, v in case.items()})
        for key in ("P", "J", "change", "iters", "status"):
            assert np.array_equal(got[key][e:e + 1], alone[key]), (e, key)


# ---- 5. properties whose bounds are derived -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu", [(12, 4), (17, 5)])
def test_policy_evaluation_of_the_optimal_gain_and_of_a_worse_one(ctx, nx, nu):
    """(a) closed_loop_cost(A, B, sol.K).P is solve_dare's X.  Both kernels carry their own rounding, so the bound is that of the sum of
    the two float64 restatements' errors against the long-double DARE solution (8 x, floor 1e-13) - the error of sol.K itself enters P
    only in second order, K being the minimiser.
    (b) For K perturbed by 5 % (every closed loop stays stable), P - X is positive semi-definite in exact arithmetic.  Computed P and X
    are off by at most eP max|P| and eX max|X| entrywise (the bounds of the two restatements), a symmetric perturbation E moves an
    eigenvalue by at most ||E||_2 <= nx max|E| (Weyl), so lambda_min(P - X) >= -nx (eP max|P| + eX max|X|)."""
    import mujoco_template_amd as mt

    torch, _, data = ctx
    case = lc.gain_case(f"gen{nx}x{nu}", lambda n: dc.generator_case(nx, nu, n), NB)
    A, B, Q, R = (_dev(torch, case[k]) for k in "ABQR")
    sol = mt.solve_dare(data, A, B, Q, R)
    res = mt.closed_loop_cost(data, A, B, sol.K, Q=Q, R=R)
    assert sol.status.tolist() == [0] * NB and res.status.tolist() == [0] * NB
    X, P = sol.X.cpu().numpy(), res.P.cpu().numpy()
    sys_ = [tuple(case[k][e] for k in "ABQR") for e in range(NB)]
    Xt = np.stack([dc.truth(*s)["X"] for s in sys_])
    eX = lc.rel_err(np.stack([dc.restate(*s, np.float64)["X"] for s in sys_]), Xt)
    eP = lc.rel_err(np.stack([lc.restate(s[0], s[1], case["K"][e], s[2], s[3], np.float64)["P"] for e, s in enumerate(sys_)]), Xt)
    mine = lc.rel_err(P, X)
    print(f"gen{nx}x{nu} P(sol.K) vs X: kernels {mine:.2e}  float64 numpy {eX:.2e} + {eP:.2e}")
    measured(f"dlyap/optimal_gain/gen{nx}x{nu}/P_vs_X", mine, lc.bound(eX + eP), "(8 x the sum of the two float64 restatements' errors)")

    Kp = case["K"] * (1.0 + 0.05 * np.random.default_rng(11).normal(size=case["K"].shape))
    worse = mt.closed_loop_cost(data, A, B, _dev(torch, Kp), Q=Q, R=R)
    assert worse.status.tolist() == [0] * NB
    Pw = worse.P.cpu().numpy()
    Pt = np.stack([lc.truth(s[0], s[1], Kp[e], s[2], s[3])["P"] for e, s in enumerate(sys_)])
    ePw = lc.rel_err(np.stack([lc.restate(s[0], s[1], Kp[e], s[2], s[3], np.float64)["P"] for e, s in enumerate(sys_)]), Pt)
    for e in range(NB):
        lam = float(np.linalg.eigvalsh(Pw[e] - X[e]).min()) / np.abs(X[e]).max()
        allowed = nx * (lc.bound(ePw) * np.abs(Pw[e]).max() + lc.bound(eX) * np.abs(X[e]).max()) / np.abs(X[e]).max()
        print(f"gen{nx}x{nu} [{e}] lambda_min(P - X) / max|X| = {lam:.2e}  allowed >= {-allowed:.2e}")
        measured(f"dlyap/worse_gain/gen{nx}x{nu}/minus_lambda_min_{e}", -lam, allowed, "(nx x the two entrywise bounds: Weyl)")


# ---- 6. the per-environment pipeline ----------------------------------------------------------------------------------------------------
def test_nominal_gain_is_priced_on_every_environment():
    """set_env_params (body_mass scaled 0.6 .. 1.6) -> linearize_rollout(T = 1) -> solve_dare per environment -> the gain of environment
    0, shared as [nu, nx], against every (A_e, B_e): closed_loop_poles and closed_loop_cost on the [:, 0] views in place.  Where the
    nominal gain stabilises (rho < 1; environment 0 at least) the status is 0 and J agrees with scipy.linalg.solve_discrete_lyapunov on
    the downloaded matrices within 8 x the float64 restatement's distance from scipy (floor 1e-11); elsewhere J is +inf.  J_nominal /
    J_optimal >= 1 - b and, for environment 0, |ratio - 1| <= b: each J carries a relative error of at most the bound of the float64
    restatement's J against the long-double one, and two relative errors add in a quotient, so b is twice that bound."""
    import torch
    from scipy.linalg import solve_discrete_lyapunov

    import mujoco_template_amd as mt
    from mujoco_template_amd import mj

    B = 8
    model = mj.MjModel.from_xml_path(MODELS["cartpole"])
    data = mj.MjData(model, batch=B, dtype="float64")
    cm = data.sim.model.compiled
    nq, nv, nu = int(cm.nq), int(cm.nv), int(cm.nu)
    mass = np.asarray(cm.body_mass, dtype=np.float64)[None] * np.linspace(0.6, 1.6, B)[:, None]
    data.sim.set_env_params(body_mass=mass)
    x0 = torch.zeros(1 + nq + nv, dtype=torch.float64, device="cuda")
    u0 = torch.zeros((B, 1, nu), dtype=torch.float64, device="cuda")
    _, _, A, Bm = mt.linearize_rollout(model, data, u0, initial_state=x0)
    Av, Bv = A[:, 0], Bm[:, 0]
    Q = torch.diag(torch.tensor([0.5, 10.0, 0.05, 0.1], dtype=torch.float64, device="cuda"))
    R = 0.01 * torch.eye(nu, dtype=torch.float64, device="cuda")
    dx0 = torch.tensor([0.1, 0.05, -0.2, 0.3], dtype=torch.float64, device="cuda")
    sol = mt.solve_dare(data, Av, Bv, Q, R)
    K0 = sol.K[0]                                                 # [nu, nx]: read once for every environment
    poles = mt.closed_loop_poles(data, Av, Bv, K0)
    nominal = mt.closed_loop_cost(data, Av, Bv, K0, Q=Q, R=R, x0=dx0)
    optimal = mt.closed_loop_cost(data, Av, Bv, sol.K, Q=Q, R=R, x0=dx0)
    assert sol.status.tolist() == [0] * B and poles.status.tolist() == [0] * B and optimal.status.tolist() == [0] * B
    rho, st = poles.rho.cpu().numpy(), nominal.status.cpu().numpy()
    print("rho of the nominal gain per environment:", rho, "status:", st)
    assert rho[0] < 1 and st.tolist() == [0 if r < 1 else 2 for r in rho]
    Ah, Bh, Kh, Qh, Rh, xh = (t.cpu().numpy() for t in (Av, Bv, sol.K, Q, R, dx0))
    Jn, Jo = nominal.J.cpu().numpy(), optimal.J.cpu().numpy()
    ok = [e for e in range(B) if st[e] == 0]
    assert np.isinf(Jn[[e for e in range(B) if st[e] != 0]]).all()
    worst = worst64 = rel64 = 0.0
    for e in ok:
        for K, J in ((Kh[0], Jn[e]), (Kh[e], Jo[e])):
            M, S = lc.closed_loop(Ah[e], Bh[e], K, Qh, Rh, np.float64)
            Js = xh @ solve_discrete_lyapunov(M.T, S) @ xh
            f64 = lc.restate(Ah[e], Bh[e], K, Qh, Rh, np.float64, x0=xh)
            tr = lc.truth(Ah[e], Bh[e], K, Qh, Rh, x0=xh)
            assert f64["status"] == 0 and tr["status"] == 0
            worst, worst64 = max(worst, abs(J - Js) / abs(Js)), max(worst64, abs(f64["J"] - Js) / abs(Js))
            rel64 = max(rel64, float(abs(f64["J"] - tr["J"]) / abs(tr["J"])))
    print(f"cart-pole J vs scipy: kernel {worst:.2e}  float64 numpy {worst64:.2e}")
    measured("dlyap/cartpole_env_params/J_vs_scipy", worst, lc.bound(worst64, lc.FLOOR_DARE), f"(float64 numpy restatement: {worst64:.3e})")
    b = 2.0 * lc.bound(rel64)
    ratio = Jn[ok] / Jo[ok]
    print("J_nominal / J_optimal:", ratio, "b:", b)
    measured("dlyap/cartpole_env_params/one_minus_ratio", float((1.0 - ratio).max()), b, "(twice the bound of J)")
    measured("dlyap/cartpole_env_params/ratio_env0", abs(float(ratio[0]) - 1.0), b, "(twice the bound of J)")
    assert len(ok) >= 2 and bool((ratio[1:] > 1.0).any())           # other models: the nominal gain costs more somewhere


# ---- 7. argument checks -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_leave_the_outputs_alone(ctx):
    import mujoco_template_amd as mt
    from mujoco_template_amd.exceptions import ConfigError

    torch, _, data = ctx
    case = lc.gain_case("gen4x1", lambda n: dc.generator_case(4, 1, n), 3)
    A, B, K, Q, R, x0 = (_dev(torch, case[k]) for k in ("A", "B", "K", "Q", "R", "x0"))
    big = torch.eye(65, dtype=torch.float64, device="cuda")
    bad_calls = [
        lambda: mt.closed_loop_cost(data, A.float(), B, K, Q=Q, R=R),              # wrong dtype
        lambda: mt.closed_loop_cost(data, A, B.cpu(), K, Q=Q, R=R),                # a CPU tensor
        lambda: mt.closed_loop_cost(data, A, B[:2], K, Q=Q, R=R),                  # mismatched nb
        lambda: mt.closed_loop_cost(data, A, B, K, Q=Q, R=R, x0=x0[:2]),
        lambda: mt.closed_loop_cost(data, big, Q=big),                             # nx = 65
        lambda: mt.closed_loop_cost(data, A, B, Q=Q),                              # B without K
        lambda: mt.closed_loop_cost(data, A, None, K, Q=Q),
        lambda: mt.closed_loop_cost(data, A, Q=Q, R=R),                            # R without K
        lambda: mt.closed_loop_cost(data, A, B, K.transpose(1, 2), Q=Q, R=R),      # K of B's shape
        lambda: mt.closed_loop_cost(data, A, B, K, Q=Q[:, :, :3], R=R),            # Q not [nx, nx]
    ]
    for call in bad_calls:
        with pytest.raises(ConfigError):
            call()
    for kw in ({"max_iter": 0}, {"max_iter": 65}, {"max_iter": 1.5}, {"tol": -1.0}, {"tol": float("nan")}, {"feedback_sign": 0}, {"feedback_sign": True}):
        with pytest.raises(ConfigError):
            mt.closed_loop_cost(data, A, B, K, Q=Q, R=R, **kw)
    # the C entry point itself: rejected before anything is launched, the outputs keep their contents
    P = torch.full((3, 4, 4), -77.0, dtype=torch.float64, device="cuda")
    J, change = (torch.full((3,), -77.0, dtype=torch.float64, device="cuda") for _ in range(2))
    iters, status = (torch.full((3,), -77, dtype=torch.int32, device="cuda") for _ in range(2))
    arrays = {"A": (A.data_ptr(), 0, 16), "B": (B.data_ptr(), 0, 4), "K": (K.data_ptr(), 0, 4), "Q": (Q.data_ptr(), 0, 16), "R": (R.data_ptr(), 0, 1),
              "x0": (x0.data_ptr(), 0, 4)}
    ptrs = {"P": P.data_ptr(), "J": J.data_ptr(), "change": change.data_ptr(), "iters": iters.data_ptr(), "status": status.data_ptr()}
    good = {"batch": 3, "nx": 4, "nu": 1, "feedback_sign": -1, "transpose": 0, "max_iter": 64, "tol": 1e-12}
    # batch 2^30: every array would end far beyond its allocation (torch's allocator hands out parts of larger blocks, so one
    # problem too many may still lie inside the block behind the pointer)
    for bad in ({"max_iter": 0}, {"max_iter": 65}, {"tol": -1.0}, {"batch": 1 << 30}, {"batch": 0}, {"nx": 65}, {"nu": 0}, {"nu": 33}, {"feedback_sign": 0}):
        with pytest.raises(ConfigError):
            data.sim.lqr_dlyap({**good, **bad}, arrays, ptrs)
    none = (0, 0, 0)
    for bad in ({"A": (A.data_ptr(), 0, -16)}, {"x0": (x0.data_ptr(), 0, -4)},     # a negative stride
                {"K": none}, {"B": none},                                            # B without K, K without B
                {"B": none, "K": none},                                              # R without K
                {"Q": none}, {"A": none}):
        with pytest.raises(ConfigError):
            data.sim.lqr_dlyap(good, {**arrays, **bad}, ptrs)
    for bad in ({"J": 0}, {"status": 0}, {"iters": 0}, {"P": 0}):                    # x0 without J, NULL outputs
        with pytest.raises(ConfigError):
            data.sim.lqr_dlyap(good, arrays, {**ptrs, **bad})
    with pytest.raises(ConfigError):
        data.sim.lqr_dlyap(good, {**arrays, "x0": none}, ptrs)                       # J without x0
    torch.cuda.synchronize()
    for t in (P, J, change):
        assert bool((t == -77.0).all())
    assert bool((iters == -77).all()) and bool((status == -77).all())
    data.sim.lqr_dlyap(good, arrays, ptrs)                                           # and the same call, well-formed, runs
    assert status.tolist() == [0, 0, 0] and bool((J > 0).all())
    data.sim.lqr_dlyap(good, arrays, {**ptrs, "change": 0})                          # change is optional
    assert status.tolist() == [0, 0, 0]
