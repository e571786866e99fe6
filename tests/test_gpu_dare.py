"""``mjb_lqr_dare`` on the GPU (``mt.solve_dare``).

The yardstick is never the kernel: the numpy restatement of ``tests/dare_common.py`` in long double is the truth, the same restatement
in float64 measures what float64 arithmetic alone loses, and every bound is 8 x that measure (floor 1e-13; 1e-11 against scipy's
``solve_discrete_are``).  Both values of every comparison go through ``tests.conftest.measured`` under ``dare/...``
(profiles/dare_parity_measured.json keeps the recorded pairs)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import dare_common as dc
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
    return {k: getattr(res, k).cpu().numpy() for k in ("X", "K", "status", "iters", "change")}


def _record(key, value, tol):
    measured(key, value, tol, "(8 x the float64 numpy restatement's own figure, with the floor)")


_REFERENCE = {}


def _case(name, make):
    """The five systems of a case, generated once and shared by the two layouts (left unchanged: each test works on a copy)."""
    if name not in _REFERENCE:
        _REFERENCE[name] = make(NB)
    return _REFERENCE[name]


# ---- 1. the restatement cases, five distinct systems per launch -----------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "strided_shared_cost"])
@pytest.mark.parametrize("name,make", dc.CASES, ids=[c[0] for c in dc.CASES])
def test_doubling_matches_the_restatement(ctx, name, make, layout):
    """dense: A, B, Q, R as [5, ...] tensors.  strided_shared_cost: Q, R passed once as their trailing block (the first system's, for
    all five) and A, B as non-contiguous leading-axis views (every second block of a [10, ...] tensor) - read in place."""
    import mujoco_template_amd as mt

    torch, _, data = ctx
    case = {k: v.copy() for k, v in _case(name, make).items()}
    if layout == "dense":
        res = mt.solve_dare(data, *(_dev(torch, case[k]) for k in "ABQR"))
    else:
        case["Q"] = np.broadcast_to(case["Q"][0], case["Q"].shape).copy()
        case["R"] = np.broadcast_to(case["R"][0], case["R"].shape).copy()
        wide = {}
        for k in "AB":
            w = torch.full((2 * NB,) + case[k].shape[1:], float("nan"), dtype=torch.float64, device="cuda")
            w[::2] = _dev(torch, case[k])
            wide[k] = w[::2]
            assert not wide[k].is_contiguous()
        res = mt.solve_dare(data, wide["A"], wide["B"], _dev(torch, case["Q"][0]), _dev(torch, case["R"][0]))
    nx, nu = case["A"].shape[1], case["B"].shape[2]
    assert res.X.shape == (NB, nx, nx) and res.K.shape == (NB, nu, nx) and res.status.shape == (NB,)
    dc.judge(case, _np(res), f"dare/{layout}/{name}", record=_record)


# ---- 2. the humanoid balance design ---------------------------------------------------------------------------------------------------
def test_humanoid_design_matches_the_restatement_and_scipy(ctx):
    """The fixture and two copies with Q scaled by 0.5 and 2: against the restatement, and against scipy.linalg.solve_discrete_are within
    8 x the float64 restatement's error against scipy (floor 1e-11); closed-loop spectral radius within 1e-6 of scipy's."""
    import mujoco_template_amd as mt
    from scipy.linalg import solve_discrete_are

    torch, _, data = ctx
    case = dc.humanoid_case((1.0, 0.5, 2.0))
    got = _np(mt.solve_dare(data, _dev(torch, case["A"][0]), _dev(torch, case["B"][0]), _dev(torch, case["Q"]), _dev(torch, case["R"][0])))
    _, f64 = dc.judge(case, got, "dare/humanoid", record=_record)
    A, B, R = case["A"][0], case["B"][0], case["R"][0]
    P = np.stack([solve_discrete_are(A, B, case["Q"][e], R) for e in range(3)])
    Ks = np.stack([np.linalg.solve(R + B.T @ P[e] @ B, B.T @ P[e] @ A) for e in range(3)])
    for key, ref in (("X", P), ("K", Ks)):
        mine, np64 = dc.rel_err(got[key], ref), dc.rel_err(np.stack([f[key] for f in f64]), ref)
        print(f"humanoid {key} vs scipy: kernel {mine:.2e}  float64 numpy {np64:.2e}")
        measured(f"dare/humanoid/{key}_vs_scipy", mine, dc.bound(np64, dc.FLOOR_DARE), f"(float64 numpy restatement: {np64:.3e})")
    rho = lambda K: np.abs(np.linalg.eigvals(A - B @ K)).max()
    for e in range(3):
        measured(f"dare/humanoid/closed_loop_radius_{e}", abs(rho(got["K"][e]) - rho(Ks[e])), 1e-6)


# ---- 3. statuses and isolation ----------------------------------------------------------------------------------------------------------
def test_failures_are_reported_not_propagated(ctx):
    import mujoco_template_amd as mt

    torch, _, data = ctx
    dc.check_statuses(lambda case, max_iter: _np(mt.solve_dare(data, *(_dev(torch, case[k]) for k in "ABQR"), max_iter=max_iter)), "gpu")


def test_results_do_not_depend_on_the_batch_position(ctx):
    """(16, 9), k_lqr_dare<1, 32>: five systems in one launch against each system launched alone, every output bit for bit."""
    import mujoco_template_amd as mt

    torch, _, data = ctx
    case = _case("gen16x9", lambda n: dc.generator_case(16, 9, n))
    got = _np(mt.solve_dare(data, *(_dev(torch, case[k]) for k in "ABQR")))
    assert got["status"].tolist() == [0] * NB and np.abs(got["K"]).max() > 0
    for e in range(NB):
        alone = _np(mt.solve_dare(data, *(_dev(torch, case[k][e:e + 1]) for k in "ABQR")))
        for key in ("X", "K", "change", "iters", "status"):
            assert np.array_equal(got[key][e:e + 1], alone[key]), (e, key)


# ---- 4. the per-environment pipeline ----------------------------------------------------------------------------------------------------
def test_per_environment_design_stays_on_the_device():
    """set_env_params (a different body_mass per environment) -> linearize_rollout(T = 1) at the upright state -> solve_dare on the
    [:, 0] views in place: each K[e] against scipy on that environment's (A, B) copied to the host; the eight gains differ pairwise."""
    import torch
    from scipy.linalg import solve_discrete_are

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
    res = mt.solve_dare(data, Av, Bv, Q, R)
    got = _np(res)
    assert got["status"].tolist() == [0] * B
    Ah, Bh, Qh, Rh = Av.cpu().numpy(), Bv.cpu().numpy(), Q.cpu().numpy(), R.cpu().numpy()
    Ks, K64 = [], []
    for e in range(B):
        P = solve_discrete_are(Ah[e], Bh[e], Qh, Rh)
        Ks.append(np.linalg.solve(Rh + Bh[e].T @ P @ Bh[e], Bh[e].T @ P @ Ah[e]))
        K64.append(dc.restate(Ah[e], Bh[e], Qh, Rh, np.float64)["K"])
    mine, np64 = dc.rel_err(got["K"], np.stack(Ks)), dc.rel_err(np.stack(K64), np.stack(Ks))
    print(f"cart-pole per-environment K vs scipy: kernel {mine:.2e}  float64 numpy {np64:.2e}")
    measured("dare/cartpole_env_params/K_vs_scipy", mine, dc.bound(np64, dc.FLOOR_DARE), f"(float64 numpy restatement: {np64:.3e})")
    for a in range(B):
        for b in range(a + 1, B):
            assert not np.array_equal(got["K"][a], got["K"][b]), (a, b)


# ---- 5. argument checks -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_leave_the_outputs_alone(ctx):
    import mujoco_template_amd as mt
    from mujoco_template_amd.exceptions import ConfigError

    torch, _, data = ctx
    case = dc.generator_case(4, 1, 3)
    A, B, Q, R = (_dev(torch, case[k]) for k in "ABQR")
    with pytest.raises(ConfigError):
        mt.solve_dare(data, A.float(), B, Q, R)                                  # wrong dtype
    with pytest.raises(ConfigError):
        mt.solve_dare(data, A, B.cpu(), Q, R)                                    # a CPU tensor
    with pytest.raises(ConfigError):
        mt.solve_dare(data, A, B[:2], Q, R)                                      # mismatched nb
    big = torch.eye(65, dtype=torch.float64, device="cuda")
    with pytest.raises(ConfigError):
        mt.solve_dare(data, big, big[:, :1].contiguous(), big, R[0])             # nx = 65
    with pytest.raises(ConfigError):
        mt.solve_dare(data, A, B, Q, R, max_iter=0)
    # the C entry point itself: rejected before anything is launched, the outputs keep their contents
    X = torch.full((3, 4, 4), -77.0, dtype=torch.float64, device="cuda")
    K = torch.full((3, 1, 4), -77.0, dtype=torch.float64, device="cuda")
    change = torch.full((3,), -77.0, dtype=torch.float64, device="cuda")
    iters, status = (torch.full((3,), -77, dtype=torch.int32, device="cuda") for _ in range(2))
    arrays = {"A": (A.data_ptr(), 0, 16), "B": (B.data_ptr(), 0, 4), "Q": (Q.data_ptr(), 0, 16), "R": (R.data_ptr(), 0, 1)}
    ptrs = {"X": X.data_ptr(), "K": K.data_ptr(), "change": change.data_ptr(), "iters": iters.data_ptr(), "status": status.data_ptr()}
    good = {"batch": 3, "nx": 4, "nu": 1, "max_iter": 32, "tol": 1e-12}
    # batch 2^30: every array would end far beyond its allocation (torch's allocator hands out parts of larger blocks, so one
    # problem too many may still lie inside the block behind the pointer)
    for bad in ({"max_iter": 0}, {"max_iter": 65}, {"tol": -1.0}, {"batch": 1 << 30}, {"nx": 65}, {"nu": 0}):
        with pytest.raises(ConfigError):
            data.sim.lqr_dare({**good, **bad}, arrays, ptrs)
    with pytest.raises(ConfigError):
        data.sim.lqr_dare(good, {**arrays, "A": (A.data_ptr(), 0, -16)}, ptrs)
    with pytest.raises(ConfigError):
        data.sim.lqr_dare(good, arrays, {**ptrs, "status": 0})
    torch.cuda.synchronize()
    for t in (X, K, change):
        assert bool((t == -77.0).all())
    assert bool((iters == -77).all()) and bool((status == -77).all())
    data.sim.lqr_dare(good, arrays, ptrs)                                        # and the same call, well-formed, runs
    assert status.tolist() == [0, 0, 0]
