"""``solve_kalman`` on the GPU: the steady-state Kalman predictor gain as the dual of ``solve_dare`` on ``mjb_lqr_dare``, against
``scipy.linalg.solve_discrete_are`` with the bound tests/test_gpu_dare.py uses for the same kernel against scipy: 8 x the error of the
float64 numpy restatement of the doubling algorithm against scipy, floor 1e-11 (``dare_common.bound(np64, FLOOR_DARE)``)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import dare_common as dc  # noqa: E402
from tests import kalman_common as kc  # noqa: E402
from tests.conftest import MODELS, measured  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    import torch

    from mujoco_template_amd import mj

    model = mj.MjModel.from_xml_path(MODELS["cartpole"])
    return torch, mj.MjData(model, batch=1, dtype="float64")


def _dev(torch, x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")


_REFERENCE = {}


def _reference(nx, ny, shared_c):
    """Systems, scipy's (P, L) and the float64 restatement's (P, L): computed once per shape, left unchanged."""
    key = (nx, ny, shared_c)
    if key not in _REFERENCE:
        s = kc.systems(nx, ny)
        if shared_c:
            s["C"] = np.broadcast_to(s["C"][0], s["C"].shape).copy()
        ref = [kc.scipy_kalman(s["A"][e], s["C"][e], s["W"][e], s["V"][e]) for e in range(kc.NB)]
        f64 = [dc.restate(s["A"][e].T.copy(), s["C"][e].T.copy(), s["W"][e], s["V"][e], np.float64) for e in range(kc.NB)]
        assert all(f["status"] == 0 for f in f64)
        _REFERENCE[key] = (s, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]),
                           np.stack([f["X"] for f in f64]), np.stack([f["K"].T for f in f64]))
    return _REFERENCE[key]


@pytest.mark.parametrize("shared_c", [False, True], ids=["per_system_C", "shared_C"])
@pytest.mark.parametrize("nx,ny", kc.SIZES)
def test_solve_kalman_matches_scipy(ctx, nx, ny, shared_c):
    import mujoco_template_amd as mt

    torch, data = ctx
    s, P, L, P64, L64 = _reference(nx, ny, shared_c)
    C = _dev(torch, s["C"][0] if shared_c else s["C"])
    A = _dev(torch, s["A"])
    res = mt.solve_kalman(data, A, C, _dev(torch, s["W"]), _dev(torch, s["V"]))
    assert tuple(res.P.shape) == (kc.NB, nx, nx) and tuple(res.L.shape) == (kc.NB, nx, ny)
    assert res.status.cpu().tolist() == [0] * kc.NB
    for key, got, ref, f64 in (("P", res.P, P, P64), ("L", res.L, L, L64)):
        mine, np64 = dc.rel_err(got.cpu().numpy(), ref), dc.rel_err(f64, ref)
        print(f"kalman {nx}x{ny} {key}: kernel {mine:.2e}  float64 numpy {np64:.2e}  bound {dc.bound(np64, dc.FLOOR_DARE):.2e}")
        measured(f"kalman/{nx}x{ny}/{'shared' if shared_c else 'own'}/{key}", mine, dc.bound(np64, dc.FLOOR_DARE),
                 f"(float64 numpy restatement against scipy: {np64:.3e})")
    # the predictor's error dynamics A - L C: the poles of A' - C' L'
    poles = mt.closed_loop_poles(data, A.mT, C.mT, res.L.mT)
    assert poles.status.cpu().tolist() == [0] * kc.NB and bool((poles.rho < 1).all()), poles.rho


def test_undetectable_pair_fails_alone(ctx):
    """A = diag(1.1, 0.5), C = [0, 1]: the unstable mode is not seen.  status != 0 and zeros; the neighbour is bitwise what it is alone."""
    import mujoco_template_amd as mt

    torch, data = ctx
    A = _dev(torch, np.stack([np.diag([1.1, 0.5]), np.array([[1.1, 0.0], [0.2, 0.5]])]))
    C = _dev(torch, np.array([[0.0, 1.0]]))
    W, V = _dev(torch, np.eye(2)), _dev(torch, np.eye(1))
    res = mt.solve_kalman(data, A, C, W, V)
    alone = mt.solve_kalman(data, A[1:], C, W, V)
    status = res.status.cpu().tolist()
    assert status[0] != 0 and status[1] == 0 and alone.status.cpu().tolist() == [0]
    assert not bool(res.P[0].any()) and not bool(res.L[0].any())
    assert torch.equal(res.P[1], alone.P[0]) and torch.equal(res.L[1], alone.L[0])
